"""GPU: plain PointPillars on the HIP path — hvpr_pillar_vfe_plain_fwd_f32 against the reference's record (G28) and against float64
inside the derived bound of pointpillar_cases.py, BaseBEVBackbone and the detector against G28, the eager forward against the
hand-called chain, the captured graph, the config-size model, and the evaluate / demo commands on a four-frame KITTI tree."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import kitti_infos_cases as K
import pointpillar_cases as PC
from hvpr_amd import bev_backbone, config, detector, kernels, vfe
from hvpr_amd._lib import call
from hvpr_amd.voxel_generator import VoxelGenerator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(config.CFG_DIR, "kitti_models", "pointpillar.yaml")
VS, RNG = [0.16, 0.16, 3.0], [0, -19.84, -2.5, 47.36, 19.84, 0.5]          # make_golden.VOXEL_SIZE / PC_RANGE: G28's vfe cases
SENTINEL, TAIL = -7.5, 4096


@pytest.fixture(scope="module")
def g28():
    return np.load(PC.GOLDEN)


def _close(got, ref, rtol=1e-3):
    """The rule of tests/test_gpu_eval_fixtures.py."""
    ref = np.asarray(ref)
    rms = float(np.sqrt(np.mean(np.square(ref, dtype=np.float64))))
    np.testing.assert_allclose(np.asarray(got), ref, rtol=rtol, atol=rtol * max(rms, 1e-30))


def _kernel(vox, n, coords, w, b, vs, off, m_device=None):
    """One call of the entry point into buffers that end in a sentinel tail -> (features (M, C), mask (M, P)) on the host."""
    M, P, _ = vox.shape
    C = w.shape[0]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    out = torch.full((M * C + TAIL,), SENTINEL, device=DEV)
    mask = torch.full((M * P + TAIL,), SENTINEL, device=DEV)
    call("hvpr_pillar_vfe_plain_fwd_f32", t(vox, torch.float32), t(n, torch.int32), t(coords, torch.int32), M, P, m_device, float(vs[0]),
         float(vs[1]), float(vs[2]), float(off[0]), float(off[1]), float(off[2]), t(w, torch.float32), t(b, torch.float32), C, out, mask,
         kernels._stream())
    torch.cuda.synchronize()
    assert bool((out[M * C:] == SENTINEL).all()) and bool((mask[M * P:] == SENTINEL).all()), "written past an output"
    return out[:M * C].view(M, C).cpu().numpy(), mask[:M * P].view(M, P).cpu().numpy()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("tag", ["A", "B"])
def test_kernel_against_the_reference_record(g28, tag, observed):
    """G28(a) through the module (its fold) and the wrapper: the standing bar of test_vfe_golden_fixture, rtol 1e-3 / atol 1e-4, the
    mask exactly."""
    z, p = g28, f"vfe.{tag}."
    m = vfe.PillarVFE(PC.vfe_cfg(NUM_FILTERS=[int(v) for v in z[p + "num_filters"]]), 4, VS, RNG)
    PC.load_det(m, PC.recorded_shapes(z, f"vfe.{tag}"), int(z[p + "param_seed"]))
    m = m.to(DEV).eval()
    with torch.no_grad():
        d = m({"voxels": torch.from_numpy(z[p + "voxels"]).to(DEV), "voxel_num_points": torch.from_numpy(z[p + "voxel_num_points"]).to(DEV),
               "voxel_coords": torch.from_numpy(z[p + "voxel_coords"]).to(DEV)})
    got, ref = d["pillar_features"].cpu().numpy(), z[p + "pillar_features"]
    observed(f"G28 vfe.{tag} on the HIP path: max |diff| {np.abs(got - ref).max():.2e} (bar rtol 1e-3, atol 1e-4)")
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-4)
    assert d["pillar_mask"].shape == z[p + "pillar_mask"].shape
    np.testing.assert_array_equal(d["pillar_mask"].cpu().numpy(), z[p + "pillar_mask"])


SHAPES = [(1, 32, 64), (2, 32, 64), (2, 20, 32), (37, 1, 32), (37, 1, 128), (133, 20, 64), (133, 20, 128), (133, 32, 32), (133, 32, 128),
          (40000, 32, 64)]


@pytest.mark.parametrize("M,P,c_out", SHAPES, ids=str)
def test_kernel_against_float64_inside_the_derived_bound(M, P, c_out, observed):
    """Element by element |kernel - float64| <= bound, the bound of pointpillar_cases.py: u = 2^-24 times the magnitudes that enter
    each rounding — gamma(P) A_j / n for the mean (P - 1 additions and the quotient), (1 + u) E + u |difference| for each of the two
    subtractions (the centre's product and sum add gamma(2) (|cell vs| + |off|)), gamma(11) over the bias and the ten products of the
    layer plus the features' own errors through |w| — carried through relu and the maximum over the slots, both 1-Lipschitz, as the
    largest slot bound.  No constant is fitted and no element excluded.  M = 1; M = 2 is n = 1 and n = P; P = 1, 20, 32; every
    width; M = 40 000 is more rows than the grid's waves take in one pass (the strided walk).  The mask is exact."""
    nx, ny = 296, 248
    vox, n, coords = PC.synth_pillars(1000 + M + P, M, P, VS, RNG, nx, ny)
    if M == 2:
        assert n.tolist() == [1, P]
    w, b = PC.folded_layer(M + c_out, c_out)
    off = PC.offsets_of(VS, RNG)
    got, mask = _kernel(vox, n, coords, w, b, VS, off)
    assert np.isfinite(got).all()
    r = PC.pfn64(vox, n, coords, w, b, VS, off)
    frac = PC.used_fraction(got, r)
    observed(f"pillar encoder {(M, P, c_out)}: max err / bound {frac:.4f}")
    assert frac <= 1.0, ((M, P, c_out), frac)
    np.testing.assert_array_equal(mask, r["mask"].astype(np.float32))


def test_kernel_reads_the_live_row_count_from_the_device():
    M, P, c_out, count = 90, 32, 64, 41
    vox, n, coords = PC.synth_pillars(77, M, P, VS, RNG, 296, 248)
    w, b = PC.folded_layer(3, c_out)
    off = PC.offsets_of(VS, RNG)
    r = PC.pfn64(vox, n, coords, w, b, VS, off)
    md = torch.tensor([count], dtype=torch.int32, device=DEV)
    got, mask = _kernel(vox, n, coords, w, b, VS, off, m_device=md)
    assert (np.abs(got[:count] - r["out"][:count]) <= r["bound"][:count]).all()          # rows at or past the count are unspecified
    np.testing.assert_array_equal(mask[:count], r["mask"][:count].astype(np.float32))
    _kernel(vox, n, coords, w, b, VS, off, m_device=torch.zeros(1, dtype=torch.int32, device=DEV))      # a count of 0: nothing to do
    pf, mk = kernels.pillar_vfe_plain_fwd(torch.from_numpy(vox).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(coords).to(DEV),
                                          torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), VS, off, m_device=md, want_mask=False)
    assert mk is None and np.array_equal(pf[:count].cpu().numpy(), got[:count])
    empty = kernels.pillar_vfe_plain_fwd(torch.zeros((0, P, 4), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                         torch.zeros((0, 4), dtype=torch.int32, device=DEV), torch.from_numpy(w).to(DEV),
                                         torch.from_numpy(b).to(DEV), VS, off)
    assert empty[0].shape == (0, c_out) and empty[1].shape == (0, P, 1)


# ------------------------------------------------------------------------------------------------ the backbone
@pytest.mark.parametrize("algo", [None, "direct"])
@pytest.mark.parametrize("tag", ["small", "full"])
def test_backbone_against_the_reference_record(g28, tag, algo, observed, monkeypatch):
    z, p = g28, f"bev.{tag}."
    if algo is None:
        monkeypatch.delenv("HVPR_CONV_ALGO", raising=False)
    else:
        monkeypatch.setenv("HVPR_CONV_ALGO", algo)
    shapes = PC.recorded_shapes(z, f"bev.{tag}")
    m = bev_backbone.BaseBEVBackbone(PC.backbone_cfg(LAYER_NUMS=[int(v) for v in z[p + "layer_nums"]],
                                                     LAYER_STRIDES=[int(v) for v in z[p + "layer_strides"]],
                                                     NUM_FILTERS=[shapes[f"blocks.{i}.1.weight"][0] for i in range(3)],
                                                     UPSAMPLE_STRIDES=[int(v) for v in z[p + "upsample_strides"]],
                                                     NUM_UPSAMPLE_FILTERS=[int(v) for v in z[p + "num_upsample_filters"]]),
                                     input_channels=z[p + "spatial_features"].shape[1])
    PC.load_det(m, shapes, int(z[p + "param_seed"]))
    m = m.to(DEV).eval()
    with torch.no_grad():
        d = m({"spatial_features": torch.from_numpy(z[p + "spatial_features"]).to(DEV).contiguous(memory_format=torch.channels_last)})
    kinds = {type(pc).__name__ for lv in m._fold.value.levels for pc in lv.trunk}
    assert kinds == ({"PackedConv"} if algo == "direct" else {"PackedConv", "PackedConvWino"}), kinds
    got, ref = d["spatial_features_2d"].cpu().numpy(), z[p + "spatial_features_2d"]
    assert got.shape == ref.shape and d["spatial_features_2d"].is_contiguous(memory_format=torch.channels_last)
    observed(f"G28 bev.{tag} [{algo or 'default'}]: max-norm error {np.abs(got - ref).max() / np.abs(ref).max():.2e} (element-wise bar 1e-3)")
    _close(got, ref)


# ------------------------------------------------------------------------------------------------ the detector
def test_detector_against_the_recorded_chain(g28, observed):
    z = g28
    cfg = PC.grid_cfg(z["chain.point_cloud_range"], z["chain.voxel_size"])
    model = PC.build_model(cfg, seed=9)
    assert list(model.dataset.grid_size[:2]) == [int(v) for v in z["chain.grid"]]
    PC.load_det(model, PC.recorded_shapes(z, "chain"), int(z["chain.param_seed"]))
    model = model.to(DEV).eval()
    batch = {"voxels": torch.from_numpy(z["chain.voxels"]).to(DEV), "voxel_num_points": torch.from_numpy(z["chain.voxel_num_points"]).to(DEV),
             "voxel_coords": torch.from_numpy(z["chain.voxel_coords"]).to(DEV), "batch_size": 2}
    with torch.no_grad():
        _, _, d = model(batch, sync=False)
    for key in ("batch_cls_preds", "batch_box_preds"):
        got, ref = d[key].cpu().numpy(), z["chain." + key]
        assert got.shape == ref.shape
        observed(f"G28 chain {key}: max-norm error {np.abs(got - ref).max() / np.abs(ref).max():.2e}")
        _close(got, ref)


def _points_batch(seeds, point_cloud_range, n=None):
    frames = [PC.frame_points(s, point_cloud_range, b) for b, s in enumerate(seeds)]
    if n is not None:
        assert all(len(f) >= n for f in frames)
        frames = [f[:n] for f in frames]
    return {"points": torch.from_numpy(np.concatenate(frames)).to(DEV), "batch_size": len(frames)}


@pytest.fixture(scope="module")
def tiny():
    cfg = PC.tiny_cfg()
    return cfg, PC.build_model(cfg, seed=0, cls_bias=-2.0, device=DEV)


def _snapshot(rec):
    n = int(rec["pred_count"].item())
    return {k: rec[k][:n].cpu().numpy().copy() for k in ("pred_boxes", "pred_scores", "pred_labels", "selected")}


def test_eager_forward_equals_the_chain_called_by_hand(tiny):
    cfg, model = tiny
    batch = _points_batch([11, 12], PC.TINY_RANGE)
    assert batch["points"].shape[0] > 1000
    with torch.no_grad():
        recs, _, d = model(dict(batch), sync=False)
        pts, B = batch["points"], 2
        vc = model._voxel_cfg()
        vg = VoxelGenerator(vc.VOXEL_SIZE, model.dataset.point_cloud_range, vc.MAX_POINTS_PER_VOXEL, vc.MAX_NUMBER_OF_VOXELS["test"], device=DEV)
        v, c, n, vo = vg.generate_batch(pts, kernels.frame_offsets(pts, B), B, xyz_col=1, n_feat=4)
        live = int(vo[B].item())
        assert 100 < live < v.shape[0]                             # the live row count matters: the buffers are longer
        md = vo[B:B + 1]
        f = model.vfe._build_folded()
        pf, mask = kernels.pillar_vfe_plain_fwd(v, n, c, f["w"], f["b"], model.vfe.voxel_size, model.vfe.offsets, m_device=md)
        nx, ny = [int(g) for g in model.dataset.grid_size[:2]]
        assert (nx, ny) == (64, 64)
        sp, _ = kernels.scatter_bev_fwd(pf, None, None, c, B, nx, ny, kernels.scatter_workspace(B, nx, ny, DEV), m_device=md)
        h = model.dense_head(model.backbone_2d({"spatial_features": sp, "batch_size": B}))
    assert torch.equal(d["pillar_features"][:live], pf[:live]) and torch.equal(d["pillar_mask"][:live], mask[:live])
    assert torch.equal(d["spatial_features"], sp)
    assert torch.equal(d["batch_cls_preds"], h["batch_cls_preds"]) and torch.equal(d["batch_box_preds"], h["batch_box_preds"])
    assert d["batch_cls_preds"].shape == (2, 32 * 32 * 6, 3) and sum(int(r["pred_count"].item()) for r in recs) > 0


def test_graph_replay_equals_the_eager_forward(tiny):
    cfg, model = tiny
    batches = [_points_batch([20 + i], PC.TINY_RANGE, n=1500) for i in range(3)]
    with torch.no_grad():
        want = [_snapshot(model(dict(b), sync=False)[0][0]) for b in batches]
    assert len(want[1]["selected"]) > 0 and not np.array_equal(want[1]["pred_boxes"], want[2]["pred_boxes"])
    graphed = detector.GraphedForward(model, batches[0])
    for b, w in zip(batches[1:], want[1:]):
        got = _snapshot(graphed(b)[0][0])
        for k in w:
            np.testing.assert_array_equal(got[k], w[k])
    graphed.check_status()
    model.load_state_dict(model.state_dict())                       # drops the folds the graph was captured on
    with pytest.raises(RuntimeError, match="capture a new graph"):
        graphed(batches[1])
    with torch.no_grad():                                           # the model itself goes on: it folds again
        again = _snapshot(model(dict(batches[1]), sync=False)[0][0])
    for k in again:
        np.testing.assert_array_equal(again[k], want[1][k])


def test_config_size_model_on_a_batch_of_two():
    cfg = config.pointpillar_cfg()
    model = PC.build_model(cfg, seed=0, cls_bias=-2.0, device=DEV)
    rng = cfg.DATA_CONFIG.POINT_CLOUD_RANGE
    post = int(cfg.MODEL.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE)
    both = _points_batch([31, 32], rng)
    with torch.no_grad():
        recs, _, d = model(dict(both), sync=False)
        singles = [model(_points_batch([s], rng), sync=False)[0][0] for s in (31, 32)]
    assert d["batch_cls_preds"].shape == (2, 321408, 3) and d["spatial_features_2d"].shape == (2, 384, 248, 216)
    assert bool(torch.isfinite(d["batch_cls_preds"]).all()) and bool(torch.isfinite(d["batch_box_preds"]).all())
    for rec, one in zip(recs, singles):
        a, b = _snapshot(rec), _snapshot(one)
        assert 0 < len(a["selected"]) <= post and np.isfinite(a["pred_boxes"]).all() and np.isfinite(a["pred_scores"]).all()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])


# ------------------------------------------------------------------------------------------------ the commands
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Two train and two val frames as a KITTI tree with its infos, and a random-weight checkpoint of pointpillar.yaml."""
    from hvpr_amd import kitti_dataset
    root = tmp_path_factory.mktemp("kitti_pp")
    train, _ = K.labelled_frames([3000] * 2, [4] * 2, seed=1)
    val, _ = K.labelled_frames([3000] * 2, [4] * 2, seed=2)
    for f in val:
        f["split"] = "val"
    K.write_tree(root, K.tree_files(train + val, {"train": [f["id"] for f in train], "val": [f["id"] for f in val], "test": []}))
    cfg = config.pointpillar_cfg()
    kitti_dataset.create_kitti_infos(cfg.DATA_CONFIG, ["Car", "Pedestrian", "Cyclist"], root, root, device=DEV)
    model = PC.build_model(cfg, seed=0, cls_bias=-2.0)
    torch.save({"model_state": model.state_dict()}, root / "checkpoint_epoch_80.pth")
    return {"root": root, "cfg": cfg, "model": model.to(DEV).eval(), "val": [f["id"] for f in val]}


def test_evaluate_command(scene, tmp_path):
    from hvpr_amd import evaluate
    root = scene["root"]
    res = evaluate.main(["--cfg_file", YAML, "--batch_size", "2", "--data_path", str(root), "--output_dir", str(tmp_path),
                         "--ckpt", str(root / "checkpoint_epoch_80.pth")])
    out = tmp_path / "pointpillar" / "default" / "eval" / "epoch_80" / "val" / "default"
    with open(out / "result.pkl", "rb") as f:
        annos = pickle.load(f)
    assert [a["frame_id"] for a in annos] == scene["val"] and sum(len(a["name"]) for a in annos) > 0
    metrics = json.load(open(out / "metrics.json"))
    assert metrics == {k: float(v) for k, v in res["80"].items()} and any(k.startswith("recall/rcnn_") for k in metrics)


def test_demo_command(scene, tmp_path):
    from hvpr_amd import demo
    root, model, cfg = scene["root"], scene["model"], scene["cfg"]
    data = root / "training" / "velodyne"
    entries = demo.main(["--cfg_file", YAML, "--data_path", str(data), "--ckpt", str(root / "checkpoint_epoch_80.pth"), "--output_dir",
                         str(tmp_path / "demo")])
    files = demo.list_files(data, ".bin")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    assert len(files) == 4 and sorted(p.name for p in (tmp_path / "demo").iterdir()) == sorted([s + ".png" for s in stems] + ["result.pkl"])
    with open(tmp_path / "demo" / "result.pkl", "rb") as f:
        stored = pickle.load(f)
    assert [e["frame_id"] for e in stored] == [e["frame_id"] for e in entries] == stems
    loader = demo.build_loader(cfg, files, ".bin", DEV)
    for i, e in enumerate(stored):
        with torch.no_grad():
            recs, _, _ = model(demo.prepare(loader, [i], 0), sync=True)
        assert e["boxes_lidar"].tobytes() == recs[0]["pred_boxes"].cpu().numpy().tobytes() and len(e["score"]) > 0
        assert e["score"].tobytes() == recs[0]["pred_scores"].cpu().numpy().tobytes()
        assert set(e["name"].tolist()) <= set(cfg.CLASS_NAMES)
