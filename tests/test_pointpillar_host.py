"""CPU: plain PointPillars without a GPU — the float64 restatement of the pillar encoder against the reference's record (G28), the
rounding bound of pointpillar_cases.py on plain float32 arithmetic, the two new modules' parameter names, the shipped config, what
is refused at construction and by the C entry point, and a checkpoint under the reference's key names."""
import os

import numpy as np
import pytest
import torch

import pointpillar_cases as PC
from detparams import det_state
from hvpr_amd import anchor_head, bev_backbone, config, detector, folding, vfe

VS, RNG = [0.16, 0.16, 3.0], [0, -19.84, -2.5, 47.36, 19.84, 0.5]          # make_golden.VOXEL_SIZE / PC_RANGE: G28's vfe cases


@pytest.fixture(scope="module")
def g28():
    return np.load(PC.GOLDEN)


def _vfe_of(z, tag):
    """The product module with the recorded parameters, and its folded layer."""
    shapes = PC.recorded_shapes(z, f"vfe.{tag}")
    m = vfe.PillarVFE(PC.vfe_cfg(NUM_FILTERS=[int(v) for v in z[f"vfe.{tag}.num_filters"]]), 4, VS, RNG)
    PC.load_det(m, shapes, int(z[f"vfe.{tag}.param_seed"])).eval()
    with torch.no_grad():
        f = m._build_folded()
    return m, shapes, f["w"].numpy(), f["b"].numpy()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_float64_restatement_reproduces_the_reference_record(g28, tag, observed):
    """G28's record is the reference's own chain in float32 with BatchNorm applied unfused, so it is held to the bar the kernel is
    held to against the same record (rtol 1e-3, atol 1e-4; the mask exactly); the stored counts say that both a padded slot and a
    live slot decide maxima in it."""
    z = g28
    m, _, w, b = _vfe_of(z, tag)
    p = f"vfe.{tag}."
    r = PC.pfn64(z[p + "voxels"], z[p + "voxel_num_points"], z[p + "voxel_coords"], w, b, m.voxel_size, m.offsets)
    ref = z[p + "pillar_features"]
    observed(f"G28 vfe.{tag}: float64 restatement against the record, max |diff| {np.abs(r['out'] - ref).max():.2e}")
    np.testing.assert_allclose(r["out"], ref, rtol=1e-3, atol=1e-4)
    np.testing.assert_array_equal(r["mask"][..., None].astype(np.float32), z[p + "pillar_mask"])
    assert int(z[p + "pad_wins"]) >= 1 and int(z[p + "live_wins"]) >= 1
    n, P = z[p + "voxel_num_points"], z[p + "voxels"].shape[1]
    assert n.min() == 1 and n.max() == P


@pytest.mark.parametrize("P,c_out", [(1, 32), (20, 64), (32, 128)])
def test_plain_float32_arithmetic_stays_inside_the_bound(P, c_out, observed):
    """The bound is a bound: unfused float32 numpy, one rounding per operation, uses a part of it; dropping the padded slots from
    the maximum (the quirk) or one live slot falls outside it."""
    vox, n, coords = PC.synth_pillars(5 + P, 300, P, VS, RNG, 296, 248)
    w, b = PC.folded_layer(7, c_out)
    off = PC.offsets_of(VS, RNG)
    r = PC.pfn64(vox, n, coords, w, b, VS, off)
    frac = PC.used_fraction(PC.pfn32(vox, n, coords, w, b, VS, off), r)
    observed(f"pillar encoder bound, P = {P}, c_out = {c_out}: float32 numpy uses {frac:.3f} of it")
    assert 0 < frac <= 1.0
    if P > 1:
        live = r["mask"][..., None] > 0
        no_pad = np.where(live, r["y"], -np.inf).max(axis=1)
        assert (np.abs(no_pad - r["out"]) > r["bound"]).any(), "the padded slot decides no maximum in this case"
        first_off = np.where((np.arange(P)[None, :, None] > 0) | ~live, r["y"], -np.inf).max(axis=1)
        assert (np.abs(first_off - r["out"]) > r["bound"]).any()


def test_state_dict_names_and_shapes_equal_the_records(g28):
    z = g28
    for tag in ("A", "B"):
        m, shapes, _, _ = _vfe_of(z, tag)
        own = {k: tuple(v.shape) for k, v in m.state_dict().items() if "num_batches_tracked" not in k}
        assert own == shapes
        assert "pfn_layers.0.linear.weight" in own and "pfn_layers.0.norm.running_var" in own
    for tag in ("small", "full"):
        p = f"bev.{tag}."
        shapes = PC.recorded_shapes(z, f"bev.{tag}")
        filt = [shapes[f"blocks.{i}.1.weight"][0] for i in range(3)]
        m = bev_backbone.BaseBEVBackbone(PC.backbone_cfg(LAYER_NUMS=[int(v) for v in z[p + "layer_nums"]],
                                                         LAYER_STRIDES=[int(v) for v in z[p + "layer_strides"]], NUM_FILTERS=filt,
                                                         NUM_UPSAMPLE_FILTERS=[int(v) for v in z[p + "num_upsample_filters"]]),
                                         input_channels=z[p + "spatial_features"].shape[1])
        own = {k: tuple(v.shape) for k, v in m.state_dict().items() if "num_batches_tracked" not in k}
        assert own == shapes and list(own) == list(shapes)
        assert m.num_bev_features == z[p + "spatial_features_2d"].shape[1]


def test_shipped_config_builds_on_the_cpu():
    cfg = config.pointpillar_cfg()
    ds = detector.SyntheticDataset(cfg)
    assert list(ds.grid_size) == [432, 496, 1]
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    assert isinstance(model, detector.PointPillar) and isinstance(model.vfe, vfe.PillarVFE)
    assert isinstance(model.backbone_2d, bev_backbone.BaseBEVBackbone) and model.backbone_2d.num_bev_features == 384
    assert model.dense_head.num_anchors_per_location == 6
    assert sum(int(np.prod(a.shape[:-1])) for a in model.dense_head.anchors) == 321408 == 216 * 248 * 6
    assert hasattr(model.vfe, "_fold") and hasattr(model.backbone_2d, "_fold")
    assert all(isinstance(m, folding.FoldCached) for m in (model.vfe, model.backbone_2d, model.dense_head))   # what _CapturedState walks
    assert [type(m).__name__ for m in model.module_list] == ["PillarVFE", "PointPillarScatter", "BaseBEVBackbone", "AnchorHeadSingle"]


@pytest.mark.parametrize("kw,n_feat,match", [
    (dict(NUM_FILTERS=[32, 64]), 4, "one PFN layer"),
    (dict(NUM_FILTERS=[]), 4, "one PFN layer"),
    (dict(NUM_FILTERS=[48]), 4, r"\[32\], \[64\] or \[128\]"),
    (dict(USE_NORM=False), 4, "USE_NORM"),
    (dict(WITH_DISTANCE=True), 4, "WITH_DISTANCE"),
    (dict(USE_ABSLOTE_XYZ=False), 4, "USE_ABSLOTE_XYZ"),
    (dict(), 5, "4 raw point features"),
])
def test_vfe_refuses_what_the_kernel_is_not_built_for(kw, n_feat, match):
    with pytest.raises(ValueError, match=match):
        vfe.PillarVFE(PC.vfe_cfg(**kw), n_feat, VS, RNG)


@pytest.mark.parametrize("kw,cin,match", [
    (dict(UPSAMPLE_STRIDES=[1, 2, 0.5]), 64, "integer UPSAMPLE_STRIDES"),
    (dict(UPSAMPLE_STRIDES=[1, 2, 4, 4], NUM_UPSAMPLE_FILTERS=[128] * 4), 64, "extra final deblock"),
    (dict(UPSAMPLE_STRIDES=[], NUM_UPSAMPLE_FILTERS=[]), 64, "UPSAMPLE_STRIDES"),
    (dict(UPSAMPLE_STRIDES=None), 64, "UPSAMPLE_STRIDES"),
    (dict(), 36, "multiples of 8"),
    (dict(NUM_FILTERS=[64, 100, 256]), 64, "multiples of 8"),
    (dict(NUM_UPSAMPLE_FILTERS=[128, 126, 128]), 64, "multiples of 4"),
    (dict(LAYER_STRIDES=[2, 3, 2]), 64, "LAYER_STRIDES of 1 or 2"),
    (dict(CONV_PRECISION="bf16x3"), 64, "fp32 convolutions only"),
])
def test_backbone_refuses_what_the_ops_do_not_take(kw, cin, match):
    with pytest.raises(ValueError, match=match):
        bev_backbone.BaseBEVBackbone(PC.backbone_cfg(**kw), input_channels=cin)


def test_modules_build_with_supported_settings_and_refuse_training_forwards():
    for width in (32, 64, 128):
        m = vfe.PillarVFE(PC.vfe_cfg(NUM_FILTERS=[width]), 4, VS, RNG)
        assert m.get_output_feature_dim() == width and tuple(m.pfn_layers[0].linear.weight.shape) == (width, 10)
    m.train()
    with pytest.raises(NotImplementedError, match="no training forward"):
        m({"voxels": torch.zeros(1, 32, 4), "voxel_num_points": torch.ones(1), "voxel_coords": torch.zeros(1, 4)})
    bb = bev_backbone.BaseBEVBackbone(PC.backbone_cfg(), input_channels=64).train()
    with pytest.raises(NotImplementedError, match="no training forward"):
        bb({"spatial_features": torch.zeros(1, 64, 8, 8)})


def test_fold_caches_are_dropped_by_train_and_load_state_dict():
    hvpr = config.hvpr_car_cfg().MODEL
    head = anchor_head.AnchorHeadSingle(model_cfg=hvpr.DENSE_HEAD, input_channels=64, num_class=1, class_names=["Car"],
                                        grid_size=np.array([16, 16, 1]), point_cloud_range=np.array([0, -1.28, -3, 2.56, 1.28, 1], np.float32))
    for m in (vfe.PillarVFE(PC.vfe_cfg(), 4, VS, RNG), bev_backbone.BaseBEVBackbone(PC.backbone_cfg(), input_channels=64),
              vfe.PillarVFE_Scale(hvpr.VFE, 4, VS, RNG), bev_backbone.BaseBEVBackbone_Scale(hvpr.BACKBONE_2D, input_channels=64), head):
        assert isinstance(m, folding.FoldCached) and type(m._fold) is folding.FoldCache and m._fold.value is None
        m.eval()
        m._fold.value, m._fold.device = "stale", torch.device("cpu")
        m.load_state_dict(m.state_dict())
        assert m._fold.value is None
        m._fold.value = "stale"
        m.train(False)
        assert m._fold.value is None


def test_fold_cached_alone_drops_its_fold_and_registers_nothing():
    class Toy(folding.FoldCached):
        pass

    m = Toy()
    assert type(m._fold) is folding.FoldCache and m._fold.value is None and m._fold.device is None
    for drop in (lambda: m.train(False), lambda: m.train(True), lambda: m.load_state_dict(m.state_dict())):
        m._fold.value = "stale"
        drop()
        assert m._fold.value is None
    assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers()) and not list(m.children())
    assert m.train(False) is m and m.training is False and m.train() is m and m.training is True


# Every shipped model's names in registration order, taken at the commit before the modules got their common bases: optimizer
# checkpoints and the fused flat optimizer steps index parameters by position.  Per kind the count and sha256("\n".join(names))[:16];
# RUNS: the submodules in that order with their (named_parameters, state_dict) counts, which say where an order first departs.
_HVPR_RUNS = [("global_step", 0, 1), ("backbone_3d.SA_modules", 36, 72), ("backbone_3d.FP_modules", 12, 24), ("vfe.pfn_layers", 6, 12),
              ("vfe.pfn_scale_layers", 6, 12), ("map_to_bev_module.memory", 1, 1), ("backbone_2d.sfmblocks_down", 9, 18),
              ("backbone_2d.scale_layers", 9, 18), ("backbone_2d.blocks", 36, 72), ("backbone_2d.deblocks", 9, 18),
              ("backbone_2d.attention", 4, 7), ("dense_head.conv_cls", 2, 2), ("dense_head.conv_box", 2, 2), ("dense_head.conv_dir_cls", 2, 2)]
_HVPR_NAMES = {"named_parameters": (134, "2affb0e0d6df95bf"), "state_dict": (261, "759ab6ee4bab47ed"), "runs": _HVPR_RUNS}
NAME_ORDER = {"hvpr_car_cfg": _HVPR_NAMES, "hvpr_3class_cfg": _HVPR_NAMES, "hvpr_car_atss_cfg": _HVPR_NAMES,
              "pointpillar_cfg": {"named_parameters": (66, "c1d37bc01841e3aa"), "state_dict": (127, "073b7e2706caa69b"),
                                  "runs": [("global_step", 0, 1), ("vfe.pfn_layers", 3, 6), ("backbone_2d.blocks", 48, 96),
                                           ("backbone_2d.deblocks", 9, 18), ("dense_head.conv_cls", 2, 2), ("dense_head.conv_box", 2, 2),
                                           ("dense_head.conv_dir_cls", 2, 2)]}}


def _first_departure(names, runs):
    """'' when `names` follow `runs` = [(prefix, count), ...]; else the first position that does not, with both neighbours."""
    want = [p for p, n in runs for _ in range(n)]
    for i in range(max(len(names), len(want))):
        if i >= len(names) or i >= len(want) or not (names[i] + ".").startswith(want[i] + "."):
            return f"position {i}: {names[max(i - 1, 0):i + 2]} where {want[max(i - 1, 0):i + 2]} stood"
    return ""


@pytest.mark.parametrize("which", sorted(NAME_ORDER))
def test_parameter_and_state_dict_names_keep_their_order(which):
    import hashlib
    cfg = getattr(config, which)()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
    for col, kind, names in ((1, "named_parameters", [n for n, _ in model.named_parameters()]), (2, "state_dict", list(model.state_dict()))):
        count, digest = NAME_ORDER[which][kind]
        assert sum(r[col] for r in NAME_ORDER[which]["runs"]) == count
        where = _first_departure(names, [(r[0], r[col]) for r in NAME_ORDER[which]["runs"]])
        print(f"{which} {kind}(): {where or 'every submodule in its place'}")
        assert not where, f"{which}: {kind}() order changed at {where}"
        assert (len(names), hashlib.sha256("\n".join(names).encode()).hexdigest()[:16]) == (count, digest)


def test_c_entry_refuses_unsupported_shapes_without_a_device():
    from hvpr_amd._lib import lib
    L = lib()

    def status(M, P, c_out, ptr=None):
        return L.hvpr_pillar_vfe_plain_fwd_f32(ptr, ptr, ptr, M, P, None, 0.16, 0.16, 4.0, 0.08, -39.6, -1.0, ptr, ptr, c_out, ptr, None, None)

    assert status(1, 32, 48) == -2 and status(1, 33, 64) == -2 and status(1, 33, 48) == -2          # HVPR_ERR_UNSUPPORTED
    assert status(1, 0, 64) == -1 and status(-1, 32, 64) == -1 and status(1, 32, 0) == -1            # HVPR_ERR_INVALID_ARG
    assert status(1, 32, 64) == -1                                                                  # NULL tensors
    assert status(0, 32, 64) == 0 and status(0, 1, 128) == 0 and status(0, 32, 32) == 0             # nothing to do: no launch


def test_plain_entry_is_declared_in_the_one_header_and_bound_from_it():
    """hvpr_pillar_vfe_plain_fwd_f32 stands in include/hvpr_amd.h, the only header, and is bound through the one pair of tables with
    the derived types."""
    import ctypes as c
    from hvpr_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert not any(hasattr(_lib, name) for name in ("ADDED_SIGNATURES", "ADDED_PARAMS", "params_of"))
    # one header per library: libhvpr_amd.so's, and hvpr_cpu.h of the host-side libhvpr_cpu.so (gt_sampling.py), which declares no GPU entry
    headers = sorted(f for f in os.listdir(os.path.join(root, "include")) if f.endswith(".h"))
    assert headers == ["hvpr_amd.h", "hvpr_cpu.h"] and [h for h in headers if h != "hvpr_cpu.h"] == ["hvpr_amd.h"]
    assert '#include "hvpr_' not in open(os.path.join(root, "include", "hvpr_amd.h")).read()
    P, I, F = c.c_void_p, c.c_int, c.c_float
    res, args = _lib.SIGNATURES["hvpr_pillar_vfe_plain_fwd_f32"]
    assert res is I and args == [P, P, P, I, I, P, F, F, F, F, F, F, P, P, I, P, P, P]
    kinds = dict(_lib.PARAMS["hvpr_pillar_vfe_plain_fwd_f32"])
    assert len(kinds) == 18 and kinds["voxels"] == torch.float32 and kinds["num_points"] == kinds["coords"] == kinds["m_device"] == torch.int32
    assert kinds["pillar_mask"] == torch.float32 and kinds["c_out"] is None and kinds["stream"] is None
    fn = _lib.lib().hvpr_pillar_vfe_plain_fwd_f32
    assert fn.restype is I and list(fn.argtypes) == args
    with pytest.raises(TypeError, match="c_out is a scalar"):
        _lib.call("hvpr_pillar_vfe_plain_fwd_f32", *([None] * 14), torch.tensor(64), None, None, None)


def test_wrapper_has_no_cpu_path():
    from hvpr_amd import kernels
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.pillar_vfe_plain_fwd(torch.zeros(2, 32, 4), torch.ones(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                                     torch.zeros(64, 10), torch.zeros(64), VS, [0.08, -19.76, -1.0])


def test_pointpillar_in_training_mode_still_raises():
    model = PC.build_model(PC.tiny_cfg())
    model.train()
    with pytest.raises(NotImplementedError, match="no training path"):
        model({"voxels": torch.zeros(1, 32, 4), "batch_size": 1})


def test_checkpoint_under_the_reference_key_names_loads(g28, tmp_path):
    z = g28
    shapes = PC.recorded_shapes(z, "chain")
    assert {k.split(".")[0] for k in shapes} == {"vfe", "backbone_2d", "dense_head"}
    state = {k: torch.from_numpy(v) for k, v in det_state(shapes, int(z["chain.param_seed"])).items()}
    path = os.path.join(tmp_path, "checkpoint_epoch_80.pth")
    torch.save({"model_state": state, "epoch": 80}, path)
    model = PC.build_model(PC.grid_cfg(z["chain.point_cloud_range"], z["chain.voxel_size"]), seed=1)
    model.vfe._fold.value = "stale"
    updated, total = model.load_params_from_file(path, to_cpu=True)
    own = model.state_dict()
    assert updated == len(shapes) and total == len(own)
    assert sorted(k for k in own if k not in shapes) == sorted(k for k in own if k == "global_step" or k.endswith("num_batches_tracked"))
    for k, v in state.items():
        assert torch.equal(own[k].cpu(), v), k
    assert model.vfe._fold.value is None
