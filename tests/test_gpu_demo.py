"""GPU: python -m hvpr_amd.demo over five synthetic point-cloud files, a checkpoint saved from synthetic_weights and the car config.
The pictures must decode to `bev_vis.render_bev` of the same records, result.pkl must equal the eager `sync=True` detections of the
same batches, and the pipelined run and the `.npy` run must leave the same bytes as the eager `.bin` run."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import bev_vis_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAR = os.path.join(ROOT, "hvpr_amd", "cfgs", "kitti_models", "hvpr_car.yaml")
DEV = "cuda:0"
STEMS = ["000002", "000010", "a_frame", "b_frame", "c_half"]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Five frames as .bin and as .npy, a checkpoint, and the eager .bin run of the command (in this process)."""
    import torch
    from hvpr_amd import demo, detector, synthetic, synthetic_weights
    from hvpr_amd.config import hvpr_car_cfg
    root = tmp_path_factory.mktemp("demo")
    (root / "bin").mkdir()
    (root / "npy").mkdir()
    for k, stem in enumerate(STEMS):
        pts = synthetic.kitti_like_frame(40 + k)
        if stem == "c_half":
            pts = np.ascontiguousarray(pts[::2])           # fewer points in range than NUM_POINTS: the padded branch of sample_points
        pts.tofile(root / "bin" / f"{stem}.bin")
        np.save(root / "npy" / f"{stem}.npy", pts)
    (root / "bin" / "notes.txt").write_text("not a point cloud")
    cfg = hvpr_car_cfg()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
    synthetic_weights.load_synthetic(model, seed=0, cls_bias=-2.0)
    torch.save({"model_state": model.state_dict()}, root / "ckpt.pth")
    entries = demo.main(["--cfg_file", CAR, "--data_path", str(root / "bin"), "--ckpt", str(root / "ckpt.pth"), "--output_dir",
                         str(root / "eager")])
    return {"root": root, "cfg": cfg, "model": model.to(DEV).eval(), "entries": entries}


def _same_entries(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) == ["boxes_lidar", "frame_id", "name", "pred_labels", "score"]
        assert x["frame_id"] == y["frame_id"] and x["name"].tolist() == y["name"].tolist()
        for k in ("boxes_lidar", "score", "pred_labels"):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (x["frame_id"], k)


def test_pictures_and_records_of_the_eager_run(scene):
    import torch
    from hvpr_amd import bev_vis, demo
    root, cfg, model = scene["root"], scene["cfg"], scene["model"]
    out = root / "eager"
    assert sorted(p.name for p in out.iterdir()) == sorted([s + ".png" for s in STEMS] + ["result.pkl"])
    with open(out / "result.pkl", "rb") as f:
        entries = pickle.load(f)
    _same_entries(entries, scene["entries"])
    assert [e["frame_id"] for e in entries] == STEMS and sum(len(e["score"]) for e in entries) > 0
    files = demo.list_files(root / "bin", ".bin")
    loader = demo.build_loader(cfg, files, ".bin", DEV)
    H, W = C.grid_of(cfg.DATA_CONFIG["POINT_CLOUD_RANGE"], 0.1)
    for i, stem in enumerate(STEMS):
        with torch.no_grad():
            batch = demo.prepare(loader, [i], 0)
            assert batch["points"].shape == (16384, 5)
            records, _, _ = model(batch, sync=False)
            image = bev_vis.render_bev(batch, records, cfg=cfg).cpu().numpy()
            synced, _, _ = model(demo.prepare(loader, [i], 0), sync=True)
        got = C.decode_png((out / f"{stem}.png").read_bytes())
        assert got.shape == (H, W, 3) and (got == image[0]).all()
        n = len(synced[0]["pred_scores"])
        e = entries[i]
        assert e["boxes_lidar"].tobytes() == synced[0]["pred_boxes"].cpu().numpy().tobytes() and len(e["score"]) == n
        assert e["score"].tobytes() == synced[0]["pred_scores"].cpu().numpy().tobytes()
        assert e["pred_labels"].tolist() == synced[0]["pred_labels"].cpu().numpy().tolist()
        assert e["name"].tolist() == ["Car"] * n
        # the picture shows the frame: points in grey, and the class ink wherever a box was kept
        ink = (got == bev_vis.class_palette(1)[1]).all(axis=-1)
        assert ink.any() == (n > 0) and got[~ink].max() > 0


def test_pipelined_run_leaves_the_same_bytes(scene):
    from hvpr_amd import demo
    root = scene["root"]
    entries = demo.main(["--cfg_file", CAR, "--data_path", str(root / "bin"), "--ckpt", str(root / "ckpt.pth"), "--output_dir",
                         str(root / "pipe"), "--pipeline"])
    _same_entries(entries, scene["entries"])
    with open(root / "pipe" / "result.pkl", "rb") as f:
        _same_entries(pickle.load(f), scene["entries"])
    for stem in STEMS:
        assert (root / "pipe" / f"{stem}.png").read_bytes() == (root / "eager" / f"{stem}.png").read_bytes(), stem


def test_npy_run_of_the_command_line_equals_the_bin_run(scene):
    root = scene["root"]
    r = subprocess.run([sys.executable, "-m", "hvpr_amd.demo", "--cfg_file", CAR, "--data_path", str(root / "npy"), "--ext", ".npy",
                        "--ckpt", str(root / "ckpt.pth"), "--output_dir", str(root / "npy_out")], cwd=ROOT, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "FOV_POINTS_ONLY" in r.stdout and "forced off" in r.stdout and "Demo done: 5 frames" in r.stdout
    with open(root / "npy_out" / "result.pkl", "rb") as f:
        _same_entries(pickle.load(f), scene["entries"])
    for stem in STEMS:
        assert (root / "npy_out" / f"{stem}.png").read_bytes() == (root / "eager" / f"{stem}.png").read_bytes(), stem


def test_one_file_no_png_and_a_refused_frame(scene, tmp_path):
    from hvpr_amd import demo
    root = scene["root"]
    entries = demo.main(["--cfg_file", CAR, "--data_path", str(root / "bin" / "a_frame.bin"), "--ckpt", str(root / "ckpt.pth"),
                         "--output_dir", str(tmp_path / "one"), "--no_png", "--batch_size", "2"])
    assert sorted(p.name for p in (tmp_path / "one").iterdir()) == ["result.pkl"] and len(entries) == 1
    assert entries[0]["frame_id"] == "a_frame"
    # batch 1 seeds by the frame's index in the list: a_frame is frame 2 of the folder and frame 0 here, so only the sizes agree
    assert entries[0]["boxes_lidar"].shape[1] == 7
    small = tmp_path / "small.bin"
    np.zeros((100, 4), np.float32).tofile(small)                    # 100 points: sample_points cannot pad to 16384
    loader = demo.build_loader(scene["cfg"], [str(small)], ".bin", DEV)
    with pytest.raises(ValueError, match="small.bin"):
        demo.prepare(loader, [0], 0)
