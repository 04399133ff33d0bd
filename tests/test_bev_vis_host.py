"""CPU: the numpy restatement of the BEV picture (tests/bev_vis_cases.py) against fixture G24, the reference's own tools/vis.py run
as plain Python (tests/golden/make_golden_bev_vis.py); the PNG encoder of hvpr_amd/bev_vis.py; the argument handling, the file
list and the config override of python -m hvpr_amd.demo."""
import os
import struct
import zlib

import numpy as np
import pytest

import bev_vis_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAR = os.path.join(ROOT, "hvpr_amd", "cfgs", "kitti_models", "hvpr_car.yaml")


@pytest.fixture(scope="module")
def g24(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g24_bev_vis.npz")))


# ------------------------------------------------------------------------------------------------ restatement == G24
@pytest.mark.parametrize("tag", ["full", "empty"])
def test_height_pass_equals_reference(g24, tag):
    height, counts = C.height_pass(g24[tag + "_points"][:, :3], g24["range"], float(g24["pixel"]))
    assert counts.dtype == np.int32 and (counts == g24[tag + "_counts"]).all()
    image = np.repeat(C.grey_of(height)[:, :, None], 3, axis=2)
    assert image.shape == g24[tag + "_image"].shape and (image == g24[tag + "_image"]).all()


def test_fixture_holds_its_cases(g24):
    pts, rng, counts = g24["full_points"], g24["range"], g24["full_counts"]
    for j in range(3):
        assert (pts[:, j] == rng[j]).any() and (pts[:, j] == rng[j + 3]).any()          # on lo and on hi, every axis
    assert int(counts.sum()) < len(pts) and counts.max() >= 40                            # points dropped; a crowded cell
    lone = np.nonzero((pts[:, 2] == rng[2]) & (pts[:, 0] == 1.0))[0]
    assert len(lone) == 1 and counts[34, 10] == 1 and g24["full_image"][34, 10, 0] == 0   # z == z_lo: counted, height 0
    assert len(g24["empty_points"]) == 0 and g24["empty_counts"].sum() == 0
    assert (counts > 0).sum() < 80000                                                     # under the reference's cell cap


def test_segments_equal_reference(g24):
    seg, drawn = C.box_segments(g24["boxes"], g24["range"], float(g24["pixel"]), sign=1)
    assert drawn.all() and seg.dtype == np.int32
    assert (seg.reshape(-1, 4) == g24["segments"]).all()
    assert (g24["segment_thickness"] == 2).all() and (g24["segment_colour"] == [0, 255, 0]).all()
    for s in (1, -1):
        assert (C.corner_margin(g24["boxes"], g24["range"], float(g24["pixel"]), s) >= C.MARGIN).all()
    H, W = C.grid_of(g24["range"], float(g24["pixel"]))
    s = g24["segments"].reshape(-1, 3, 4)
    out = ((s[:, :, [0, 2]] < 0) | (s[:, :, [0, 2]] >= W) | (s[:, :, [1, 3]] < 0) | (s[:, :, [1, 3]] >= H))
    assert out.reshape(len(s), -1).all(axis=1).any()                                      # a box wholly outside
    assert (out.reshape(len(s), -1).any(axis=1) & ~out.reshape(len(s), -1).all(axis=1)).any()   # one across the border
    assert ((s[:, :, 0] == s[:, :, 2]) & (s[:, :, 1] == s[:, :, 3])).all(axis=1).any()   # the zero-size box


def test_negated_heading_and_sign_minus_one_is_the_same_drawing(g24):
    boxes = g24["boxes"].copy()
    a, _ = C.box_segments(boxes, g24["range"], float(g24["pixel"]), sign=1)
    boxes[:, 6] = -boxes[:, 6]
    b, _ = C.box_segments(boxes, g24["range"], float(g24["pixel"]), sign=-1)
    assert (a == b).all()


# ------------------------------------------------------------------------------------------------ the integer line rule
def _bresenham(ax, ay, bx, by):
    dx, dy, sx, sy = abs(bx - ax), -abs(by - ay), 1 if ax < bx else -1, 1 if ay < by else -1
    err, out = dx + dy, []
    while True:
        out.append((ax, ay))
        if ax == bx and ay == by:
            return out
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            ax += sx
        if e2 <= dx:
            err += dx
            ay += sy


def test_thickness_one_contains_every_bresenham_pixel():
    gen = np.random.default_rng(5)
    for _ in range(40):
        ax, ay, bx, by = (int(v) for v in gen.integers(0, 40, 4))
        plane = np.zeros((40, 40), np.uint32)
        C.draw_segment(plane, (ax, ay, bx, by), 3, 1)
        for x, y in _bresenham(ax, ay, bx, by):
            assert plane[y, x] == 3, (ax, ay, bx, by, x, y)


def test_line_rule_against_float_distance():
    """4 d^2 <= t^2 with d from a float64 point-segment distance, on pixels that are not within 1e-9 of the boundary."""
    gen = np.random.default_rng(6)
    for t in (1, 2, 5):
        for _ in range(20):
            ax, ay, bx, by = (int(v) for v in gen.integers(-10, 50, 4))
            plane = np.zeros((37, 53), np.uint32)
            C.draw_segment(plane, (ax, ay, bx, by), 1, t)
            py, px = np.mgrid[0:37, 0:53].astype(np.float64)
            ab = np.array([bx - ax, by - ay], np.float64)
            L = float(ab @ ab)
            u = np.clip(((px - ax) * ab[0] + (py - ay) * ab[1]) / L, 0, 1) if L > 0 else np.zeros_like(px)
            d = np.hypot(px - (ax + u * ab[0]), py - (ay + u * ab[1]))
            sure = np.abs(d - t / 2) > 1e-9
            assert ((plane == 1) == (d <= t / 2))[sure].all()


def test_larger_ink_wins_whatever_the_order():
    a, b = (2, 2, 30, 20), (30, 2, 2, 20)
    p, q = np.zeros((24, 34), np.uint32), np.zeros((24, 34), np.uint32)
    C.draw_segment(p, a, 1, 2); C.draw_segment(p, b, 4, 2)
    C.draw_segment(q, b, 4, 2); C.draw_segment(q, a, 1, 2)
    assert (p == q).all() and set(np.unique(p)) == {0, 1, 4}


# ------------------------------------------------------------------------------------------------ PNG
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (48, 64)])
def test_png_round_trip(shape, tmp_path):
    from hvpr_amd import bev_vis
    a = np.random.default_rng(7).integers(0, 256, shape + (3,)).astype(np.uint8)
    data = bev_vis.encode_png(a)
    assert (C.decode_png(data) == a).all()
    bev_vis.write_png(tmp_path / "a.png", a)
    assert (tmp_path / "a.png").read_bytes() == data
    # the layout by hand: signature, IHDR of 13 bytes, 8-bit RGB
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[8:16] == struct.pack(">I4s", 13, b"IHDR")
    assert struct.unpack(">IIBBBBB", data[16:29]) == (shape[1], shape[0], 8, 2, 0, 0, 0)
    assert struct.unpack(">I", data[29:33])[0] == zlib.crc32(data[12:29]) & 0xffffffff
    bad = bytearray(data)
    bad[40] ^= 1
    with pytest.raises((AssertionError, zlib.error)):
        C.decode_png(bytes(bad))


def test_png_refuses_other_arrays():
    from hvpr_amd import bev_vis
    for a in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            bev_vis.encode_png(a)


def test_class_palette():
    from hvpr_amd import bev_vis
    p = bev_vis.class_palette(3)
    assert p.shape == (5, 3) and p.dtype == np.uint8 and tuple(p[-1]) == bev_vis.GT_COLOUR and tuple(p[1]) == (0, 255, 0)
    assert len({tuple(r) for r in p[1:]}) == 4


# ------------------------------------------------------------------------------------------------ the command's host side
def test_demo_arguments():
    from hvpr_amd import demo
    args, cfg = demo.parse_config(["--cfg_file", CAR, "--data_path", "d", "--ckpt", "c.pth"])
    assert (args.ext, args.batch_size, args.pixel, args.no_png, args.pipeline, args.score_thresh, args.output_dir) == \
        (".bin", 1, 0.1, False, False, None, None)
    assert cfg.CLASS_NAMES == ["Car"] and cfg.TAG == "hvpr_car"
    args, cfg = demo.parse_config(["--cfg_file", CAR, "--data_path", "d", "--ckpt", "c.pth", "--ext", ".npy", "--output_dir", "o",
                                   "--batch_size", "3", "--score_thresh", "0.3", "--pixel", "0.2", "--no_png", "--set",
                                   "MODEL.POST_PROCESSING.SCORE_THRESH", "0.2"])
    assert (args.ext, args.batch_size, args.pixel, args.no_png, args.score_thresh, args.output_dir) == (".npy", 3, 0.2, True, 0.3, "o")
    assert cfg.MODEL.POST_PROCESSING.SCORE_THRESH == 0.2
    with pytest.raises(ValueError, match="batch_size 1"):
        demo.parse_config(["--cfg_file", CAR, "--pipeline", "--batch_size", "2"])
    with pytest.raises(ValueError):
        demo.parse_config(["--cfg_file", CAR, "--pixel", "0"])
    with pytest.raises(SystemExit):
        demo.parse_config(["--data_path", "d"])                     # --cfg_file is required
    assert demo.batch_indices(5, 2) == [[0, 1], [2, 3], [4]] and demo.batch_indices(2, 1) == [[0], [1]]


def test_file_list_is_demo_datasets(tmp_path):
    import glob
    from hvpr_amd import demo
    for name in ("10.bin", "2.bin", "000001.bin", "b.bin", "B.bin", "a.npy", "2.npy", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    for ext in (".bin", ".npy"):
        want = glob.glob(str(tmp_path / f"*{ext}"))
        want.sort()                                                  # tools/demo.py:36-38
        assert demo.list_files(tmp_path, ext) == want and len(want) == (5 if ext == ".bin" else 2)
    assert [os.path.basename(f) for f in demo.list_files(tmp_path, ".bin")] == ["000001.bin", "10.bin", "2.bin", "B.bin", "b.bin"]
    assert demo.list_files(tmp_path / "2.bin", ".bin") == [str(tmp_path / "2.bin")]      # a file stands for itself
    assert demo.list_files(tmp_path, ".pcd") == []


def test_reading_and_unknown_extension(tmp_path):
    from hvpr_amd import demo
    pts = np.random.default_rng(8).normal(size=(11, 4)).astype(np.float32)
    pts.tofile(tmp_path / "a.bin")
    np.save(tmp_path / "a.npy", pts)
    assert (demo.read_points(tmp_path / "a.bin", ".bin") == pts).all()
    assert (demo.read_points(tmp_path / "a.npy", ".npy") == pts).all()
    with pytest.raises(NotImplementedError):
        demo.read_points(tmp_path / "a.bin", ".pcd")
    with pytest.raises(NotImplementedError):
        demo.DemoFrames([str(tmp_path / "a.bin")], ".txt", device="cpu")
    f = demo.DemoFrames([str(tmp_path / "a.bin")], ".bin", device="cpu")(0)
    assert f["frame_id"] == "a" and (f["points"].numpy() == pts).all()


def test_fov_filter_is_forced_off_and_logged():
    from hvpr_amd import demo

    class Log:
        lines = []

        def info(self, s):
            self.lines.append(s)
    _, cfg = demo.parse_config(["--cfg_file", CAR])
    assert cfg.DATA_CONFIG["FOV_POINTS_ONLY"] is True
    dc = demo.demo_data_config(cfg, Log())
    assert dc["FOV_POINTS_ONLY"] is False and cfg.DATA_CONFIG["FOV_POINTS_ONLY"] is True       # the config itself is left alone
    assert len(Log.lines) == 1 and "FOV_POINTS_ONLY" in Log.lines[0] and "forced off" in Log.lines[0]
    cfg.DATA_CONFIG["FOV_POINTS_ONLY"] = False
    Log.lines.clear()
    assert demo.demo_data_config(cfg, Log())["FOV_POINTS_ONLY"] is False and Log.lines == []


def test_record_entry():
    from hvpr_amd import demo
    rec = {"pred_boxes": np.arange(28, dtype=np.float32).reshape(4, 7), "pred_scores": np.array([.9, .8, .7, .6], np.float32),
           "pred_labels": np.array([1, 2, 1, 1]), "pred_count": np.array([2], np.int32)}
    e = demo.record_entry(rec, "f", ["Car", "Cyclist"])
    assert sorted(e) == ["boxes_lidar", "frame_id", "name", "pred_labels", "score"]
    assert e["name"].tolist() == ["Car", "Cyclist"] and e["score"].tolist() == rec["pred_scores"][:2].tolist()
    assert e["boxes_lidar"].shape == (2, 7) and e["pred_labels"].tolist() == [1, 2]
    rec["pred_count"] = np.array([0], np.int32)
    assert len(demo.record_entry(rec, "f", ["Car"])["name"]) == 0
