"""Fixture G24 (build container only, like its siblings): the reference's BEV picture, tools/vis.py, run as plain Python.

Nothing of the reference is restated here: the file is read, cut in front of its demo half (`import argparse`), its imports of
matplotlib and the pcdet packages dropped, and executed in memory with two stubs --
  numba   jit -> identity, as g13_voxel_index does it;
  cv2     cvtColor repeats the channel (GRAY2RGB), line RECORDS its endpoints, colour and thickness (cv2 is not installed
          where the fixtures are made, so how it rasterises a line is not pinned; what the reference hands to it is).
Then kitti_vis' two calls (:282-284) are made on a small view: point_to_vis_bev for the height picture and the count plane
(bev_map[-1], taken from points_to_bev by a spy), draw_box_in_bev for the segments.

The view's numbers are float32 values given as Python floats, so that the float64 arithmetic of draw_box_in_bev (which reads the
range as a float64 array) and the float32 arithmetic of points_to_bev see the same range.

The device's float32 sin / cos may differ from numpy's in the last bit and astype(np.int32) turns that into a pixel, so every
scaled corner coordinate, computed in float64, must lie at least 1e-2 px from an integer: a box that does not is redrawn
(bev_vis_cases.settle_boxes).  On this fixture equality of the segments is then a requirement, not a tolerance.

Writes tests/golden/g24_bev_vis.npz."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bev_vis_cases as C  # noqa: E402

REF = "/root/reference"


def load_vis(lines_drawn):
    def jit(*a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else (lambda f: f)
    nb = types.ModuleType("numba")
    nb.jit, nb.prange = jit, range
    cv2 = types.ModuleType("cv2")
    cv2.LINE_8, cv2.COLOR_GRAY2RGB = 8, 8

    def cvt(img, code):
        assert code == cv2.COLOR_GRAY2RGB and img.ndim == 2
        return np.repeat(img[:, :, None], 3, axis=2)

    def line(img, a, b, color, thickness):
        lines_drawn.append([int(a[0]), int(a[1]), int(b[0]), int(b[1])] + [int(c) for c in color] + [int(thickness)])
        return img
    cv2.cvtColor, cv2.line = cvt, line
    sys.modules["numba"], sys.modules["cv2"] = nb, cv2
    path = os.path.join(REF, "tools/vis.py")
    src = open(path).read().split("\n")
    stop = next(i for i, l in enumerate(src) if l.startswith("import argparse"))
    keep = [l for l in src[:stop] if not (l.startswith("import matplotlib") or l.startswith("from pcdet"))]
    mod = types.ModuleType("hvpr_ref_tools_vis")
    mod.__file__ = path
    exec(compile("\n".join(keep), path, "exec"), mod.__dict__)
    return mod


def main():
    drawn = []
    vis = load_vis(drawn)
    captured = {}
    inner = vis.points_to_bev

    def spy(*a, **k):
        captured["bev"] = inner(*a, **k)
        return captured["bev"]
    vis.points_to_bev = spy

    pixel = float(np.float32(0.1))
    view = [float(np.float32(v)) for v in (0.0, -2.4, -1.0, 6.4, 2.4, 1.0)]       # 64 x 48 pixels
    H, W = C.grid_of(view, pixel)
    assert (H, W) == (48, 64)
    gen = np.random.default_rng(2424)
    out = {"range": np.array(view, np.float32), "pixel": np.float32(pixel)}

    pts = C.frame_points(gen, 700, view)
    lo, hi = np.array(view[:3], np.float32), np.array(view[3:], np.float32)
    inside = np.array([3.21, 0.37, 0.2], np.float32)
    k = 0
    for j in range(3):                                                           # on lo (kept) and on hi (dropped), every axis
        for edge in (lo[j], hi[j], np.nextafter(hi[j], np.float32(-np.inf), dtype=np.float32)):
            pts[k, :3] = inside
            pts[k, j] = edge
            k += 1
    pts[k, :3] = (1.0, 1.0, lo[2]); k += 1                                        # z == z_lo alone in its cell: counted, height 0
    pts[k:k + 60, 0] = gen.uniform(4.0, 4.1, 60)                                  # a cell with many points
    pts[k:k + 60, 1] = gen.uniform(-1.0, -0.9, 60)
    pts[k:k + 60, 2] = gen.uniform(-1.2, 1.2, 60)
    keep = ~((np.floor((pts[:, 0] - lo[0]) / np.float32(pixel)) == 10) & (np.floor((pts[:, 1] - lo[1]) / np.float32(pixel)) == 34))
    keep[k - 1] = True
    pts = pts[keep]                                                              # nothing else in the z_lo point's cell
    gen.shuffle(pts, axis=0)
    for tag, p in (("full", pts), ("empty", np.zeros((0, 4), np.float32))):
        img = vis.point_to_vis_bev(p, [pixel, pixel, pixel], list(view))
        counts = captured["bev"][-1]
        assert img.shape == (H, W, 3) and img.dtype == np.uint8 and (counts > 0).sum() < 80000
        out[tag + "_points"] = p
        out[tag + "_image"] = img
        out[tag + "_counts"] = counts.astype(np.int32)
        print("g24", tag, len(p), "points,", int((counts > 0).sum()), "cells, max count", int(counts.max()))
    assert out["full_counts"][34, 10] == 1 and out["full_image"][34, 10, 0] == 0
    assert out["full_counts"].max() >= 40

    boxes = np.array([
        [2.03, 0.21, 0.0, 1.63, 0.71, 1.5, 0.0],                   # headings 0, +-pi/2
        [4.51, -1.13, 0.0, 1.41, 0.63, 1.5, np.pi / 2],
        [1.27, -1.41, 0.0, 1.23, 0.57, 1.5, -np.pi / 2],
        [3.33, 1.27, 0.0, 1.71, 0.83, 1.5, 0.6137],                # general angles
        [5.17, 0.53, 0.0, 1.37, 0.67, 1.5, -2.3171],
        [0.23, 2.07, 0.0, 1.93, 0.91, 1.5, 1.1],                   # across the image border
        [6.21, -2.13, 0.0, 1.57, 0.77, 1.5, 2.9],
        [9.7, 5.3, 0.0, 1.5, 0.7, 1.5, 0.4],                       # wholly outside
        [2.57, -0.63, 0.0, 0.0, 0.0, 0.0, 0.3],                    # zero size
    ], np.float32)
    boxes = C.settle_boxes(boxes, view, pixel, gen)
    for s in (1, -1):
        assert (C.corner_margin(boxes, view, pixel, s) >= C.MARGIN).all()
    img = np.zeros((H, W, 3), np.uint8)
    vis.draw_box_in_bev(img, list(view), boxes, [0, 255, 0], 2)
    rec = np.array(drawn, np.int32)
    assert rec.shape == (3 * len(boxes), 8)
    out["boxes"] = boxes
    out["segments"] = rec[:, :4]
    out["segment_colour"] = rec[:, 4:7]
    out["segment_thickness"] = rec[:, 7]
    np.savez_compressed(os.path.join(HERE, "g24_bev_vis.npz"), **out)
    print("g24", len(boxes), "boxes,", len(rec), "segments")


if __name__ == "__main__":
    main()
