"""Times the BEV picture op (csrc/bev_render.hip) against the numpy restatement of tests/bev_vis_cases.py on the same inputs: one
frame of 123 k points and 50 boxes on the car config's range at 0.1 m pixels (397 x 474).

Three runs of each side, alternating (op, numpy, op, numpy, ...): an op run is the median of `--iters` calls timed one by one with
device events after `--warmup` calls; a numpy run is one call timed with perf_counter.  The two outputs are compared byte for byte
first (the boxes keep the margin rule of bev_vis_cases.settle_boxes).  Prints one JSON line.

    python tools/bench_bev_render.py [--points 123000] [--boxes 50] [--iters 50] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import bev_vis_cases as C
    from hvpr_amd import bev_vis, kernels
    from hvpr_amd.config import hvpr_car_cfg
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=123000)
    ap.add_argument("--boxes", type=int, default=50)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pixel", type=float, default=0.1)
    args = ap.parse_args()
    rng = [float(v) for v in hvpr_car_cfg().DATA_CONFIG["POINT_CLOUD_RANGE"]]
    gen = np.random.default_rng(19)
    pts = np.concatenate([np.zeros((args.points, 1), np.float32), C.frame_points(gen, args.points, rng)], axis=1)
    off = np.array([0, args.points], np.int32)
    boxes = C.random_boxes(gen, args.boxes, rng, args.pixel)
    boxes[:, 3:5] = gen.uniform([3.2, 1.4], [4.8, 2.0], (args.boxes, 2))               # cars
    boxes = C.settle_boxes(boxes, rng, args.pixel, gen)
    labels = np.ones((1, args.boxes), np.int64)
    pal = bev_vis.class_palette(1)
    tab = {"boxes": boxes[None], "labels": labels, "ink": 0, "count": np.array([args.boxes], np.int32)}
    dev = "cuda:0"
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                      # noqa: E731
    d_pts, d_off, d_pal = d(pts), d(off), d(pal)
    d_tab = {k: (d(v) if isinstance(v, np.ndarray) else v) for k, v in tab.items()}
    H, W = kernels.bev_grid(rng, args.pixel)
    image = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
    _, _, ws = kernels.render_bev(d_pts, d_off, rng, args.pixel, d_pal, tables=[d_tab], xyz_col=1, image=image)
    torch.cuda.synchronize()
    want, _ = C.render_batch(pts, off, 1, rng, args.pixel, [tab], pal, 2, -1)
    same = bool((image.cpu().numpy() == want).all())

    def op_run():
        for _ in range(args.warmup):
            kernels.render_bev(d_pts, d_off, rng, args.pixel, d_pal, tables=[d_tab], xyz_col=1, image=image, workspace=ws)
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            kernels.render_bev(d_pts, d_off, rng, args.pixel, d_pal, tables=[d_tab], xyz_col=1, image=image, workspace=ws)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        return statistics.median(times)

    def numpy_run():
        t0 = time.perf_counter()
        C.render_batch(pts, off, 1, rng, args.pixel, [tab], pal, 2, -1)
        return (time.perf_counter() - t0) * 1e6

    op_us, np_us = [], []
    for _ in range(3):
        op_us.append(op_run())
        np_us.append(numpy_run())
    print(json.dumps({"bench": "bev_render", "points": args.points, "boxes": args.boxes, "H": H, "W": W, "equal_bytes": same,
                      "op_us_runs": [round(t, 2) for t in op_us], "numpy_us_runs": [round(t, 1) for t in np_us],
                      "op_us": round(statistics.median(op_us), 2), "numpy_us": round(statistics.median(np_us), 1)}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
