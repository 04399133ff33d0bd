"""KITTI AP table (3 classes, bbox + BEV + 3-D + AOS): seconds of the host evaluator (hvpr_amd/kitti_eval.py) and of the device
evaluator (hvpr_amd/kitti_eval_device.py) on F frames of synthetic annotations.

The frames are tests/golden/make_golden.synthetic_kitti_annos tiled 24 at a time with a different seed per tile (2 to 10 ground
truths and about as many detections per frame).  Wall clock around get_official_eval_result, the device synchronised before and
after; the device figure includes building and uploading the annotation tables.  The host evaluator runs at F = 24 and 96 only
(it launches and synchronises once per frame and metric and interprets every frame x class x difficulty x overlap set x
threshold); its figure at 3769 frames, the KITTI val split, is printed as a PROJECTION (seconds per frame at 96 x 3769), which
nobody measured.  The device evaluator runs at 24, 96 and 3769.  One JSON line per measurement; both results are compared.

    python tools/bench_kitti_ap.py [--host-frames 24 96] [--device-frames 24 96 3769] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
CLASSES = ["Car", "Pedestrian", "Cyclist"]


def tiled_annos(n_frames):
    from make_golden import synthetic_kitti_annos
    gts, dts = [], []
    for tile in range((n_frames + 23) // 24):
        g, d = synthetic_kitti_annos(1212 + tile, 24)
        gts += g
        dts += d
    return gts[:n_frames], dts[:n_frames]


def timed(fn, reps):
    out, secs = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return out, float(np.median(secs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--host-frames", nargs="*", type=int, default=[24, 96])
    ap.add_argument("--device-frames", nargs="*", type=int, default=[24, 96, 3769])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from hvpr_amd import kitti_eval, kitti_eval_device
    g, d = tiled_annos(24)
    kitti_eval_device.get_official_eval_result(g, d, CLASSES)        # warm-up: library load, first launches
    results, host_s = {}, {}
    for F in args.host_frames:
        g, d = tiled_annos(F)
        (_, ret), s = timed(lambda: kitti_eval.get_official_eval_result(g, d, CLASSES), 1)
        results["host", F], host_s[F] = ret, s
        print(json.dumps({"evaluator": "host", "frames": F, "boxes_gt": sum(len(a["name"]) for a in g),
                          "boxes_dt": sum(len(a["name"]) for a in d), "seconds": round(s, 4)}), flush=True)
    for F in args.device_frames:
        g, d = tiled_annos(F)
        (_, ret), s = timed(lambda: kitti_eval_device.get_official_eval_result(g, d, CLASSES), args.reps)
        line = {"evaluator": "device", "frames": F, "boxes_gt": sum(len(a["name"]) for a in g),
                "boxes_dt": sum(len(a["name"]) for a in d), "seconds": round(s, 4), "reps": args.reps}
        if ("host", F) in results:
            ref = results["host", F]
            line["max_abs_diff_to_host"] = max(abs(ret[k] - ref[k]) for k in ref)
            line["host_over_device"] = round(host_s[F] / s, 1)
        print(json.dumps(line), flush=True)
    if host_s:
        F = max(host_s)
        print(json.dumps({"evaluator": "host", "frames": 3769, "PROJECTED_seconds": round(host_s[F] / F * 3769, 1),
                          "note": f"projection from {F} frames, linear in the frames; not measured"}), flush=True)


if __name__ == "__main__":
    main()
