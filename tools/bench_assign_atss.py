"""The ATSS target assigner beside the nearest-axis one, on tools/bench_assign.py's workload (a batch of 16 at the full anchor sets of
hvpr_car.yaml and hvpr_3class.yaml, --gts uniform ground truths a frame padded to --pad rows), three legs:

    old        hvpr_assign_targets_f32 (nearest-axis BEV IoU; the leg of bench_assign.py, on the same build)
    atss_bev   hvpr_assign_targets_atss_f32, TOPK --topk, match_height 0 (rotated BEV IoU)
    atss_3d    hvpr_assign_targets_atss_f32, TOPK --topk, match_height 1 (rotated 3-D IoU)

A run is --reps assignments of all anchor sets of the configuration between two device events after --warmup assignments; the
legs alternate run by run, --runs runs each, and the median run is reported per assignment.  One JSON line per configuration.  The
per-launch split comes from a kernel trace of this command with --reps 20 --runs 1.

    python tools/bench_assign_atss.py [--reps 200] [--runs 3] [--gts 20] [--pad 50] [--batch 16] [--topk 9]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_assign as BA  # noqa: E402
from hvpr_amd import kernels  # noqa: E402
from hvpr_amd.config import hvpr_3class_cfg, hvpr_car_cfg  # noqa: E402


class Case(BA.Case):
    def __init__(self, cfg, gt, topk):
        super().__init__(cfg, gt)
        self.topk = topk
        q = kernels.lib().hvpr_assign_targets_atss_workspace_bytes
        self.ws_atss = torch.empty(max(int(q(self.B, self.G, s[0].shape[0], topk)) for s in self.sets), dtype=torch.uint8, device=BA.DEV)

    def assign(self, leg, clipped=None):
        if leg == "old":
            return super().assign(leg)
        off = 0
        for a, per_loc, *_ in self.sets:
            kernels.call("hvpr_assign_targets_atss_f32", a, a.shape[0], self.gt, self.B, self.G, self.n_classes, self.topk, int(leg == "atss_3d"),
                         per_loc, self.stride, off, self.A, self.labels, self.targets, self.weights, self.pos, self.ws_atss,
                         self.ws_atss.numel(), kernels._stream())
            off += per_loc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--pad", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--topk", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assign_atss needs the GPU: nothing is timed without one")
    legs = ("old", "atss_bev", "atss_3d")
    for name, cfg in (("hvpr_car", hvpr_car_cfg()), ("hvpr_3class", hvpr_3class_cfg())):
        case = Case(cfg, BA.ground_truths(cfg, args.batch, args.gts, args.pad, 2100), args.topk)
        positives = {}
        for leg in legs:
            for _ in range(args.warmup):
                case.assign(leg)
            torch.cuda.synchronize()
            positives[leg] = int((case.labels > 0).sum())
        ms = {leg: [] for leg in legs}
        for _ in range(args.runs):
            for leg in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    case.assign(leg)
                e1.record()
                torch.cuda.synchronize()
                ms[leg].append(e0.elapsed_time(e1) / args.reps)
        out = {"config": name, "batch": args.batch, "gts_per_frame": args.gts, "padded_rows": args.pad, "topk": args.topk,
               "anchors_per_frame": case.A, "anchor_sets": len(case.sets), "reps": args.reps, "runs": args.runs,
               "workspace_bytes": int(case.ws_atss.numel())}
        for leg in legs:
            out[leg + "_ms"] = round(float(np.median(ms[leg])), 4)
            out[leg + "_runs_ms"] = [round(x, 4) for x in ms[leg]]
            out["positives_" + leg] = positives[leg]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
