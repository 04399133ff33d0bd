"""Target assignment of a batch of 16 at the full anchor sets of hvpr_car.yaml and hvpr_3class.yaml, three ways:

    old        hvpr_assign_targets_f32 (nearest-axis BEV IoU)
    ex_flags0  hvpr_assign_targets_ex_f32 with match_height 0 and norm_by_num_examples 0 (forwards to the old entry point)
    ex_match   hvpr_assign_targets_ex_f32 with match_height 1 (rotated 3-D IoU: rejects on the whole table, clip on packed survivors)

About --gts ground truths a frame (uniform over the range, classes in turn) padded with zero rows to --pad.  A run is --reps
assignments of all anchor sets of the configuration between two device events after --warmup assignments; the three legs alternate
run by run, --runs runs each, and the median run is reported per assignment, next to the number of (anchor, ground truth) pairs
that reached the clip (read from the workspace after a call, summed over the anchor sets).  One JSON line per configuration.

    python tools/bench_assign.py [--reps 200] [--runs 3] [--gts 20] [--pad 50] [--batch 16]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvpr_amd import anchor_head, kernels  # noqa: E402
from hvpr_amd.config import hvpr_3class_cfg, hvpr_car_cfg  # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)


def ground_truths(cfg, batch, n, pad, seed):
    r = np.random.default_rng(seed)
    pcr = cfg.DATA_CONFIG.POINT_CLOUD_RANGE
    nc = len(cfg.CLASS_NAMES)
    g = np.zeros((batch, pad, 8), np.float32)
    for b in range(batch):
        cls = np.arange(n) % nc
        g[b, :n, 0] = r.uniform(pcr[0] + 2, pcr[3] - 2, n)
        g[b, :n, 1] = r.uniform(pcr[1] + 2, pcr[4] - 2, n)
        g[b, :n, 2] = r.uniform(-1.2, -0.6, n)
        g[b, :n, 3:6] = SIZES[cls] * r.uniform(0.85, 1.15, (n, 3))
        g[b, :n, 6] = r.uniform(-np.pi, np.pi, n)
        g[b, :n, 7] = cls + 1
    return torch.from_numpy(g).to(DEV)


class Case:
    def __init__(self, cfg, gt):
        head = anchor_head.AnchorHeadSingle(model_cfg=cfg.MODEL.DENSE_HEAD, input_channels=64, num_class=len(cfg.CLASS_NAMES),
                                            class_names=cfg.CLASS_NAMES, grid_size=np.array([296, 248, 1]),
                                            point_cloud_range=np.array(cfg.DATA_CONFIG.POINT_CLOUD_RANGE, np.float32))
        acfg = cfg.MODEL.DENSE_HEAD.ANCHOR_GENERATOR_CONFIG
        self.sets = [(a.reshape(-1, 7).to(DEV).float().contiguous(), int(a.shape[3] * a.shape[4]), list(cfg.CLASS_NAMES).index(c["class_name"]),
                      float(c["matched_threshold"]), float(c["unmatched_threshold"])) for a, c in zip(head.anchors, acfg)]
        self.n_classes = len(cfg.CLASS_NAMES)
        self.gt = gt
        self.B, self.G = int(gt.shape[0]), int(gt.shape[1])
        self.stride = sum(s[1] for s in self.sets)
        self.A = self.sets[0][0].shape[0] // self.sets[0][1] * self.stride
        self.labels = torch.empty((self.B, self.A), dtype=torch.int32, device=DEV)
        self.targets = torch.empty((self.B, self.A, 7), device=DEV)
        self.weights = torch.empty((self.B, self.A), device=DEV)
        self.pos = torch.zeros((self.B,), dtype=torch.int32, device=DEV)
        L = kernels.lib()
        need = max(int(L.hvpr_assign_targets_ex_workspace_bytes(self.B, self.G, s[0].shape[0], 1)) for s in self.sets)
        self.ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def assign(self, leg, clipped=None):
        off = 0
        for a, per_loc, ci, matched, unmatched in self.sets:
            args = (a, a.shape[0], self.gt, self.B, self.G, ci, self.n_classes, matched, unmatched, per_loc, self.stride, off, self.A,
                    self.labels, self.targets, self.weights, self.pos)
            if leg == "old":
                kernels.call("hvpr_assign_targets_f32", *args, self.ws, self.ws.numel(), kernels._stream())
            else:
                kernels.call("hvpr_assign_targets_ex_f32", *args, int(leg == "ex_match"), 0, self.ws, self.ws.numel(), kernels._stream())
            if clipped is not None:
                clipped.append(int(self.ws[:8].view(torch.int64).item()))
            off += per_loc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--pad", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assign needs the GPU: nothing is timed without one")
    legs = ("old", "ex_flags0", "ex_match")
    for name, cfg in (("hvpr_car", hvpr_car_cfg()), ("hvpr_3class", hvpr_3class_cfg())):
        case = Case(cfg, ground_truths(cfg, args.batch, args.gts, args.pad, 2100))
        clipped = []
        case.assign("ex_match", clipped)
        labels_match = case.labels.clone()
        for leg in legs:
            for _ in range(args.warmup):
                case.assign(leg)
        torch.cuda.synchronize()
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
        case.assign("old")
        torch.cuda.synchronize()
        out = {"config": name, "batch": args.batch, "gts_per_frame": args.gts, "padded_rows": args.pad, "anchors_per_frame": case.A,
               "anchor_sets": len(case.sets), "reps": args.reps, "runs": args.runs}
        for leg in legs:
            out[leg + "_ms"] = round(float(np.median(ms[leg])), 4)
            out[leg + "_runs_ms"] = [round(x, 4) for x in ms[leg]]
        out["pairs_in_table"] = int(args.batch * args.pad * sum(s[0].shape[0] for s in case.sets))
        out["pairs_clipped"] = int(sum(clipped))
        out["positives_nearest_axis"] = int((case.labels > 0).sum())
        out["positives_match_height"] = int((labels_match > 0).sum())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
