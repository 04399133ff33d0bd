"""Plain PointPillars beside HVPR on the same kernels: what the memory module, the scale stream and the attentive branches cost.

    pointpillar   detector.GraphedForward of pointpillar.yaml (432 x 496 pillars, head 216 x 248) at batch 1, frames/s
    hvpr_3class   detector.GraphedForward of hvpr_3class.yaml (296 x 248, head 296 x 248) at batch 1, in the same process
    vfe           kernels.pillar_vfe_plain_fwd alone at M = 40 000, P = 32, c_out = 64 against the same expression in plain torch on
                  the GPU (PillarVFE.forward's chain of ops on the folded layer)

Frames are synthetic.kitti_like_frame masked to each config's range; a captured graph has one input shape, so PointPillars' frames
are cut to the shortest of the --frames frames (hvpr_3class samples 16 384 points itself).  A run is --reps replays (calls) over
the frames in turn between two device events, after --warmup replays per shape; the two models alternate run by run, --runs runs
each.  One JSON line: the median run and every run of each leg.

    python tools/bench_pointpillar.py [--reps 200] [--runs 3] [--warmup 20] [--frames 8]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hvpr_amd import detector, kernels, synthetic, synthetic_weights  # noqa: E402
from hvpr_amd.config import hvpr_3class_cfg, pointpillar_cfg  # noqa: E402

DEV = "cuda:0"
CLS_BIAS = -4.59511985013459          # -log(99), the head's own initialisation (bench.py times the same)


def _batch(points):
    pts = np.concatenate([np.zeros((len(points), 1), np.float32), points], axis=1)
    return {"points": torch.from_numpy(pts).to(DEV), "batch_size": 1}


def _model(cfg):
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
    synthetic_weights.load_synthetic(model, seed=0, cls_bias=CLS_BIAS)
    return model.to(DEV).eval()


def pointpillar_leg(n_frames):
    cfg = pointpillar_cfg()
    frames = [synthetic.mask_points_by_range(synthetic.kitti_like_frame(100 + i), cfg.DATA_CONFIG.POINT_CLOUD_RANGE) for i in range(n_frames)]
    n = min(len(f) for f in frames)
    batches = [_batch(np.ascontiguousarray(f[:n])) for f in frames]
    model = _model(cfg)
    return {"graph": detector.GraphedForward(model, batches[0]), "batches": batches, "model": model, "points": n}


def hvpr_leg(n_frames):
    batches = [_batch(synthetic.hvpr_frame(100 + i)) for i in range(n_frames)]
    model = _model(hvpr_3class_cfg())
    return {"graph": detector.GraphedForward(model, batches[0]), "batches": batches, "model": model, "points": 16384}


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_pfn(vox, num, coords, w, b, vs, off):
    """PillarVFE.forward (pillar_vfe.py:94-124) with the folded layer, op for op, in torch on the device."""
    mean = vox[:, :, :3].sum(dim=1, keepdim=True) / num.to(vox.dtype).view(-1, 1, 1)
    f_cluster = vox[:, :, :3] - mean
    c = coords.to(vox.dtype)
    f_center = torch.stack([vox[:, :, 0] - (c[:, 3:4] * vs[0] + off[0]), vox[:, :, 1] - (c[:, 2:3] * vs[1] + off[1]),
                            vox[:, :, 2] - (c[:, 1:2] * vs[2] + off[2])], dim=-1)
    feats = torch.cat([vox, f_cluster, f_center], dim=-1)
    mask = (num.view(-1, 1) > torch.arange(vox.shape[1], device=vox.device).view(1, -1)).unsqueeze(-1).to(vox.dtype)
    feats = feats * mask
    return torch.relu(torch.nn.functional.linear(feats, w, b)).max(dim=1)[0], mask


def vfe_leg(reps, runs, warmup, M=40000, P=32, C=64):
    rng = np.random.default_rng(5)
    vs, lo = [0.16, 0.16, 4.0], [0.0, -39.68, -3.0]
    off = [vs[i] / 2 + lo[i] for i in range(3)]
    n = rng.integers(1, P + 1, M).astype(np.int32)
    cells = rng.permutation(432 * 496)[:M]
    cx, cy = cells % 432, cells // 432
    u = rng.random((M, P, 4))
    vox = np.stack([lo[0] + (cx[:, None] + u[..., 0]) * vs[0], lo[1] + (cy[:, None] + u[..., 1]) * vs[1], lo[2] + u[..., 2] * vs[2],
                    u[..., 3]], axis=-1) * (np.arange(P)[None, :] < n[:, None])[..., None]
    coords = np.stack([np.zeros(M, np.int64), np.zeros(M, np.int64), cy, cx], axis=1).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    vox, n, coords = t(vox.astype(np.float32)), t(n), t(coords)
    w, b = t(rng.normal(0, 0.45, (C, 10)).astype(np.float32)), t(rng.normal(0, 0.3, (C,)).astype(np.float32))
    legs = {"kernel": lambda i: kernels.pillar_vfe_plain_fwd(vox, n, coords, w, b, vs, off),
            "torch": lambda i: torch_pfn(vox, n, coords, w, b, vs, off)}
    a, ref = legs["kernel"](0)[0], legs["torch"](0)[0]
    err = float((a - ref).abs().max() / ref.abs().max())
    us = {k: [] for k in legs}
    for k, fn in legs.items():
        _timed(fn, warmup)
    for _ in range(runs):
        for k, fn in legs.items():
            us[k].append(1e3 * _timed(fn, reps))
    bytes_moved = M * (P * 16 + 16 + 4) + M * 4 * C + M * P * 4          # in, features out, mask out
    out = {"M": M, "P": P, "c_out": C, "max_norm_diff_kernel_torch": err, "bytes": bytes_moved}
    for k in legs:
        out[k + "_us"] = round(float(np.median(us[k])), 2)
        out[k + "_runs_us"] = [round(x, 2) for x in us[k]]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--vfe-only", action="store_true", help="the encoder leg alone (for a kernel trace of this command)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointpillar needs the GPU: nothing is timed without one")
    torch.set_grad_enabled(False)
    if args.vfe_only:
        print(json.dumps({"vfe": vfe_leg(args.reps, args.runs, args.warmup)}), flush=True)
        return
    legs = {"pointpillar": pointpillar_leg(args.frames), "hvpr_3class": hvpr_leg(args.frames)}
    boxes = {}
    for name, leg in legs.items():
        g, bs = leg["graph"], leg["batches"]
        _timed(lambda i: g(bs[i % len(bs)]), args.warmup)
        g.check_status()
        boxes[name] = int(g(bs[0])[0][0]["pred_count"].item())
    ms = {name: [] for name in legs}
    for _ in range(args.runs):
        for name, leg in legs.items():
            g, bs = leg["graph"], leg["batches"]
            ms[name].append(_timed(lambda i: g(bs[i % len(bs)]), args.reps))
    out = {"batch": 1, "reps": args.reps, "runs": args.runs, "frames": args.frames}
    for name, leg in legs.items():
        med = float(np.median(ms[name]))
        out[name] = {"frames_per_s": round(1e3 / med, 1), "ms": round(med, 4), "runs_ms": [round(x, 4) for x in ms[name]],
                     "points_per_frame": int(leg["points"]), "boxes_frame0": boxes[name]}
    out["hvpr_over_pointpillar_ms"] = round(out["hvpr_3class"]["ms"] / out["pointpillar"]["ms"], 3)
    out["vfe"] = vfe_leg(args.reps, args.runs, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
