"""The "attend over k rows" op (hvpr_attend_rows_fwd_f32 through map_to_bev._AttendRows) against the torch expression it replaced
in map_to_bev.py (_GatherRows -> mul -> sum -> softmax -> mul -> sum, kept HERE as the comparator), forward and forward + backward,
at one frame (M = 3 900 pillars, N = 16 384 points) and batch 16 (M = 61 000, N = 262 144), k = 20.

Picks: a point is picked ~5 times on average and a few by hundreds (16 384 points against ~3 900 pillars x 20) — each
pick comes from a lognormal popularity over the frame's points.  The two forms alternate in one process; device-event times after
warm-up (median of the repeats, per call) and torch.cuda.max_memory_allocated over one forward + backward of each form.  The edge
plan (one argsort of the picks) is built once outside the timed region for both forms: in the training step it is shared.

    python tools/bench_attend.py [--reps 20]
Prints one JSON line per size.  Needs the GPU: there is nothing to fall back to."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hvpr_amd import kernels, map_to_bev  # noqa: E402

DEV = "cuda:0"
K, C = 20, 64


def picks(frames, m_per_frame, n_per_frame, gen):
    """(M, K) int64 picks, frame by frame into the frame's own points; popularity lognormal(sigma 1.5): mean ~4.8 picks per point,
    the most popular points of a frame picked by several hundred pillars, no point twice in one pillar."""
    out = []
    for f in range(frames):
        logp = (torch.randn(n_per_frame, generator=gen) * 1.5).to(DEV)
        u = torch.rand(m_per_frame, n_per_frame, generator=gen).to(DEV).clamp_(1e-12, 1 - 1e-7)
        # Gumbel top-k = sampling K distinct points per pillar with probabilities ~ exp(logp)
        out.append(torch.topk(logp[None, :] - torch.log(-torch.log(u)), K, dim=1)[1] + f * n_per_frame)
    return torch.cat(out, 0)


def torch_form(q, rows, idx, plan):
    pos = map_to_bev._GatherRows.apply(rows, idx, plan)
    w = torch.softmax((q.unsqueeze(1) * pos).sum(dim=2), dim=1)
    return (w.detach().unsqueeze(2) * pos).sum(dim=1)


def op_form(q, rows, idx, plan):
    return map_to_bev._AttendRows.apply(q, rows, idx, plan)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run(name, frames, m_per_frame, n_per_frame, reps, rounds=5):
    g = torch.Generator().manual_seed(frames)
    M, N = frames * m_per_frame, frames * n_per_frame
    idx = picks(frames, m_per_frame, n_per_frame, g)
    cnt = torch.bincount(idx.reshape(-1), minlength=N)
    q = torch.relu(torch.randn(M, C, generator=g)).to(DEV)
    rows = (torch.relu(torch.randn(N, C, generator=g)) * 0.5).to(DEV).requires_grad_(True)
    cot = torch.randn(M, C, generator=g).to(DEV)
    plan = kernels.EdgePlan(idx, N)
    plan.build().edge_rows(K), plan.idx32()
    forms = {"torch": torch_form, "op": op_form}

    def fwd(f):
        with torch.no_grad():
            f(q, rows, idx, plan)

    def fwd_bwd(f):
        rows.grad = None
        f(q, rows, idx, plan).backward(cot)

    res = {n: {"fwd_us": [], "fwd_bwd_us": []} for n in forms}
    for n, f in forms.items():                 # warm-up; also the agreement of the two forms
        fwd_bwd(f)
        res[n]["out"], res[n]["grad"] = f(q, rows, idx, plan).detach(), rows.grad.clone()
    for _ in range(rounds):                    # alternate the two forms
        for n, f in forms.items():
            res[n]["fwd_us"].append(timed(lambda: fwd(f), reps))
            res[n]["fwd_bwd_us"].append(timed(lambda: fwd_bwd(f), reps))
    for n, f in forms.items():
        rows.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fwd_bwd(f)
        torch.cuda.synchronize()
        res[n]["peak_rise_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    moved = M * K * 256 + 2 * M * C * 4 + 2 * M * K * 4
    rec = {"workload": name, "M": M, "N": N, "k": K, "picks_per_point_mean": round(float(cnt.float().mean()), 2), "picks_per_point_max": int(cnt.max()),
           "gathered_MiB": round(M * K * C * 4 / 2**20, 1), "fwd_bytes_MB": round(moved / 1e6, 1)}
    for n in forms:
        for key in ("fwd_us", "fwd_bwd_us"):
            v = res[n][key]
            rec[f"{n}_{key}"] = round(float(np.median(v)), 1)
            rec[f"{n}_{key}_minmax"] = [round(min(v), 1), round(max(v), 1)]
        rec[f"{n}_peak_rise_MiB"] = res[n]["peak_rise_MiB"]
    rec["op_fwd_GBps"] = round(moved / rec["op_fwd_us"] / 1e3, 1)
    rec["max_abs_diff_out"] = float((res["op"]["out"] - res["torch"]["out"]).abs().max())
    rec["rel_diff_grad"] = float((res["op"]["grad"] - res["torch"]["grad"]).norm() / res["torch"]["grad"].norm())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attend.py needs an MI355X: the op has no CPU path")
    run("one frame", 1, 3900, 16384, args.reps)
    run("batch 16", 16, 3812, 16384, args.reps)
