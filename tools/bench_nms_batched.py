"""Rotated NMS of S candidate lists: one hvpr_nms_bev_batched_f32 call against a loop of S hvpr_nms_bev_f32 calls.

4096 clustered car-sized candidates per list (many overlapping pairs), a random ranking, threshold 0.1, at most --max-keep
survivors; S in {1, 2, 4, 16}.  HIP events around each leg, the legs alternating repetition by repetition; after a warm-up the
median of --reps repetitions is reported with the 10th and 90th percentile.  One JSON line per S.

    python tools/bench_nms_batched.py [S ...] [--reps 30] [--warmup 5] [--max-keep 500] [--loop-only]

--loop-only times the loop leg alone and needs only the single entry point, so it also runs on a library from before the
batched call: HVPR_AMD_LIB=/path/to/older/libhvpr_amd.so python tools/bench_nms_batched.py --loop-only.  (In a build that has
the batched call the single call IS the batched kernel with one segment, so its own loop leg is not an independent baseline.)
The library is loaded here with ctypes, not through hvpr_amd._lib.lib(), which insists on every symbol of its own version; the
prototypes come from hvpr_amd._lib.SIGNATURES (include/hvpr_amd.h)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
N, THRESH = 4096, 0.1
sys.path.insert(0, ROOT)
from hvpr_amd._lib import SIGNATURES  # noqa: E402  (the header's prototypes; the library itself is loaded here)


def car_boxes(rng, n, spread=40.0):
    """Car-sized boxes around n / 6 cluster centres, so that many pairs overlap (the generator of the NMS tests)."""
    centres = rng.uniform([0, -20], [spread, 20], (max(n // 6, 1), 2))
    xy = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.8, (n, 2))
    z = rng.normal(-1.0, 0.2, (n, 1))
    size = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (n, 3))
    yaw = rng.uniform(-np.pi, np.pi, (n, 1))
    return np.concatenate([xy, z, size, yaw], 1).astype(np.float32)


def load(loop_only):
    path = os.environ.get("HVPR_AMD_LIB", os.path.join(ROOT, "hvpr_amd", "libhvpr_amd.so"))
    L = ctypes.CDLL(path)
    names = ["hvpr_nms_workspace_bytes", "hvpr_nms_bev_f32"]
    if not loop_only:
        names += ["hvpr_nms_bev_batched_workspace_bytes", "hvpr_nms_bev_batched_f32"]
    for name in names:
        getattr(L, name).restype, getattr(L, name).argtypes = SIGNATURES[name]
    return L, path


def percentiles(ms):
    a = np.sort(np.asarray(ms))
    return {"median_us": round(1e3 * float(np.median(a)), 1), "p10_us": round(1e3 * float(np.percentile(a, 10)), 1),
            "p90_us": round(1e3 * float(np.percentile(a, 90)), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("segments", nargs="*", type=int, default=[1, 2, 4, 16])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-keep", type=int, default=500)
    ap.add_argument("--loop-only", action="store_true")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20")
    L, path = load(args.loop_only)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for S in args.segments:
        rng = np.random.default_rng(100 + S)
        boxes = torch.from_numpy(np.stack([car_boxes(rng, N) for _ in range(S)])).to(DEV)
        order = torch.from_numpy(np.stack([rng.permutation(N) for _ in range(S)]).astype(np.int32)).to(DEV)
        counts = torch.full((S,), N, dtype=torch.int32, device=DEV)
        K = args.max_keep
        keep_l, kc_l = torch.zeros((S, K), dtype=torch.int32, device=DEV), torch.zeros((S,), dtype=torch.int32, device=DEV)
        ws_l = torch.empty(L.hvpr_nms_workspace_bytes(N), dtype=torch.uint8, device=DEV)

        def loop():
            for s in range(S):
                st = L.hvpr_nms_bev_f32(boxes[s].data_ptr(), 7, order[s].data_ptr(), counts[s:s + 1].data_ptr(), N, THRESH, K, 1,
                                        keep_l[s].data_ptr(), kc_l[s:s + 1].data_ptr(), ws_l.data_ptr(), ws_l.numel(), stream())
                assert st == 0, st
        legs = {"loop": loop}
        if not args.loop_only:
            keep_b, kc_b = torch.zeros((S, K), dtype=torch.int32, device=DEV), torch.zeros((S,), dtype=torch.int32, device=DEV)
            ws_b = torch.empty(L.hvpr_nms_bev_batched_workspace_bytes(S, N), dtype=torch.uint8, device=DEV)

            def batched():
                st = L.hvpr_nms_bev_batched_f32(boxes.data_ptr(), 7, N * 7, 1, order.data_ptr(), counts.data_ptr(), S, N, THRESH, K, 1,
                                                keep_b.data_ptr(), kc_b.data_ptr(), ws_b.data_ptr(), ws_b.numel(), stream())
                assert st == 0, st
            legs["batched"] = batched
        times = {k: [] for k in legs}
        for rep in range(args.warmup + args.reps):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        out = {"segments": S, "candidates": N, "max_keep": K, "reps": args.reps, "lib": path,
               "kept": kc_l.cpu().tolist(), **{k: percentiles(v) for k, v in times.items()}}
        if not args.loop_only:      # the two legs computed the same thing
            assert torch.equal(kc_b, kc_l) and torch.equal(keep_b, keep_l), "batched and looped survivors differ"
            out["batched_over_loop"] = round(out["batched"]["median_us"] / out["loop"]["median_us"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
