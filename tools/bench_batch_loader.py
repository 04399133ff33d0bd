"""Training batches at batch 16: DeviceBatchLoader.prepare_batch (hvpr_amd/batch_loader.py, csrc/collate.hip) against the
per-frame chain it replaces, on the same build, the same frames and the same seed.

Frames: synthetic.kitti_like_frame at ~120 k points, 8 Car boxes each, one KITTI calibration; bank and augmentor config as
tools/bench_augment.py (DATA_AUGMENTOR_3CLASS without the road plane; --bank-scale shrinks the bank).

  chain leg    per frame: FOV flags + compaction + its read (PointPreprocessor.fov_filter); DeviceAugmentor on the batch (one
               read); per frame: range flags + compaction + its read, a host permutation through gather_rows; torch.cat with
               a batch column.  2 B + 1 reads.
  loader leg   prepare_batch: 2 reads.
Both legs draw from the same seed in the same order, so their batches must be bit-equal (`legs_agree`).

Reported per leg: HIP-event time from the first enqueue to the last kernel (median of --iters, p10, p90; it contains the host
gaps between the launches, which is the point), wall time around the call ending in a synchronise, synchronising calls counted
under torch's sync-debug "warn".  The host time of the permutation draws is reported on its own (the reference pays it too).
The two new kernels are timed alone over the augmented batch, HIP events around --reps back-to-back launches, against the bytes
the algorithm needs: count pass rows * 16 read; write pass rows * 16 + kept * 4 (inv_perm) read, kept * 20 written; and
"compact, then gather" (write pass without inv_perm + hvpr_gather_rows_f32 over the flat permutation) next to "scatter the
stores" (write pass with inv_perm).

With --sample-points P (off by default, the default output is unchanged) `sample_points` with NUM_POINTS P stands between the
range mask and the shuffle on both legs (chain: PointPreprocessor.sample_points per frame, one more read each; loader:
sample_points=True, still 2 reads), and the line gains `sample_points`: the count pass with the second ballot and the write
pass through the destination table, timed alone against the count pass and the inv_perm write pass over the same kept rows, and
"compact, then gather the B * P chosen rows" next to it.

    python tools/bench_batch_loader.py [--batch 16] [--bank-scale 0.1] [--sample-points 16384]
Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_augment import CLASSES, RANGE, SIZES, synthetic_bank  # noqa: E402
from hvpr_amd import kernels, preprocess, synthetic  # noqa: E402
from hvpr_amd.augment import DeviceAugmentor  # noqa: E402
from hvpr_amd.batch_loader import DeviceBatchLoader, plan_sample_points, sample_destinations  # noqa: E402
from hvpr_amd.config import cfg_from_yaml_file  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
CALIB = {
    "P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
    "R0": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
                    [0.007402527, 0.004351614, 0.9999631]], np.float32),
    "Tr_velo2cam": np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                             [0.9998621, 0.007523790, 0.01480755, -0.2717806]], np.float32),
}
SHAPE = (375, 1242)


def pct(v, q):
    return round(float(np.percentile(v, q)), 4)


def timed(fn, iters, warmup):
    """[(event ms, wall ms, synchronising calls)] of fn(it)."""
    out = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            t0 = time.perf_counter()
            e0.record()
            fn(it)
            e1.record()
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        syncs = sum("synchroniz" in str(x.message).lower() and "prototype" not in str(x.message) for x in w)
        if it >= warmup:
            out.append((e0.elapsed_time(e1), wall, syncs))
    return np.asarray(out, np.float64)


def kernel_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--bank-scale", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n-az", type=int, default=1900)
    ap.add_argument("--sample-points", type=int, default=0, help="NUM_POINTS of a sample_points step on both legs (0: none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_loader: needs the GPU (there is no CPU path to time)")
    rng = np.random.RandomState(7)
    base = os.path.join(ROOT, "hvpr_amd", "cfgs")
    cfg = cfg_from_yaml_file(os.path.join(base, "dataset_configs", "kitti_dataset.yaml"))
    cfg["DATA_AUGMENTOR"] = cfg_from_yaml_file(os.path.join(base, "dataset_configs", "kitti_augmentor.yaml"))["DATA_AUGMENTOR_3CLASS"]
    cfg["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0]["USE_ROAD_PLANE"] = False
    P = a.sample_points
    if P:
        cfg["DATA_PROCESSOR"].insert(1, {"NAME": "sample_points", "NUM_POINTS": {"train": P, "test": P}})
    bank = synthetic_bank(a.bank_scale, rng)
    bank.on_device()
    B = a.batch
    frames = []
    for b in range(B):
        g = np.zeros((8, 7), np.float32)
        g[:, 0], g[:, 1], g[:, 2] = rng.uniform(3, 60, 8), rng.uniform(-30, 30, 8), rng.uniform(-1.2, -0.8, 8)
        g[:, 3:6], g[:, 6] = SIZES["Car"], rng.uniform(-np.pi, np.pi, 8)
        frames.append({"points": torch.from_numpy(synthetic.kitti_like_frame(100 + b, n_az=a.n_az)).cuda(), "gt_boxes": g,
                       "gt_names": np.array(["Car"] * 8), "calib": CALIB, "image_shape": SHAPE, "frame_id": str(b)})
    loader = DeviceBatchLoader(cfg, CLASSES, lambda i: frames[i], B, bank=bank, training=True, sample_points=bool(P))
    sampler = preprocess.PointPreprocessor(RANGE, num_points=P, training=True) if P else None
    aug = DeviceAugmentor(cfg["DATA_AUGMENTOR"], CLASSES, bank, RANGE)
    pp = preprocess.PointPreprocessor(RANGE, num_points=-1, training=True)
    keep = {}

    def chain(it):
        r = np.random.RandomState(1000 + it)
        fr = [dict(f) for f in frames]
        for f in fr:
            f["points"] = pp.fov_filter(f["points"], f["calib"], f["image_shape"])
        out = aug(fr, r)
        off = np.cumsum([0] + out["num_points"].tolist())
        parts = []
        for b in range(B):
            p = pp.mask_points_and_boxes_outside_range(out["points"][off[b]: off[b + 1]])
            if sampler is not None:
                p = sampler.sample_points(p, r)
            p = preprocess.shuffle_points(p, r)
            parts.append(torch.cat([torch.full((p.shape[0], 1), float(b), device=p.device), p], dim=1))
        keep["chain"] = (torch.cat(parts), out["gt_boxes"])

    def batched(it):
        keep["loader"] = loader.prepare_batch(list(range(B)), np.random.RandomState(1000 + it))

    t_chain = timed(chain, a.iters, a.warmup)
    t_load = timed(batched, a.iters, a.warmup)
    # the same seed once more on both legs, compared
    chain(0)
    batched(0)
    torch.cuda.synchronize()
    lb = keep["loader"]
    agree = bool(torch.equal(keep["chain"][0].view(torch.int32), lb["points"].view(torch.int32)) and
                 torch.equal(keep["chain"][1][:, : lb["gt_boxes"].shape[1]], lb["gt_boxes"]) and not lb["redraw_index"])
    kept = int(lb["points"].shape[0])
    t0 = time.perf_counter()
    r = np.random.RandomState(3)
    for m in np.diff(lb["point_frame_offsets"].cpu().numpy()):
        r.permutation(int(m))
    perm_ms = (time.perf_counter() - t0) * 1e3

    # the two new kernels alone, over an augmented batch (its device offsets, capacity rows behind them)
    st = loader._augment_stage(frames, [np.random.RandomState(5)] * B)
    pts, off = st["points"], st["aug_off_dev"]
    rows, F = pts.shape
    live, m = int(st["aug_off"][-1]), int(st["new_off"][-1])
    new_off, ws = kernels.ragged_select_count(pts, off, 2, range_xy=loader.range_xy)
    perm = np.concatenate([int(st["new_off"][b]) + np.random.RandomState(b).permutation(int(st["new_off"][b + 1] - st["new_off"][b]))
                           for b in range(B)]).astype(np.int32)
    inv = np.empty_like(perm)
    for b in range(B):
        s, e = int(st["new_off"][b]), int(st["new_off"][b + 1])
        inv[perm[s:e]] = np.arange(e - s, dtype=np.int32)
    inv_d, perm_d = torch.from_numpy(inv).cuda(), torch.from_numpy(perm).cuda()
    out5 = torch.empty((m, F + 1), dtype=torch.float32, device=pts.device)
    out4 = torch.empty((rows, F), dtype=torch.float32, device=pts.device)
    flag = torch.zeros((1,), dtype=torch.int32, device=pts.device)
    ms_count = kernel_ms(lambda: kernels.ragged_select_count(pts, off, 2, range_xy=loader.range_xy, new_off=new_off, workspace=ws), a.reps)
    ms_scatter = kernel_ms(lambda: kernels.ragged_select_write(pts, off, 2, new_off, ws, range_xy=loader.range_xy, inv_perm=inv_d,
                                                               batch_column=True, out=out5, flag=flag), a.reps)
    ms_compact = kernel_ms(lambda: kernels.ragged_select_write(pts, off, 2, new_off, ws, range_xy=loader.range_xy, out=out4, flag=flag),
                           a.reps)
    ms_gather = kernel_ms(lambda: preprocess.gather_rows(out4[:m], perm_d), a.reps)
    bytes_count = live * F * 4
    bytes_write = live * F * 4 + m * 4 + m * (F + 1) * 4

    sampled = None
    if P:
        n_off, c_off, ws2 = kernels.ragged_sample_count(pts, off, 2, range_xy=loader.range_xy)
        table, modes, order = np.empty((m, 2), np.int32), np.empty((B,), np.int32), []
        for b in range(B):
            s, e = int(st["new_off"][b]), int(st["new_off"][b + 1])
            plan = plan_sample_points(e - s, int(st["near_off"][b + 1] - st["near_off"][b]), P, np.random.RandomState(b), shuffle=True)
            table[s:e], modes[b] = sample_destinations(plan["order"], e - s), plan["mode"]
            order.append(plan["order"])
        t0 = time.perf_counter()
        for b in range(B):
            s, e = int(st["new_off"][b]), int(st["new_off"][b + 1])
            sample_destinations(plan_sample_points(e - s, int(st["near_off"][b + 1] - st["near_off"][b]), P, np.random.RandomState(b),
                                                   shuffle=True)["order"], e - s)
        plan_ms = (time.perf_counter() - t0) * 1e3
        table_d, modes_d = torch.from_numpy(table).cuda(), torch.from_numpy(modes).cuda()
        outp = torch.empty((B * P, F + 1), dtype=torch.float32, device=pts.device)
        # "compact, then gather": the chosen rows by their flat compacted index (mode 0 frames only know it without the flags;
        # the timing does not depend on which rows are named)
        flat = torch.from_numpy(np.concatenate([int(st["new_off"][b]) + order[b] for b in range(B)]).astype(np.int32)).cuda()
        ms_count2 = kernel_ms(lambda: kernels.ragged_sample_count(pts, off, 2, range_xy=loader.range_xy, new_off=n_off, near_off=c_off,
                                                                  workspace=ws2), a.reps)
        ms_write2 = kernel_ms(lambda: kernels.ragged_sample_write(pts, off, 2, n_off, c_off, modes_d, table_d, P, ws2,
                                                                  range_xy=loader.range_xy, batch_column=True, out=outp, flag=flag),
                              a.reps)
        ms_gather2 = kernel_ms(lambda: preprocess.gather_rows(out4[:m], flat), a.reps)
        bytes_write2 = live * F * 4 + m * 8 + B * P * (F + 1) * 4
        sampled = {"num_points": P, "rows_out": B * P, "host_plan_ms": round(plan_ms, 3),
                   "count_pass": {"ms": round(ms_count2, 5), "against_select_count_ms": round(ms_count, 5)},
                   "write_pass_table": {"ms": round(ms_write2, 5), "against_inv_perm_write_ms": round(ms_scatter, 5),
                                        "bytes": int(bytes_write2), "tb_per_s": round(bytes_write2 / ms_write2 / 1e9, 3),
                                        "share_of_achievable_hbm": round(bytes_write2 / (ms_write2 * 1e-3) / HBM_ACHIEVABLE, 3)},
                   "compact_then_gather": {"compact_ms": round(ms_compact, 5), "gather_ms": round(ms_gather2, 5),
                                           "ms": round(ms_compact + ms_gather2, 5), "note": "without the batch column"}}

    def leg(t):
        return {"event_ms_median": pct(t[:, 0], 50), "event_ms_p10": pct(t[:, 0], 10), "event_ms_p90": pct(t[:, 0], 90),
                "wall_ms_median": pct(t[:, 1], 50), "sync_calls": int(np.median(t[:, 2]))}

    line = {
        "bench": "batch_loader", "batch": B, "points_in": int(sum(f["points"].shape[0] for f in frames)), "points_augmented": live,
        "points_out": kept, "bank_objects": len(bank), "iters": a.iters, "chain": leg(t_chain), "loader": leg(t_load),
        "legs_agree": agree, "permutation_draws_host_ms": round(perm_ms, 3),
        "count_pass": {"ms": round(ms_count, 5), "bytes": int(bytes_count), "tb_per_s": round(bytes_count / ms_count / 1e9, 3),
                       "share_of_achievable_hbm": round(bytes_count / (ms_count * 1e-3) / HBM_ACHIEVABLE, 3),
                       "note": "two launches: tiles, then the one-workgroup scan"},
        "write_pass_scatter": {"ms": round(ms_scatter, 5), "bytes": int(bytes_write), "tb_per_s": round(bytes_write / ms_scatter / 1e9, 3),
                               "share_of_achievable_hbm": round(bytes_write / (ms_scatter * 1e-3) / HBM_ACHIEVABLE, 3)},
        "compact_then_gather": {"compact_ms": round(ms_compact, 5), "gather_ms": round(ms_gather, 5),
                                "ms": round(ms_compact + ms_gather, 5), "note": "without the batch column"}}
    if sampled is not None:
        line["sample_points"] = sampled
    print(json.dumps(line))


if __name__ == "__main__":
    main()
