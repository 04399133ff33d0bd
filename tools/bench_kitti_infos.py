"""get_infos' num_points_in_gt: the device form (hvpr_amd/kitti_dataset.py, csrc/kitti_infos.hip) against the same count in numpy
over the CPU native points_in_boxes_cpu (tests/kitti_infos_cases.count_host), on the same build.  (The reference's own form, one
scipy Delaunay and find_simplex per box, is slower than the host leg here; it is not measured.)

Scenes: the workload of tools/bench_gt_database.py — synthetic.kitti_like_frame at about 123 k points, 64 frames, 8 boxes each set
down on points of the frame — under a KITTI calibration; every point within 1e-3 m of a box face, 1e-3 px of an image border or
1e-3 m of depth 0 is removed first (the margin rule of the tests), so both legs count the same points and are compared exactly.

  host leg       count_host per frame, one thread, wall clock.
  device leg 1   frames already resident: per chunk the count call and the ONE host read; HIP events around the whole and around
                 the calls, warm-up, median of --iters with p10-p90.
  device leg 2   InfoCounter.count from numpy frames (get_infos' count path): packing into the pinned buffer, the upload, the call,
                 the read; wall clock ending in a synchronise, median of --iters-upload.

    python tools/bench_kitti_infos.py [--frames 64] [--n-az 2048] [--boxes 8] [--frames-per-call 32]
Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gt_database_cases as GC  # noqa: E402
import kitti_infos_cases as KC  # noqa: E402
from hvpr_amd import kernels, synthetic  # noqa: E402
from hvpr_amd.gt_database import StagedChunk  # noqa: E402
from hvpr_amd.kitti_dataset import InfoCounter  # noqa: E402

HBM_BYTES_PER_S = 8.0e12           # MI355X peak


def scene(n_frames, n_az, n_boxes, rng):
    frames = []
    for f in range(n_frames):
        pts = synthetic.kitti_like_frame(1000 + f, n_az=n_az)
        calib, shape = KC.make_calib(f % 3), np.array((375 - f % 3, 1242 - 9 * (f % 3)), np.int32)
        seen = np.nonzero(KC.BC.fov_flag(pts, calib, shape))[0]
        pick = np.concatenate([rng.choice(seen, n_boxes - n_boxes // 4, replace=False), rng.choice(len(pts), n_boxes // 4, replace=False)])
        boxes = np.zeros((n_boxes, 7))
        for i, at in enumerate(pts[pick, :3].astype(np.float64)):
            size = np.asarray(GC.SIZES[["Car", "Pedestrian", "Cyclist", "Van"][i % 4]]) * rng.uniform(0.9, 1.1)
            boxes[i] = [at[0] + rng.uniform(-0.3, 0.3), at[1] + rng.uniform(-0.3, 0.3), at[2] + size[2] / 2 - 0.1, *size,
                        rng.uniform(-np.pi, np.pi)]
        kept = KC.clean(pts, boxes, calib, shape)
        assert len(kept) >= 0.98 * len(pts)
        frames.append({"points": kept, "boxes": boxes, "calib": calib, "image_shape": shape})
    return frames


def pct(v, q):
    return round(float(np.percentile(v, q)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--n-az", type=int, default=2048)
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--frames-per-call", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--iters-upload", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kitti_infos: needs the GPU (nothing here is measured without one)")
    frames = scene(a.frames, a.n_az, a.boxes, np.random.RandomState(23))
    n_points = sum(len(f["points"]) for f in frames)
    per = a.frames_per_call

    # ---- host leg
    torch.set_num_threads(1)
    t_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, want_fov = KC.counts_of(frames)
        t_host.append(time.perf_counter() - t0)
    want = np.concatenate(want)

    # ---- device leg 1: resident frames
    dev = torch.device("cuda:0")
    chunks = []
    for c0 in range(0, a.frames, per):
        part = frames[c0: c0 + per]
        chunks.append(StagedChunk([torch.from_numpy(f["points"]).to(dev) for f in part], [f["boxes"] for f in part], dev,
                                  calibs=[f["calib"] for f in part], image_shapes=[f["image_shape"] for f in part]))   # a staging buffer each
    count_host = torch.empty((a.frames * a.boxes,), dtype=torch.int32).pin_memory()
    ws = None
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_all, t_call = [], []
    for it in range(a.warmup + a.iters):
        e = [ev() for _ in range(2 + 2 * len(chunks))]
        k, reads = 0, 0
        e[0].record()
        for j, ch in enumerate(chunks):
            e[2 + 2 * j].record()
            cnt, _, ws = ch.count(ws)
            e[3 + 2 * j].record()
            count_host[k: k + ch.n_obj].copy_(cnt)                              # the one read of the chunk
            k, reads = k + ch.n_obj, reads + 1
        e[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            t_all.append(e[0].elapsed_time(e[1]))
            t_call.append(sum(e[2 + 2 * j].elapsed_time(e[3 + 2 * j]) for j in range(len(chunks))))
    agree = count_host.numpy().tolist() == want.tolist()
    fov = torch.cat([ch.count(ws, want_fov=True)[1] for ch in chunks]).cpu().numpy().tolist()
    agree &= fov == want_fov

    # ---- device leg 2: from numpy frames, get_infos' count path
    t_up, up_reads = [], 0
    args = ([f["points"] for f in frames], [f["boxes"] for f in frames], [f["calib"] for f in frames], [f["image_shape"] for f in frames])
    for it in range(a.warmup + a.iters_upload):
        counter = InfoCounter(dev, per)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = counter.count(*args)
        torch.cuda.synchronize()
        if it >= a.warmup:
            t_up.append((time.perf_counter() - t0) * 1e3)
        up_reads = counter.reads
    agree &= np.concatenate(got).tolist() == want.tolist()

    # what the count call moves: every scene row once (the frame's boxes and calibration per workgroup go to LDS, not counted), a
    # count per box and block written and read again
    blk = kernels.kitti_infos_block_points()
    blocks = sum(a.boxes * len(frames[c0: c0 + per]) * max((max(len(f["points"]) for f in frames[c0: c0 + per]) + blk - 1) // blk, 1)
                 for c0 in range(0, a.frames, per))
    moved = n_points * 16 + 2 * blocks * 4
    call_ms = float(np.median(t_call))
    print(json.dumps({
        "bench": "kitti_infos", "frames": a.frames, "frames_per_call": per, "scene_points": int(n_points), "boxes_per_frame": a.boxes,
        "objects": a.frames * a.boxes, "points_in_view": int(sum(want_fov)), "points_counted": int(want.sum()),
        "host_ms_median": round(float(np.median(t_host)) * 1e3, 2), "host_threads": 1,
        "device_resident_ms_median": pct(t_all, 50), "device_resident_ms_p10": pct(t_all, 10), "device_resident_ms_p90": pct(t_all, 90),
        "device_resident_host_reads": reads, "count_calls_ms_median": pct(t_call, 50),
        "device_from_host_frames_ms_median": pct(t_up, 50), "device_from_host_frames_ms_p10": pct(t_up, 10),
        "device_from_host_frames_ms_p90": pct(t_up, 90), "device_from_host_frames_host_reads": up_reads,
        "upload_bytes": int(n_points * 16), "device_bytes_moved": int(moved),
        "bytes_per_s_over_the_count_calls": round(moved / (call_ms * 1e-3), 0),
        "share_of_hbm_peak": round(moved / (call_ms * 1e-3) / HBM_BYTES_PER_S, 4), "legs_agree": bool(agree)}))


if __name__ == "__main__":
    main()
