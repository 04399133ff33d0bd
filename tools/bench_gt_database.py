"""The GT-sampling database from raw frames: the device form (hvpr_amd/gt_database.py, csrc/gt_database.hip) against the same
loop in numpy over the CPU native points_in_boxes_cpu (tests/gt_database_cases.host_database), which is what the reference's
create_groundtruth_database costs once its absent native is supplied.

Scenes: synthetic.kitti_like_frame at about 120 k points, 64 frames, 8 boxes each, set down on points of the frame; every point
within 1e-3 m of a box face is removed first (the margin rule of the tests), so both legs select the same points and their
arenas are compared byte for byte.

  host leg       host_database, one thread, wall clock, files kept in memory (no disk).
  device leg 1   frames already resident: per chunk the count call, the ONE host read, the extract call; HIP events around the
                 whole and around each call, warm-up, median of --iters with p10-p90.
  device leg 2   DatabaseBuilder.add_frames from numpy frames: packing into the pinned buffer, the upload, the calls, the growing
                 arena; wall clock ending in a synchronise, median of --iters-upload.
  file writing   DatabaseBuilder.write into a temporary directory (one device-to-host copy, then the files), wall clock, reported
                 on its own and part of neither leg.

    python tools/bench_gt_database.py [--frames 64] [--n-az 2048] [--boxes 8] [--frames-per-call 32]
Prints ONE JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gt_database_cases as GC  # noqa: E402
from hvpr_amd import kernels, synthetic  # noqa: E402
from hvpr_amd.gt_database import DatabaseBuilder, StagedChunk  # noqa: E402

HBM_BYTES_PER_S = 8.0e12           # MI355X peak


def scene(n_frames, n_az, n_boxes, rng):
    infos, clouds = [], {}
    for f in range(n_frames):
        pts = synthetic.kitti_like_frame(1000 + f, n_az=n_az)
        names = [["Car", "Pedestrian", "Cyclist", "Van"][i % 4] for i in range(n_boxes)]
        at = pts[rng.choice(len(pts), n_boxes, replace=False), :3].astype(np.float64)
        boxes = np.zeros((n_boxes, 7))
        for i, n in enumerate(names):
            size = np.asarray(GC.SIZES[n]) * rng.uniform(0.9, 1.1)
            boxes[i] = [at[i, 0] + rng.uniform(-0.3, 0.3), at[i, 1] + rng.uniform(-0.3, 0.3), at[i, 2] + size[2] / 2 - 0.1, *size,
                        rng.uniform(-np.pi, np.pi)]
        idx = "%06d" % f
        kept = GC.clean_points(pts, boxes)
        assert len(kept) >= 0.99 * len(pts)
        infos.append(GC.make_info(idx, names, boxes, seed=f))
        clouds[idx] = np.ascontiguousarray(kept)
    return infos, clouds


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
        raise SystemExit("bench_gt_database: needs the GPU (nothing here is measured without one)")
    rng = np.random.RandomState(21)
    infos, clouds = scene(a.frames, a.n_az, a.boxes, rng)
    get = lambda idx: clouds[idx]
    n_points = sum(len(c) for c in clouds.values())
    F = 4

    # ---- host leg
    torch.set_num_threads(1)
    t_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        _, _, objects = GC.host_database(infos, get)
        t_host.append(time.perf_counter() - t0)
    want = np.concatenate(objects)

    # ---- device leg 1: resident frames
    dev = torch.device("cuda:0")
    chunks = []
    for c0 in range(0, a.frames, a.frames_per_call):
        part = infos[c0: c0 + a.frames_per_call]
        pts = [torch.from_numpy(clouds[i["point_cloud"]["lidar_idx"]]).to(dev) for i in part]
        chunks.append(StagedChunk(pts, [i["annos"]["gt_boxes_lidar"] for i in part], dev, centres=True))  # a staging buffer each: they stay
    arena = torch.empty((len(want) + 16, F), dtype=torch.float32, device=dev)
    count_host = torch.empty((a.frames * a.boxes,), dtype=torch.int32).pin_memory()
    ws = None
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_all, t_count, t_extract = [], [], []
    for it in range(a.warmup + a.iters):
        e = [ev() for _ in range(2 + 4 * len(chunks))]
        rows, k = 0, 0
        e[0].record()
        for j, ch in enumerate(chunks):
            e[2 + 4 * j].record()
            cnt, _, ws = ch.count(ws)
            e[3 + 4 * j].record()
            ch_host = count_host[k: k + ch.n_obj]
            ch_host.copy_(cnt)                                                # the one read of the chunk
            n = int(ch_host.numpy().sum())
            e[4 + 4 * j].record()
            kernels.gt_database_extract(ch.points, ch.pt_off_host, ch.pt_off, ch.boxes, ch.box_off_host, ch.box_off, ch.centres,
                                        ch_host, cnt, arena[rows:], ws)
            e[5 + 4 * j].record()
            rows, k = rows + n, k + ch.n_obj
        e[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            t_all.append(e[0].elapsed_time(e[1]))
            t_count.append(sum(e[2 + 4 * j].elapsed_time(e[3 + 4 * j]) for j in range(len(chunks))))
            t_extract.append(sum(e[4 + 4 * j].elapsed_time(e[5 + 4 * j]) for j in range(len(chunks))))
    agree = rows == len(want) and arena[:rows].cpu().numpy().tobytes() == want.tobytes()

    # ---- device leg 2: from numpy frames, through the builder
    t_up = []
    for it in range(a.warmup + a.iters_upload):
        b = DatabaseBuilder(frames_per_call=a.frames_per_call, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.add_frames(infos, get)
        torch.cuda.synchronize()
        if it >= a.warmup:
            t_up.append((time.perf_counter() - t0) * 1e3)
    agree &= b.arena().cpu().numpy().tobytes() == want.tobytes()

    # ---- file writing, on its own
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        b.write(tmp)
        t_write = (time.perf_counter() - t0) * 1e3

    # what the two passes move: each reads every scene row once and the frame's boxes per workgroup (LDS, not counted); the count
    # pass writes a count per box and block, the scans read and write those, the write pass reads them and writes the arena rows
    blk = kernels.gt_database_block_points()
    blocks = sum(a.boxes * max(max((len(clouds[i["point_cloud"]["lidar_idx"]]) + blk - 1) // blk for i in infos[c0: c0 + a.frames_per_call]), 1)
                 * len(infos[c0: c0 + a.frames_per_call]) for c0 in range(0, a.frames, a.frames_per_call))
    moved = 2 * n_points * F * 4 + 5 * blocks * 4 + len(want) * F * 4
    kernel_ms = float(np.median(t_count)) + float(np.median(t_extract))
    print(json.dumps({
        "bench": "gt_database", "frames": a.frames, "frames_per_call": a.frames_per_call, "scene_points": int(n_points),
        "boxes_per_frame": a.boxes, "objects": a.frames * a.boxes, "arena_rows": int(len(want)),
        "host_ms_median": round(float(np.median(t_host)) * 1e3, 2), "host_threads": 1,
        "device_resident_ms_median": pct(t_all, 50), "device_resident_ms_p10": pct(t_all, 10), "device_resident_ms_p90": pct(t_all, 90),
        "count_calls_ms_median": pct(t_count, 50), "extract_calls_ms_median": pct(t_extract, 50),
        "device_with_upload_ms_median": pct(t_up, 50), "device_with_upload_ms_p10": pct(t_up, 10), "device_with_upload_ms_p90": pct(t_up, 90),
        "upload_bytes": int(n_points * F * 4), "file_write_ms": round(t_write, 2),
        "device_bytes_moved": int(moved), "bytes_per_s_over_the_two_calls": round(moved / (kernel_ms * 1e-3), 0),
        "share_of_hbm_peak": round(moved / (kernel_ms * 1e-3) / HBM_BYTES_PER_S, 4),
        "box_tests_per_point_per_pass": a.boxes, "box_tests": int(2 * n_points * a.boxes), "legs_agree": bool(agree)}))


if __name__ == "__main__":
    main()
