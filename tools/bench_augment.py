"""Training augmentation at batch 16: the device form (hvpr_amd/augment.py, csrc/augment.hip) against the same pipeline in
numpy over the CPU natives (libhvpr_cpu.so), which is what the reference's per-frame Python costs.

Scenes: synthetic.kitti_like_frame.  Bank: synthetic, sized like KITTI's train database after its filters (Car 14357,
Pedestrian 2207, Cyclist 734 objects; points per object log-uniform in 5..600 for cars, 5..300 otherwise; --bank-scale shrinks
it).  Config: DATA_AUGMENTOR_3CLASS of cfgs/dataset_configs/kitti_augmentor.yaml (Car:15, Pedestrian:10, Cyclist:10), without
the road plane (the synthetic frames carry none).  ONE set of plans goes to both legs.

  device leg   all launches of one call (collision, boxes, points), HIP events, warm-up, median of 30; the plan upload and the
               final read are timed separately, wall clock.
  host leg     tests/augment_cases.augment_frame with boxes_bev_iou_cpu / points_in_boxes_cpu, one thread, wall clock, per batch.

    python tools/bench_augment.py [--batch 16] [--bank-scale 1.0]
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
import augment_cases as AC  # noqa: E402
from hvpr_amd import gt_sampling, kernels, synthetic  # noqa: E402
from hvpr_amd.augment import DeviceAugmentor, ObjectBank, pack_plans, plan_words  # noqa: E402
from hvpr_amd.config import cfg_from_yaml_file  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]
SIZES = {"Car": [3.9, 1.6, 1.56], "Pedestrian": [0.8, 0.6, 1.73], "Cyclist": [1.76, 0.6, 1.73]}
KITTI_DB = {"Car": (14357, 600), "Pedestrian": (2207, 300), "Cyclist": (734, 300)}
RANGE = [0, -40, -3, 70.4, 40, 1]


def synthetic_bank(scale, rng):
    names, boxes, pts = [], [], []
    for c in CLASSES:
        n, top = KITTI_DB[c]
        for _ in range(max(20, int(n * scale))):
            size = np.array(SIZES[c], np.float32) * rng.uniform(0.9, 1.1, 3).astype(np.float32)
            k = int(np.exp(rng.uniform(np.log(5), np.log(top))))
            names.append(c)
            boxes.append(np.concatenate([[rng.uniform(3, 68), rng.uniform(-38, 38), rng.uniform(-1.2, -0.6)], size, [rng.uniform(-np.pi, np.pi)]]))
            pts.append(np.concatenate([rng.uniform(-0.5, 0.5, (k, 3)) * size, rng.uniform(0, 1, (k, 1))], axis=1).astype(np.float32))
    return ObjectBank.from_arrays(names, np.asarray(boxes, np.float32), pts, CLASSES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--bank-scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.RandomState(7)
    cfg = cfg_from_yaml_file(os.path.join(ROOT, "hvpr_amd", "cfgs", "dataset_configs", "kitti_augmentor.yaml"))["DATA_AUGMENTOR_3CLASS"]
    cfg["AUG_CONFIG_LIST"][0]["USE_ROAD_PLANE"] = False
    bank = synthetic_bank(a.bank_scale, rng)
    arena, obj_off = bank.host_points()
    aug = DeviceAugmentor(cfg, CLASSES, bank, RANGE)
    scenes = [synthetic.kitti_like_frame(100 + b) for b in range(a.batch)]
    frames = []
    for b, s in enumerate(scenes):
        g = np.zeros((8, 7), np.float32)
        g[:, 0], g[:, 1], g[:, 2] = rng.uniform(3, 60, 8), rng.uniform(-30, 30, 8), rng.uniform(-1.2, -0.8, 8)
        g[:, 3:6], g[:, 6] = SIZES["Car"], rng.uniform(-np.pi, np.pi, 8)
        frames.append({"points": torch.from_numpy(s).cuda(), "gt_boxes": g, "gt_names": np.array(["Car"] * 8)})
    plans = [aug.planner.plan_frame(f["gt_names"], rng=rng) for f in frames]
    gt_cls = [np.ones((8,), np.int32)] * a.batch
    counts = [len(s) for s in scenes]
    B, NG, G, C = a.batch, aug.planner.num_groups, 8 * a.batch, sum(len(p["cand_obj"]) for p in plans)
    stage = torch.empty((plan_words(B, NG, G, C),), dtype=torch.int32).pin_memory()
    words = pack_plans(stage.numpy(), plans, [f["gt_boxes"] for f in frames], gt_cls, counts, aug.planner.ops_word, NG, obj_off)
    points = torch.cat([f["points"] for f in frames]).contiguous()
    bank.on_device()
    g_cap = 8 + max(len(p["cand_obj"]) for p in plans)

    def device_call(dev):
        return kernels.augment_batch(stage, dev, words, points, bank, aug.planner.extra_width, aug.point_cloud_range, True, g_cap)

    dev = stage.to("cuda", non_blocking=True)
    for _ in range(a.warmup):
        out = device_call(dev)
    torch.cuda.synchronize()
    t_dev, t_up, t_read = [], [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        dev = stage.to("cuda", non_blocking=True)
        torch.cuda.synchronize()
        t_up.append(time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = device_call(dev)
        e1.record()
        torch.cuda.synchronize()
        t_dev.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        cnt = out["counts"].cpu().numpy()                                           # the one read
        t_read.append(time.perf_counter() - t0)
    n_out = int(cnt[B])
    valid = out["valid"].cpu().numpy().astype(bool)

    iou = gt_sampling.boxes_bev_iou_cpu
    inside = lambda p, b: gt_sampling.points_in_boxes_cpu(p, b) if len(b) else np.zeros((0, len(p)), np.int32)
    torch.set_num_threads(1)
    t_host, agree = [], True
    for it in range(3):
        t0 = time.perf_counter()
        for f in range(B):
            r = AC.augment_frame(scenes[f], frames[f]["gt_boxes"], gt_cls[f], plans[f], aug.planner.ops, arena, obj_off, bank.obj_box,
                                 aug.planner.extra_width, RANGE, True, np.float32,
                                 iou=lambda x, y: iou(x, y) if len(y) else np.zeros((len(x), 0), np.float32), inside=inside)
            if it == 0:
                c0 = sum(len(p["cand_obj"]) for p in plans[:f])
                agree &= r["valid"].tolist() == valid[c0: c0 + len(plans[f]["cand_obj"])].tolist() and len(r["points"]) == cnt[f + 1] - cnt[f]
        t_host.append(time.perf_counter() - t0)
    F = points.shape[1]
    starts = np.cumsum([0] + [len(p["cand_obj"]) for p in plans])
    pasted = sum(int(obj_off[o + 1] - obj_off[o]) for p, c0 in zip(plans, starts) for k, o in enumerate(p["cand_obj"]) if valid[c0 + k])
    # count pass: scene rows read, a flag byte written; write pass: flags and kept rows read, output rows written; pasted rows read
    moved = points.numel() * 4 + points.shape[0] + points.shape[0] + (n_out - pasted) * F * 4 + pasted * F * 4 + n_out * F * 4 + words * 4
    print(json.dumps({
        "bench": "augment", "batch": B, "scene_points": int(points.shape[0]), "bank_objects": len(bank), "bank_points": int(arena.shape[0]),
        "candidates": C, "accepted": int(valid.sum()), "points_out": n_out,
        "device_ms_median": round(float(np.median(t_dev)), 4), "device_ms_min": round(float(np.min(t_dev)), 4),
        "plan_upload_ms_median": round(float(np.median(t_up)) * 1e3, 4), "final_read_ms_median": round(float(np.median(t_read)) * 1e3, 4),
        "host_ms_per_batch_median": round(float(np.median(t_host)) * 1e3, 2), "host_threads": 1,
        "device_bytes_moved": int(moved), "plan_bytes": int(words * 4), "legs_agree": bool(agree)}))


if __name__ == "__main__":
    main()
