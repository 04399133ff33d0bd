"""The evaluation epilogue of one batch, host leg against device leg, both from the SAME post_processing(sync=False) records.

A batch of --batch synthetic frames goes through the 3-class detector once (NMS_POST_MAXSIZE 500); every frame gets ten ground truths
made from its own detections.  Then, per repetition and alternating:

  host    what post_processing(sync=True) does with those records (one read of the counts, the records sliced on the host,
          Detector3DTemplate.generate_recall_record per frame) and kitti_eval.generate_prediction_dicts
  device  eval_loop.DeviceEvalEpilogue.add_batch

HIP events around each leg plus wall time (`wall_us`: until the call returns; `wall_sync_us`: until the device has finished too).
After a warm-up the median of --reps repetitions with the 10th and 90th percentile, and the synchronising calls (Tensor.cpu / item /
tolist) each leg made per batch.  One JSON line.

    python tools/bench_eval_tail.py [--batch 16] [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvpr_amd import detector, eval_loop, kitti_eval, synthetic, synthetic_weights  # noqa: E402
from hvpr_amd.config import hvpr_3class_cfg  # noqa: E402

DEV = torch.device("cuda", 0)
CALIB = {
    "P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
    "R0": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
                    [0.007402527, 0.004351614, 0.9999631]], np.float32),
    "Tr_velo2cam": np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                             [0.9998621, 0.007523790, 0.01480755, -0.2717806]], np.float32),
}


def percentiles(v, scale):
    a = np.sort(np.asarray(v)) * scale
    return {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(np.percentile(a, 10)), 1), "p90_us": round(float(np.percentile(a, 90)), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    B = args.batch
    cfg = hvpr_3class_cfg()
    pp = cfg.MODEL.POST_PROCESSING
    thr, post, cls = list(pp.RECALL_THRESH_LIST), int(pp.NMS_CONFIG.NMS_POST_MAXSIZE), list(cfg.CLASS_NAMES)
    model = detector.build_network(cfg.MODEL, len(cls), detector.SyntheticDataset(cfg))
    synthetic_weights.load_synthetic(model, seed=5, cls_bias=-2.0)
    model = model.to(DEV).eval()
    frames = [synthetic.hvpr_frame(400 + b) for b in range(B)]
    pts = np.concatenate([np.concatenate([np.full((len(f), 1), b, np.float32), f], 1) for b, f in enumerate(frames)])
    host_keys = {"frame_id": ["%06d" % b for b in range(B)], "calib": [CALIB] * B, "image_shape": np.array([[375, 1242]] * B)}
    with torch.no_grad():
        preds, _, bd = model({"points": torch.from_numpy(pts).to(DEV), "batch_size": B, **host_keys})
    bd.update(host_keys)
    gt = np.zeros((B, 12, 8), np.float32)
    for b in range(B):
        pb, pl = preds[b]["pred_boxes"].cpu().numpy()[:10], preds[b]["pred_labels"].cpu().numpy()[:10]
        gt[b, :len(pb), :7], gt[b, :len(pb), 7] = pb, pl
        gt[b, :len(pb), 0] += np.linspace(0.0, 0.9, len(pb))
    bd["gt_boxes"] = torch.from_numpy(gt).to(DEV)
    with torch.no_grad():
        recs = model.post_processing(bd, sync=False)[0]
    ep = eval_loop.DeviceEvalEpilogue(cls, thr, B * (args.warmup + args.reps), post)
    out_host = {}

    def host():
        ns = torch.cat([r["pred_count"] for r in recs]).tolist()                      # detector.py: the chunk's counts, read once
        sliced, recall = [], {}
        for b, r in enumerate(recs):
            rec = {k: (v[:ns[b]] if k != "pred_count" else v) for k, v in r.items()}
            recall = detector.Detector3DTemplate.generate_recall_record(rec["pred_boxes"], recall, b, bd, thr)
            sliced.append(rec)
        out_host["recall"], out_host["annos"] = recall, kitti_eval.generate_prediction_dicts(bd, sliced, cls)

    def device():
        ep.add_batch(bd, recs)
    legs = {"host": host, "device": device}
    syncs = {k: 0 for k in legs}
    real = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist")}
    ev, wall, wall_sync = ({k: [] for k in legs} for _ in range(3))
    for rep in range(args.warmup + args.reps):
        for name, fn in legs.items():
            count = rep == args.warmup                                                  # the synchronising calls of one batch
            if count:
                for n, f in real.items():
                    setattr(torch.Tensor, n, (lambda f: lambda self, *a, **k: (syncs.__setitem__(name, syncs[name] + 1), f(self, *a, **k))[1])(f))
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            t2 = time.perf_counter()
            if count:
                for n, f in real.items():
                    setattr(torch.Tensor, n, f)
            if rep >= args.warmup:
                ev[name].append(e0.elapsed_time(e1)); wall[name].append(t1 - t0); wall_sync[name].append(t2 - t0)
    want = out_host["recall"]
    got = ep.recall_dict()
    n = args.warmup + args.reps
    assert all(got[k] == n * v for k, v in want.items()), (got, want)                    # the two legs counted the same
    out = {"batch": B, "post_max": post, "reps": args.reps, "detections_per_frame": round(float(np.mean([len(a["name"]) for a in out_host["annos"]])), 1),
           "gt_per_frame": int(want["gt"] / B), "sync_calls_per_batch": syncs}
    for name in legs:
        out[name] = {"events": percentiles(ev[name], 1e3), "wall_us": percentiles(wall[name], 1e6)["median_us"],
                     "wall_sync_us": percentiles(wall_sync[name], 1e6)["median_us"]}
    out["device_over_host_wall_sync"] = round(out["device"]["wall_sync_us"] / out["host"]["wall_sync_us"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
