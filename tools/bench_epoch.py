"""The epoch loop at batch 16: what a training iteration costs (a) as `optim.train_step` on a resident batch, (b) in
`train_loop.train_one_epoch` with the batch prepared on the step's own stream (`--no_prefetch`), (c) in the same loop with
`EpochLoader(prefetch=True)`: the batch prepared one step ahead on the loader's stream.

Data: 64 synthetic frames (synthetic.kitti_like_frame at ~123 k points, 8 Car boxes each, one KITTI calibration: the shape of
tools/bench_batch_loader.py), held in memory behind the `frame(index)` interface of kitti_dataset.KittiDataset; bank and augmentor
as tools/bench_augment.py (DATA_AUGMENTOR_3CLASS without the road plane); hvpr_car's DATA_PROCESSOR (sample_points 16384).  Model:
hvpr_car, the flat optimiser.  An epoch is 4 iterations.

Per leg: ms per iteration (wall around whole epochs, ending in a synchronise), host ms per iteration (wall until the last enqueue
returns, before that synchronise) and synchronising calls per iteration under torch's sync-debug "warn".  (b) and (c) are run
--runs times in alternation; `prefetch_wins` says whether every (c) run is below every (b) run, i.e. the difference is larger than
the spread of the runs.

    python tools/bench_epoch.py [--batch 16] [--frames 64] [--epochs 3] [--runs 3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_augment import SIZES, synthetic_bank  # noqa: E402
from bench_batch_loader import CALIB, SHAPE  # noqa: E402
from hvpr_amd import optim, synthetic, train_loop  # noqa: E402
from hvpr_amd.batch_loader import DeviceBatchLoader  # noqa: E402
from hvpr_amd.config import CFG_DIR, cfg_from_yaml_file, hvpr_car_cfg  # noqa: E402
from hvpr_amd.detector import SyntheticDataset, build_network  # noqa: E402
from hvpr_amd.epoch_loader import EpochLoader, EpochSampler  # noqa: E402


def counted(fn):
    """(wall ms to the last enqueue, wall ms to the end of the device work, synchronising calls) of fn()."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    return host, wall, sum("synchroniz" in str(x.message).lower() and "prototype" not in str(x.message) for x in w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=3, help="epochs per timed run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--bank-scale", type=float, default=0.1)
    ap.add_argument("--n-az", type=int, default=1900)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch: needs the GPU (there is no CPU path to time)")
    rng = np.random.RandomState(7)
    cfg = hvpr_car_cfg()
    data_cfg = cfg.DATA_CONFIG
    data_cfg["DATA_AUGMENTOR"] = cfg_from_yaml_file(os.path.join(CFG_DIR, "dataset_configs", "kitti_augmentor.yaml"))["DATA_AUGMENTOR_3CLASS"]
    data_cfg["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0]["USE_ROAD_PLANE"] = False
    classes = list(cfg.CLASS_NAMES)
    bank = synthetic_bank(a.bank_scale, rng)
    bank.on_device()
    frames = []
    for b in range(a.frames):
        g = np.zeros((8, 7), np.float32)
        g[:, 0], g[:, 1], g[:, 2] = rng.uniform(3, 45, 8), rng.uniform(-18, 18, 8), rng.uniform(-1.2, -0.8, 8)
        g[:, 3:6], g[:, 6] = SIZES["Car"], rng.uniform(-np.pi, np.pi, 8)
        frames.append({"points": torch.from_numpy(synthetic.kitti_like_frame(100 + b, n_az=a.n_az)).cuda(), "gt_boxes": g,
                       "gt_names": np.array(["Car"] * 8), "calib": CALIB, "image_shape": SHAPE, "frame_id": "%06d" % b})
    points_per_frame = int(np.mean([f["points"].shape[0] for f in frames]))

    def loader_of(prefetch):
        bl = DeviceBatchLoader(data_cfg, classes, lambda i: frames[i], len(frames), bank=bank, training=True, sample_points=True)
        return EpochLoader(None, bl, EpochSampler(len(frames), a.batch, True, seed=0), seed=0, prefetch=prefetch)

    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(classes), SyntheticDataset(cfg, training=True)).cuda()
    opt = optim.build_optimizer(model, cfg.OPTIMIZATION)
    iters_per_epoch = len(loader_of(False))
    sched, _ = optim.build_scheduler(opt, iters_per_epoch, 1000, -1, cfg.OPTIMIZATION)
    fn = optim.model_fn_decorator()
    clip = cfg.OPTIMIZATION.GRAD_NORM_CLIP
    state = {"it": 0, "epoch": 0}

    def epochs(loader, n):
        for _ in range(n):
            loader.sampler.set_epoch(state["epoch"])
            state["epoch"] += 1
            state["it"], _ = train_loop.train_one_epoch(model, opt, loader, fn, sched, state["it"], cfg.OPTIMIZATION)

    loaders = {False: loader_of(False), True: loader_of(True)}
    epochs(loaders[False], 1)                                    # lazy initialisation of everything
    epochs(loaders[True], 1)
    n = a.epochs * iters_per_epoch

    # (a) the step alone, on a batch that stays where it is
    resident = loaders[False].batch_loader.prepare_batch(list(range(a.batch)), np.random.RandomState(1))

    def steps():
        for _ in range(n):
            optim.train_step(model, opt, sched, dict(resident), state["it"], clip)
            state["it"] += 1
    steps()
    host, wall, syncs = counted(steps)
    line = {"bench": "epoch", "batch": a.batch, "frames": a.frames, "points_per_frame": points_per_frame, "iters_per_run": n,
            "train_step": {"ms_per_iter": round(wall / n, 3), "host_ms_per_iter": round(host / n, 3), "sync_calls_per_iter": syncs / n}}
    runs = {False: [], True: []}
    for _ in range(a.runs):
        for prefetch in (False, True):
            host, wall, syncs = counted(lambda: epochs(loaders[prefetch], a.epochs))
            runs[prefetch].append({"ms_per_iter": round(wall / n, 3), "host_ms_per_iter": round(host / n, 3), "sync_calls_per_iter": syncs / n})
    line["loop_no_prefetch"], line["loop_prefetch"] = runs[False], runs[True]
    line["prefetch_wins"] = max(r["ms_per_iter"] for r in runs[True]) < min(r["ms_per_iter"] for r in runs[False])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
