"""python -m hvpr_amd.demo: point-cloud files and a checkpoint in, detections and BEV pictures out.

The reference's tools/demo.py (`DemoDataset`: a `.bin` / `.npy` file or a folder of them, sorted) without mayavi: every frame
goes through `batch_loader.DeviceBatchLoader(training=False)`, the detector with `sync=False`, and `bev_vis.render_bev` -- the
points and the records stay on the device from the upload to the picture.  Per frame `<stem>.png` is written (unless
`--no_png`), and `result.pkl` gets one entry: `frame_id`, `name`, `score`, `boxes_lidar`, `pred_labels` (no camera fields:
there is no calibration).  The only reads of the device are the images and the records that are written, plus the loader's one
read per batch.

Flags of the reference: `--cfg_file --data_path --ckpt --ext`.  Added: `--output_dir --batch_size --score_thresh --pixel --no_png
--pipeline --seed`, and `--set` as the other commands have it.  There is no calibration, so the FOV filter is forced off (the
reference's DemoDataset never applies it either).  `--score_thresh` limits what is DRAWN; result.pkl holds every record.

`--pipeline` drives `detector.PipelinedForward`: batch 1 and a config that samples a fixed number of points only (the captured
graphs have a fixed input shape).  Each result is rendered and read before the next step on its lane; the records equal the
eager path's bit for bit."""
import argparse
import collections
import glob
import pickle
from pathlib import Path

import numpy as np
import torch

from .common_utils import create_logger
from .config import cfg_from_list, cfg_from_yaml_file
from .preprocess import to_device

REPO_ROOT = Path(__file__).resolve().parent.parent


def parse_config(argv=None):
    p = argparse.ArgumentParser(prog="python -m hvpr_amd.demo", description="detections and BEV pictures of point-cloud files")
    p.add_argument("--cfg_file", type=str, required=True, help="model config (yaml)")
    p.add_argument("--data_path", type=str, default="demo_data", help="a point-cloud file or a directory of them")
    p.add_argument("--ckpt", type=str, default=None, help="the trained model")
    p.add_argument("--ext", type=str, default=".bin", help="extension of the point-cloud files: .bin or .npy")
    p.add_argument("--output_dir", type=str, default=None, help="default: <repository>/output/demo")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--score_thresh", type=float, default=None, help="draw only predictions with at least this score")
    p.add_argument("--pixel", type=float, default=0.1, help="metres per pixel of the picture")
    p.add_argument("--no_png", action="store_true", default=False, help="write result.pkl only")
    p.add_argument("--pipeline", action="store_true", default=False, help="frame pipeline (detector.PipelinedForward), batch 1")
    p.add_argument("--seed", type=int, default=0, help="seed of the loader's generators (sample_points)")
    p.add_argument("--set", dest="set_cfgs", default=None, nargs=argparse.REMAINDER, help="KEY VALUE pairs over the config")
    args = p.parse_args(argv)
    if args.batch_size < 1:
        raise ValueError("--batch_size must be at least 1")
    if args.pipeline and args.batch_size != 1:
        raise ValueError("--pipeline runs at --batch_size 1")
    if not args.pixel > 0:
        raise ValueError("--pixel must be positive")
    cfg = cfg_from_yaml_file(args.cfg_file)
    cfg.TAG = Path(args.cfg_file).stem
    if args.set_cfgs:
        cfg_from_list(args.set_cfgs, cfg)
    return args, cfg


def list_files(data_path, ext):
    """DemoDataset's list (tools/demo.py:36-39): `*<ext>` of a directory, sorted as strings; a file stands for itself."""
    root = Path(data_path)
    files = glob.glob(str(root / f"*{ext}")) if root.is_dir() else [str(root)]
    files.sort()
    return files


def read_points(path, ext):
    """DemoDataset.__getitem__ (tools/demo.py:45-50): `.bin` is float32 in four columns, `.npy` an array; anything else raises."""
    if ext == ".bin":
        return np.fromfile(str(path), dtype=np.float32).reshape(-1, 4)
    if ext == ".npy":
        return np.ascontiguousarray(np.load(str(path)), dtype=np.float32)
    raise NotImplementedError(f"--ext {ext}: point clouds are read from .bin or .npy files")


class DemoFrames:
    """`frame_source` of DeviceBatchLoader over a list of files: the points go up through pinned memory as KittiDataset.frame's."""

    def __init__(self, files, ext, device="cuda:0"):
        if ext not in (".bin", ".npy"):
            raise NotImplementedError(f"--ext {ext}: point clouds are read from .bin or .npy files")
        self.files, self.ext, self.device = list(files), ext, torch.device(device)

    def __len__(self):
        return len(self.files)

    def __call__(self, index):
        return {"points": to_device(read_points(self.files[index], self.ext), self.device), "frame_id": Path(self.files[index]).stem,
                "file": self.files[index]}


def demo_data_config(cfg, logger=None):
    """The DATA_CONFIG block with the FOV filter off: there is no calibration to apply it with."""
    dc = dict(cfg.DATA_CONFIG)
    if dc.get("FOV_POINTS_ONLY", False):
        dc["FOV_POINTS_ONLY"] = False
        if logger is not None:
            logger.info("FOV_POINTS_ONLY is set in the config and forced off: point-cloud files carry no calibration")
    return dc


def build_loader(cfg, files, ext, device="cuda:0", logger=None):
    from .batch_loader import DeviceBatchLoader
    dc = demo_data_config(cfg, logger)
    frames = DemoFrames(files, ext, device)
    sample = any(p["NAME"] == "sample_points" for p in dc["DATA_PROCESSOR"])
    return DeviceBatchLoader(dc, cfg.CLASS_NAMES, frames, len(frames), training=False, device=device, sample_points=sample)


def batch_indices(n, batch_size):
    return [list(range(i, min(i + batch_size, n))) for i in range(0, n, batch_size)]


def prepare(loader, indices, seed):
    """One batch; its generator depends on the seed and the batch's first frame only.  A frame the loader refuses raises, naming
    the files of the batch."""
    try:
        return loader.prepare_batch(indices, np.random.RandomState([int(seed), int(indices[0])]))
    except ValueError as e:
        names = ", ".join(loader.frame_source.files[i] for i in indices)
        raise ValueError(f"{names}: the loader refuses the frame ({e})") from e


def record_entry(rec, frame_id, class_names):
    """The result.pkl entry of one frame from its record on the host (the first pred_count rows count)."""
    n = int(rec["pred_count"].reshape(-1)[0]) if "pred_count" in rec else len(rec["pred_scores"])
    labels = np.asarray(rec["pred_labels"])[:n].astype(np.int64)
    return {"frame_id": frame_id, "name": np.array(class_names)[labels - 1] if n else np.zeros((0,), dtype="<U1"),
            "score": np.asarray(rec["pred_scores"])[:n], "boxes_lidar": np.asarray(rec["pred_boxes"])[:n], "pred_labels": labels}


_REC_KEYS = ("pred_boxes", "pred_scores", "pred_labels", "pred_count")


def _to_host(records):
    return [{k: r[k].cpu().numpy() for k in _REC_KEYS} for r in records]


def run(args, cfg, logger, device="cuda:0"):
    """Returns the list written to result.pkl."""
    from . import bev_vis
    from .detector import PipelinedForward, SyntheticDataset, build_network
    if args.ckpt is None:
        raise SystemExit("demo: give --ckpt")
    files = list_files(args.data_path, args.ext)
    if not files:
        raise FileNotFoundError(f"no *{args.ext} file under {args.data_path}")
    out_dir = Path(args.output_dir) if args.output_dir is not None else REPO_ROOT / "output" / "demo"
    out_dir.mkdir(parents=True, exist_ok=True)
    loader = build_loader(cfg, files, args.ext, device, logger)
    logger.info(f"Total number of samples: \t{len(files)}")
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDataset(cfg))
    model.load_params_from_file(filename=args.ckpt, logger=logger, to_cpu=True)
    model = model.to(device).eval()
    renderer = bev_vis.BevRenderer(cfg.DATA_CONFIG["POINT_CLOUD_RANGE"], len(cfg.CLASS_NAMES), pixel=args.pixel,
                                   score_thresh=args.score_thresh, device=device)
    class_names, entries = list(cfg.CLASS_NAMES), []

    def finish(batch, records):
        """Renders, then reads what is written: the images and the records."""
        images = None if args.no_png else renderer(batch, records).cpu().numpy()
        for b, rec in enumerate(_to_host(records)):
            stem = batch["frame_id"][b]
            if images is not None:
                bev_vis.write_png(out_dir / f"{stem}.png", images[b])
            entries.append(record_entry(rec, stem, class_names))
            logger.info(f"{stem}: {len(entries[-1]['score'])} boxes")

    todo = batch_indices(len(files), args.batch_size)
    with torch.no_grad():
        if not args.pipeline:
            for indices in todo:
                batch = prepare(loader, indices, args.seed)
                records, _, _ = model(batch, sync=False)
                finish(batch, records)
        else:
            if loader.num_points is None:
                raise ValueError("--pipeline needs a config whose DATA_PROCESSOR samples a fixed number of points (sample_points)")
            waiting, pipe = collections.deque(), None
            for indices in todo:
                batch = prepare(loader, indices, args.seed)
                if pipe is None:
                    pipe = PipelinedForward(model, {k: v for k, v in batch.items() if torch.is_tensor(v) or k == "batch_size"})
                waiting.append(batch)
                records = pipe(batch)
                if records is not None:
                    finish(waiting.popleft(), records)
            for records in pipe.flush():
                if waiting:
                    finish(waiting.popleft(), records)
            pipe.check_status()
            assert not waiting
    with open(out_dir / "result.pkl", "wb") as f:
        pickle.dump(entries, f)
    logger.info(f"Demo done: {len(entries)} frames, results in {out_dir}")
    return entries


def main(argv=None):
    args, cfg = parse_config(argv)
    logger = create_logger(name="hvpr_amd.demo")
    logger.info("-----------------Quick Demo of hvpr_amd-------------------------")
    return run(args, cfg, logger)


if __name__ == "__main__":
    main()
