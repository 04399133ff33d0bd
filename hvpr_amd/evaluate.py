"""python -m hvpr_amd.evaluate: a KITTI folder and a checkpoint (or a folder of them) in, the AP table out.

The reference's tools/test.py over this package's own pieces: `epoch_loader.build_dataloader(training=False)`,
`detector.build_network`, `eval_loop.eval_one_epoch_device`.  Flags keep the reference's names; `--data_path`, `--output_dir`,
`--seed`, `--log_interval` and `--no_prefetch` are added.  Output goes to <output_dir>/<cfg stem>/<extra_tag>/eval/...: one
checkpoint under epoch_<id>/<split>/<eval_tag>/, `--eval_all` under eval_all_default/<eval_tag>/epoch_<id>/<split>/, each with
result.pkl, metrics.json (the returned dict) and, with --save_to_file, the txt files.

Evaluation runs on ONE rank: with `--launcher pytorch` rank 0 evaluates and the others wait at a barrier (sharded evaluation and
the merge of its results are not built).  `--launcher slurm` and `--merge_all_iters_to_one_epoch` are not built; `--workers` is
accepted and ignored (batches are prepared on the device, there are no worker processes)."""
import argparse
import copy
import datetime
import glob
import json
import os
import re
import time
from pathlib import Path

import torch

from . import distributed
from .common_utils import create_logger
from .config import _get, cfg_from_list, cfg_from_yaml_file

REPO_ROOT = Path(__file__).resolve().parent.parent


def common_arguments(parser):
    parser.add_argument("--cfg_file", type=str, required=True, help="model config (yaml)")
    parser.add_argument("--batch_size", type=int, default=None, help="total batch size (default: OPTIMIZATION.BATCH_SIZE_PER_GPU per rank)")
    parser.add_argument("--workers", type=int, default=4, help="accepted and ignored")
    parser.add_argument("--extra_tag", type=str, default="default")
    parser.add_argument("--ckpt", type=str, default=None)
    parser.add_argument("--launcher", choices=["none", "pytorch", "slurm"], default="none")
    parser.add_argument("--tcp_port", type=int, default=18888, help="accepted and ignored (the rendezvous comes from the environment)")
    parser.add_argument("--local_rank", type=int, default=0)
    parser.add_argument("--max_waiting_mins", type=int, default=0)
    parser.add_argument("--start_epoch", type=int, default=0)
    parser.add_argument("--save_to_file", action="store_true", default=False)
    parser.add_argument("--eval_tag", type=str, default="default")
    parser.add_argument("--eval_all", action="store_true", default=False)
    parser.add_argument("--ckpt_dir", type=str, default=None)
    parser.add_argument("--data_path", type=str, default=None, help="the KITTI directory (default: DATA_CONFIG.DATA_PATH)")
    parser.add_argument("--output_dir", type=str, default=None, help="default: <repository>/output")
    parser.add_argument("--seed", type=int, default=0, help="seed of the epoch sampler and of the loader's generators")
    parser.add_argument("--log_interval", type=int, default=50, help="iterations between two reads of the logged scalars")
    parser.add_argument("--no_prefetch", action="store_true", default=False, help="prepare each batch on the step's own stream")
    parser.add_argument("--set", dest="set_cfgs", default=None, nargs=argparse.REMAINDER, help="KEY VALUE pairs over the config")


def finish_config(args):
    """The config of args.cfg_file with --set applied, TAG set; refuses what is not built."""
    if args.launcher == "slurm":
        raise NotImplementedError("--launcher slurm is not built: use --launcher pytorch under torch.distributed.run")
    if getattr(args, "merge_all_iters_to_one_epoch", False):
        raise NotImplementedError("--merge_all_iters_to_one_epoch is not built")
    cfg = cfg_from_yaml_file(args.cfg_file)
    cfg.TAG = Path(args.cfg_file).stem
    cfg.LOCAL_RANK = 0
    if args.set_cfgs:
        cfg_from_list(args.set_cfgs, cfg)
    return cfg


def parse_config(argv=None):
    parser = argparse.ArgumentParser(prog="python -m hvpr_amd.evaluate", description="evaluate checkpoints on the KITTI val split")
    common_arguments(parser)
    args = parser.parse_args(argv)
    return args, finish_config(args)


def output_dir_of(args, cfg):
    """<output_dir>/<cfg stem>/<extra_tag>"""
    base = Path(args.output_dir) if args.output_dir is not None else REPO_ROOT / "output"
    return base / cfg.TAG / args.extra_tag


def eval_dir_of(args, cfg, output_dir):
    """(directory, epoch id) of `evaluate`'s results (tools/test.py:151-164)."""
    d = output_dir / "eval"
    epoch_id = None
    if not args.eval_all:
        nums = re.findall(r"\d+", args.ckpt) if args.ckpt is not None else []
        epoch_id = nums[-1] if nums else "no_number"
        d = d / ("epoch_%s" % epoch_id) / test_split(cfg)
    else:
        d = d / "eval_all_default"
    if args.eval_tag is not None:
        d = d / args.eval_tag
    return d, epoch_id


def test_split(cfg):
    from .kitti_dataset import DEFAULT_SPLIT
    return _get(cfg.DATA_CONFIG, "DATA_SPLIT", DEFAULT_SPLIT)["test"]


def init_launcher(args, cfg):
    """(distributed?, rank, world, device)."""
    if args.launcher == "none":
        return False, 0, 1, torch.device("cuda:0")
    _, local_rank, _ = distributed.env_rank()
    device = torch.device("cuda:%d" % local_rank)
    torch.cuda.set_device(device)
    rank, local_rank, world = distributed.init(device=device)
    cfg.LOCAL_RANK = local_rank
    return world > 1, rank, world, device


def per_rank_batch_size(args, cfg, world):
    if args.batch_size is None:
        return int(cfg.OPTIMIZATION.BATCH_SIZE_PER_GPU)
    if args.batch_size % world != 0:
        raise ValueError("--batch_size must be a multiple of the number of ranks")
    return args.batch_size // world


def gt_annos_of(dataset):
    """The split's ground-truth annotations in frame order (kitti_dataset.py:320-323)."""
    if "annos" not in dataset.kitti_infos[0]:
        raise ValueError("the split has no labels: nothing to evaluate against")
    return [copy.deepcopy(info["annos"]) for info in dataset.kitti_infos]


def eval_checkpoint(cfg, model, test_set, test_loader, ckpt, epoch_id, result_dir, logger, save_to_file=False, log_every=0):
    """One checkpoint through eval_one_epoch_device; the returned dict also goes to <result_dir>/metrics.json."""
    from . import eval_loop
    model.load_params_from_file(filename=str(ckpt), logger=logger)
    model.cuda()
    test_loader.sampler.set_epoch(0)
    with torch.no_grad():
        ret = eval_loop.eval_one_epoch_device(cfg, model, test_loader, gt_annos_of(test_set), epoch_id=epoch_id, logger=logger,
                                              save_to_file=save_to_file, result_dir=Path(result_dir), log_every=log_every)
    with open(Path(result_dir) / "metrics.json", "w") as f:
        json.dump({k: float(v) for k, v in ret.items()}, f, indent=1, sort_keys=True)
    return ret


def get_no_evaluated_ckpt(ckpt_dir, ckpt_record_file, start_epoch):
    """(epoch id, path) of the oldest checkpoint_epoch_<id>.pth (by mtime) that the record file does not list and whose epoch is
    at least start_epoch; (-1, None) when there is none (tools/test.py:67-82)."""
    files = sorted(glob.glob(os.path.join(str(ckpt_dir), "*checkpoint_epoch_*.pth")), key=os.path.getmtime)
    with open(ckpt_record_file) as f:
        done = [float(x.strip()) for x in f.readlines() if x.strip()]
    for path in files:
        ids = re.findall(r"checkpoint_epoch_(.*)\.pth", os.path.basename(path))
        if not ids or "optim" in ids[-1]:
            continue
        try:
            e = float(ids[-1])
        except ValueError:
            continue
        if e not in done and int(e) >= start_epoch:
            return ids[-1], path
    return -1, None


def repeat_eval_ckpt(cfg, model, test_set, test_loader, args, eval_output_dir, logger, ckpt_dir, wait_seconds=30):
    """Evaluates every checkpoint of ckpt_dir not yet listed in eval_list_<split>.txt, oldest first, then waits for new ones up to
    --max_waiting_mins (0: ends as soon as nothing is left).  Returns {epoch id: result dict}."""
    split = test_split(cfg)
    eval_output_dir = Path(eval_output_dir)
    eval_output_dir.mkdir(parents=True, exist_ok=True)
    record = eval_output_dir / ("eval_list_%s.txt" % split)
    with open(record, "a"):
        pass
    waited, results = 0, {}
    while True:
        epoch_id, ckpt = get_no_evaluated_ckpt(ckpt_dir, record, args.start_epoch)
        if ckpt is None:
            if waited >= args.max_waiting_mins * 60:
                break
            time.sleep(wait_seconds)
            waited += wait_seconds
            continue
        waited = 0
        results[epoch_id] = eval_checkpoint(cfg, model, test_set, test_loader, ckpt, epoch_id,
                                            eval_output_dir / ("epoch_%s" % epoch_id) / split, logger, args.save_to_file)
        with open(record, "a") as f:
            print("%s" % epoch_id, file=f)
        logger.info("Epoch %s has been evaluated" % epoch_id)
    return results


def log_run(logger, args, cfg):
    logger.info("**********************Start logging**********************")
    for key, val in vars(args).items():
        logger.info("{:16} {}".format(key, val))
    logger.info("config: %s" % json.dumps(cfg, default=str))


def build_test_loader(cfg, args, batch_size, device):
    from .epoch_loader import build_dataloader
    return build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size, dist=False, root_path=args.data_path, training=False,
                            seed=args.seed, device=str(device), prefetch=not args.no_prefetch)


def main(argv=None):
    from .detector import build_network
    args, cfg = parse_config(argv)
    dist_test, rank, world, device = init_launcher(args, cfg)
    batch_size = per_rank_batch_size(args, cfg, world)
    output_dir = output_dir_of(args, cfg)
    eval_output_dir, epoch_id = eval_dir_of(args, cfg, output_dir)
    if not args.eval_all and args.ckpt is None:
        raise SystemExit("evaluate: give --ckpt, or --eval_all with --ckpt_dir")
    results = None
    if rank == 0:
        eval_output_dir.mkdir(parents=True, exist_ok=True)
        logger = create_logger(eval_output_dir / ("log_eval_%s.txt" % datetime.datetime.now().strftime("%Y%m%d-%H%M%S")), rank)
        log_run(logger, args, cfg)
        ckpt_dir = Path(args.ckpt_dir) if args.ckpt_dir is not None else output_dir / "ckpt"
        test_set, test_loader, _ = build_test_loader(cfg, args, batch_size, device)
        model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), test_set)
        if args.eval_all:
            results = repeat_eval_ckpt(cfg, model, test_set, test_loader, args, eval_output_dir, logger, ckpt_dir)
        else:
            results = {epoch_id: eval_checkpoint(cfg, model, test_set, test_loader, args.ckpt, epoch_id, eval_output_dir, logger,
                                                 args.save_to_file)}
    if dist_test:
        distributed.barrier(device)
        distributed.finalize()
    return results


if __name__ == "__main__":
    main()
