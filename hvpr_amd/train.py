"""python -m hvpr_amd.train: a KITTI folder (with the info pickles and the GT database of
`python -m hvpr_amd.kitti_dataset create_kitti_infos`) in, checkpoints and the AP table of the last epochs out.

The reference's tools/train.py over this package's own pieces: `epoch_loader.build_dataloader`, `detector.build_network`,
`optim.build_optimizer` / `build_scheduler` / `model_fn_decorator`, `train_loop.train_model`, then `evaluate.repeat_eval_ckpt` over
the checkpoints from epoch max(epochs - 10, 0) on.  Output: <output_dir>/<cfg stem>/<extra_tag>/{ckpt/checkpoint_epoch_<e>.pth,
log_train_<time>.txt, scalars.jsonl, eval/eval_with_train/{eval_list_<split>.txt, epoch_<e>/<split>/{result.pkl, metrics.json}}}.

Resume: `--ckpt`, else the newest ckpt/*checkpoint_epoch_*.pth, through `load_params_with_optimizer`; an epoch is a pure function of
(seed, epoch, rank), so a resumed run continues as the uninterrupted one would.  `--launcher pytorch` (under torch.distributed.run)
trains data-parallel through `distributed.init` / `convert_sync_batchnorm` / `wrap_ddp`; evaluation then runs on rank 0 only while
the other ranks wait at a barrier (sharded evaluation is not built)."""
import argparse
import datetime
import glob
import os
import random
import shutil

import numpy as np
import torch

from . import distributed, evaluate as E
from .common_utils import create_logger


def parse_config(argv=None):
    parser = argparse.ArgumentParser(prog="python -m hvpr_amd.train", description="train on the KITTI train split, evaluate on val")
    parser.add_argument("--epochs", type=int, default=None)
    parser.add_argument("--pretrained_model", type=str, default=None)
    parser.add_argument("--sync_bn", action="store_true", default=False)
    parser.add_argument("--fix_random_seed", action="store_true", default=False)
    parser.add_argument("--ckpt_save_interval", type=int, default=1)
    parser.add_argument("--max_ckpt_save_num", type=int, default=30)
    parser.add_argument("--merge_all_iters_to_one_epoch", action="store_true", default=False)
    E.common_arguments(parser)
    args = parser.parse_args(argv)
    return args, E.finish_config(args)


def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def newest_checkpoint(ckpt_dir):
    files = sorted(glob.glob(os.path.join(str(ckpt_dir), "*checkpoint_epoch_*.pth")), key=os.path.getmtime)
    return files[-1] if files else None


def main(argv=None):
    from . import optim, train_loop
    from .detector import build_network
    from .epoch_loader import build_dataloader
    args, cfg = parse_config(argv)
    dist_train, rank, world, device = E.init_launcher(args, cfg)
    batch_size = E.per_rank_batch_size(args, cfg, world)
    epochs = int(cfg.OPTIMIZATION.NUM_EPOCHS) if args.epochs is None else args.epochs
    if args.fix_random_seed:
        set_random_seed(2020)
    output_dir = E.output_dir_of(args, cfg)
    ckpt_dir = output_dir / "ckpt"
    ckpt_dir.mkdir(parents=True, exist_ok=True)
    logger = create_logger(output_dir / ("log_train_%s.txt" % datetime.datetime.now().strftime("%Y%m%d-%H%M%S")), rank)
    if dist_train:
        logger.info("total_batch_size: %d" % (world * batch_size))
    E.log_run(logger, args, cfg)
    if rank == 0 and os.path.abspath(os.path.dirname(args.cfg_file)) != str(output_dir.resolve()):
        shutil.copy(args.cfg_file, str(output_dir))

    train_set, train_loader, train_sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size, dist=dist_train,
                                                              root_path=args.data_path, training=True, seed=args.seed,
                                                              device=str(device), prefetch=not args.no_prefetch)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), train_set)
    if args.sync_bn and dist_train:
        model = distributed.convert_sync_batchnorm(model)
    model.to(device)
    optimizer = optim.build_optimizer(model, cfg.OPTIMIZATION)

    start_epoch = it = 0
    last_epoch = -1
    if args.pretrained_model is not None:
        model.load_params_from_file(filename=args.pretrained_model, to_cpu=dist_train, logger=logger)
    resume = args.ckpt if args.ckpt is not None else newest_checkpoint(ckpt_dir)
    if resume is not None:
        it, start_epoch = model.load_params_with_optimizer(resume, to_cpu=dist_train, optimizer=optimizer, logger=logger)
        last_epoch = start_epoch + 1
    model.train()
    net = model
    if dist_train:
        model = distributed.wrap_ddp(model, device)
    lr_scheduler, lr_warmup_scheduler = optim.build_scheduler(optimizer, total_iters_each_epoch=len(train_loader), total_epochs=epochs,
                                                              last_epoch=last_epoch, optim_cfg=cfg.OPTIMIZATION)

    logger.info("**********************Start training %s(%s)**********************" % (cfg.TAG, args.extra_tag))
    train_loop.train_model(model, optimizer, train_loader, optim.model_fn_decorator(), lr_scheduler, cfg.OPTIMIZATION,
                           start_epoch=start_epoch, total_epochs=epochs, start_iter=int(it), rank=rank, ckpt_save_dir=ckpt_dir,
                           logger=logger, train_sampler=train_sampler, ckpt_save_interval=args.ckpt_save_interval,
                           max_ckpt_save_num=args.max_ckpt_save_num, log_interval=args.log_interval,
                           scalars_path=output_dir / "scalars.jsonl", lr_warmup_scheduler=lr_warmup_scheduler)
    logger.info("**********************End training %s(%s)**********************" % (cfg.TAG, args.extra_tag))

    results = None
    if rank == 0:
        logger.info("**********************Start evaluation %s(%s)**********************" % (cfg.TAG, args.extra_tag))
        test_set, test_loader, _ = E.build_test_loader(cfg, args, batch_size, device)
        args.start_epoch = max(epochs - 10, 0)            # only the last ten epochs
        results = E.repeat_eval_ckpt(cfg, net, test_set, test_loader, args, output_dir / "eval" / "eval_with_train", logger, ckpt_dir)
        logger.info("**********************End evaluation %s(%s)**********************" % (cfg.TAG, args.extra_tag))
    if dist_train:
        distributed.barrier(device)
        distributed.finalize()
    return results


if __name__ == "__main__":
    main()
