"""The epoch loop of training: the reference's train_one_epoch / train_model (tools/train_utils/train_utils.py:9-114) over the
product's own pieces — `optim.model_fn_decorator`, the flat optimiser's `clip_grad_norm`, `optim.checkpoint_state` /
`save_checkpoint` — in the call order fixture G17 records: scheduler.step(it), model.train(), zero_grad, model function, backward,
clip, step.

Logging.  The loop itself never synchronises on an iteration that does not log: `loss` and the device scalars of `tb_dict` are
stacked into one device row per iteration (ScalarLog), and the rows are read in ONE read every `log_interval` iterations and at the
end of the epoch.  Each read appends a line to `scalars.jsonl`: the iteration, lr, loss and tb values of the newest row, and the
losses of every row the read brought back.  tensorboardX is not used: it would force a read per scalar.

What still synchronises inside an iteration is not the loop's: the reads of `DeviceBatchLoader.prepare_batch` (on the loader's own
stream with `EpochLoader(prefetch=True)`) and whatever the training step itself reads."""
import glob
import json
import os

import torch

from . import optim


class ScalarLog:
    """Device rows of (loss, tb scalars) per iteration, read back together.  `path`: the scalars.jsonl to append to (None: keep
    the lines in `.lines` only)."""

    def __init__(self, path=None, log_interval=50):
        self.path, self.log_interval = (None if path is None else str(path)), max(1, int(log_interval))
        self.keys, self.rows, self.meta, self.lines, self.reads = None, [], [], [], 0

    def add(self, it, lr, loss, tb_dict):
        if self.keys is None:
            self.keys = [k for k, v in tb_dict.items() if torch.is_tensor(v) and v.numel() == 1]
        self.rows.append(torch.stack([loss.detach().reshape(()).float()] + [tb_dict[k].detach().reshape(()).float() for k in self.keys]))
        self.meta.append((int(it), float(lr), {k: float(v) for k, v in tb_dict.items() if isinstance(v, (int, float))}))
        if len(self.rows) >= self.log_interval:
            self.flush()

    def flush(self):
        """ONE read of every row since the last one; returns the line written (None when there was nothing)."""
        if not self.rows:
            return None
        host = torch.stack(self.rows).cpu().tolist()
        self.reads += 1
        it, lr, extra = self.meta[-1]
        line = {"it": it, "lr": lr, "loss": host[-1][0], **dict(zip(self.keys, host[-1][1:])), **extra,
                "first_it": self.meta[0][0], "losses": [r[0] for r in host]}
        self.rows, self.meta = [], []
        self.lines.append(line)
        if self.path is not None:
            with open(self.path, "a") as f:
                f.write(json.dumps(line) + "\n")
        return line


def train_one_epoch(model, optimizer, train_loader, model_func, lr_scheduler, accumulated_iter, optim_cfg, rank=0, scalar_log=None,
                    logger=None):
    """One pass over `train_loader`; returns (accumulated_iter, the memory items of the last iteration)."""
    items = None
    flat_clip = hasattr(optimizer, "clip_grad_norm")
    step_done = getattr(train_loader, "step_done", None)
    batches = optim.prefetching(model, train_loader) if getattr(train_loader, "prefetch", True) else train_loader
    for batch in batches:
        lr_scheduler.step(accumulated_iter)
        cur_lr = float(optimizer.lr) if hasattr(optimizer, "lr") else optimizer.param_groups[0]["lr"]
        model.train()
        optimizer.zero_grad()
        loss, tb_dict, disp_dict, items = model_func(model, batch)
        loss.backward()
        if flat_clip:                                   # the clip coefficient stays on the device
            optimizer.clip_grad_norm(optim_cfg.GRAD_NORM_CLIP)
        else:
            torch.nn.utils.clip_grad_norm_(model.parameters(), optim_cfg.GRAD_NORM_CLIP)
        optimizer.step()
        accumulated_iter += 1
        if step_done is not None:
            step_done()
        if scalar_log is not None and rank == 0:
            before = scalar_log.reads
            scalar_log.add(accumulated_iter, cur_lr, loss, tb_dict)
            if scalar_log.reads != before and logger is not None:
                line = scalar_log.lines[-1]
                logger.info("it %d  lr %.3e  loss %.4f" % (line["it"], line["lr"], line["loss"]))
    if scalar_log is not None:
        scalar_log.flush()
    return accumulated_iter, items


def rotate_checkpoints(ckpt_save_dir, max_ckpt_save_num):
    """Deletes the oldest checkpoint_epoch_*.pth (by mtime) so that, with the one about to be written, at most max_ckpt_save_num
    remain (train_utils.py:102-109).  Returns the files removed."""
    files = sorted(glob.glob(os.path.join(str(ckpt_save_dir), "checkpoint_epoch_*.pth")), key=os.path.getmtime)
    gone = files[: max(0, len(files) - int(max_ckpt_save_num) + 1)] if len(files) >= max_ckpt_save_num else []
    for f in gone:
        os.remove(f)
    return gone


def train_model(model, optimizer, train_loader, model_func, lr_scheduler, optim_cfg, start_epoch, total_epochs, start_iter, rank,
                ckpt_save_dir, logger, train_sampler=None, ckpt_save_interval=1, max_ckpt_save_num=50,
                merge_all_iters_to_one_epoch=False, log_interval=50, scalars_path=None, lr_warmup_scheduler=None):
    """Epochs start_epoch .. total_epochs - 1; a checkpoint `checkpoint_epoch_<e>.pth` every ckpt_save_interval epochs on rank 0.
    `lr_warmup_scheduler` (build_scheduler's second value) steps instead of `lr_scheduler` in the epochs before
    optim_cfg.WARMUP_EPOCH (train_utils.py:82-85).  Returns the iteration count."""
    if merge_all_iters_to_one_epoch:
        raise NotImplementedError("merge_all_iters_to_one_epoch is not built")
    accumulated_iter = start_iter
    scalar_log = ScalarLog(scalars_path, log_interval) if rank == 0 else None
    for cur_epoch in range(start_epoch, total_epochs):
        if train_sampler is not None:
            train_sampler.set_epoch(cur_epoch)
        warming_up = lr_warmup_scheduler is not None and cur_epoch < optim_cfg.WARMUP_EPOCH
        cur_scheduler = lr_warmup_scheduler if warming_up else lr_scheduler
        accumulated_iter, items = train_one_epoch(model, optimizer, train_loader, model_func, cur_scheduler, accumulated_iter, optim_cfg,
                                                  rank=rank, scalar_log=scalar_log, logger=logger)
        trained_epoch = cur_epoch + 1
        logger.info("**********************Epoch%d training finished**********************" % trained_epoch)
        logger.info("memory items(Epoch%d):  " % trained_epoch)
        if items is not None and rank == 0:
            logger.info(str(items[:20]))
        if trained_epoch % ckpt_save_interval == 0 and rank == 0:
            rotate_checkpoints(ckpt_save_dir, max_ckpt_save_num)
            optim.save_checkpoint(optim.checkpoint_state(model, optimizer, trained_epoch, accumulated_iter),
                                  filename=os.path.join(str(ckpt_save_dir), "checkpoint_epoch_%d" % trained_epoch))
    return accumulated_iter
