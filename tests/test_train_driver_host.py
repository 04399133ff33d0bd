"""CPU: the epoch sampler's arithmetic, `--set`, the commands' arguments, output layout, checkpoint selection and rotation."""
import os
import time

import numpy as np
import pytest
import torch

from hvpr_amd import config, evaluate, train, train_loop
from hvpr_amd.epoch_loader import EpochSampler

CAR_YAML = os.path.join(config.CFG_DIR, "kitti_models", "hvpr_car.yaml")


# ------------------------------------------------------------------------------------------------ sampler
def _perm(n, seed, epoch):
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    return torch.randperm(n, generator=g).tolist()


def test_sampler_one_rank_and_three_ranks_cut_the_same_permutation():
    n = 10
    for epoch in (0, 3):
        perm = _perm(n, 5, epoch)
        one = EpochSampler(n, 4, True, seed=5)
        one.set_epoch(epoch)
        assert one.indices() == perm                                    # world 1: no padding
        padded = perm + perm[:2]                                        # 12 = 3 * ceil(10 / 3)
        seen = set()
        for r in range(3):
            s = EpochSampler(n, 4, True, seed=5, rank=r, world=3)
            s.set_epoch(epoch)
            assert s.indices() == padded[r::3] and len(s.indices()) == 4 == s.num_samples
            seen |= set(s.indices())
        assert seen == set(range(n))


def test_sampler_evaluation_order_len_and_epochs():
    s = EpochSampler(10, 4, False, seed=9)
    assert s.indices() == list(range(10))
    assert [len(b) for b in s] == [4, 4, 2] and len(s) == 3            # drop_last is false: the last batch is short
    assert EpochSampler(10, 4, False, rank=2, world=3).indices() == [2, 5, 8, 1]      # arange padded with its head, strided
    assert len(EpochSampler(10, 4, True, rank=0, world=3)) == 1 and len(EpochSampler(8, 4, True)) == 2 and len(EpochSampler(9, 4, True)) == 3
    a = EpochSampler(10, 4, True, seed=1)
    a.set_epoch(0)
    e0 = a.indices()
    a.set_epoch(1)
    e1 = a.indices()
    a.set_epoch(0)
    assert e0 != e1 and a.indices() == e0 and sorted(e1) == list(range(10))
    b = EpochSampler(10, 4, True, seed=1)
    assert b.indices() == e0 and [i for batch in b for i in batch] == e0
    with pytest.raises(ValueError):
        EpochSampler(10, 4, True, rank=3, world=3)


# ------------------------------------------------------------------------------------------------ --set
def test_cfg_from_list():
    cfg = config.hvpr_car_cfg()
    config.cfg_from_list(["MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS", "True", "OPTIMIZATION.LR", "1", "OPTIMIZATION.MOMS", "0.9,0.8",
                          "MODEL.POST_PROCESSING.NMS_CONFIG.NMS_TYPE", "nms_gpu", "OPTIMIZATION.NUM_EPOCHS", "7"], cfg)
    assert cfg.MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS is True and cfg.OPTIMIZATION.LR == 1.0 and isinstance(cfg.OPTIMIZATION.LR, float)
    assert cfg.OPTIMIZATION.MOMS == [0.9, 0.8] and cfg.OPTIMIZATION.NUM_EPOCHS == 7
    with pytest.raises(KeyError):
        config.cfg_from_list(["MODEL.NO_SUCH_KEY", "1"], cfg)
    with pytest.raises(TypeError):
        config.cfg_from_list(["OPTIMIZATION.NUM_EPOCHS", "many"], cfg)
    with pytest.raises(TypeError):
        config.cfg_from_list(["MODEL.POST_PROCESSING", "1"], cfg)
    with pytest.raises(ValueError):
        config.cfg_from_list(["OPTIMIZATION.LR"], cfg)


# ------------------------------------------------------------------------------------------------ arguments and layout
def test_train_arguments_and_output_layout(tmp_path):
    args, cfg = train.parse_config(["--cfg_file", CAR_YAML, "--batch_size", "2", "--epochs", "3", "--extra_tag", "t1", "--output_dir", str(tmp_path),
                                    "--data_path", "/data/kitti", "--max_ckpt_save_num", "2", "--no_prefetch", "--seed", "4", "--workers", "9",
                                    "--set", "MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS", "True"])
    assert (args.batch_size, args.epochs, args.max_ckpt_save_num, args.no_prefetch, args.seed, args.log_interval) == (2, 3, 2, True, 4, 50)
    assert args.launcher == "none" and args.max_waiting_mins == 0 and not args.fix_random_seed and args.ckpt_save_interval == 1
    assert cfg.TAG == "hvpr_car" and cfg.MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS is True
    out = evaluate.output_dir_of(args, cfg)
    assert out == tmp_path / "hvpr_car" / "t1"
    assert evaluate.test_split(cfg) == "val" and evaluate.per_rank_batch_size(args, cfg, 2) == 1
    with pytest.raises(ValueError):
        evaluate.per_rank_batch_size(args, cfg, 4)


def test_evaluate_arguments_and_result_directories(tmp_path):
    args, cfg = evaluate.parse_config(["--cfg_file", CAR_YAML, "--ckpt", "/x/ckpt/checkpoint_epoch_12.pth", "--output_dir", str(tmp_path), "--save_to_file"])
    out = evaluate.output_dir_of(args, cfg)
    d, epoch_id = evaluate.eval_dir_of(args, cfg, out)
    assert epoch_id == "12" and d == tmp_path / "hvpr_car" / "default" / "eval" / "epoch_12" / "val" / "default" and args.save_to_file
    assert evaluate.per_rank_batch_size(args, cfg, 1) == cfg.OPTIMIZATION.BATCH_SIZE_PER_GPU
    args, cfg = evaluate.parse_config(["--cfg_file", CAR_YAML, "--eval_all", "--eval_tag", "again", "--ckpt_dir", "/x/ckpt"])
    d, epoch_id = evaluate.eval_dir_of(args, cfg, tmp_path)
    assert epoch_id is None and d == tmp_path / "eval" / "eval_all_default" / "again"


def test_unbuilt_flags_say_so():
    with pytest.raises(NotImplementedError, match="slurm"):
        train.parse_config(["--cfg_file", CAR_YAML, "--launcher", "slurm"])
    with pytest.raises(NotImplementedError, match="slurm"):
        evaluate.parse_config(["--cfg_file", CAR_YAML, "--launcher", "slurm"])
    with pytest.raises(NotImplementedError, match="merge_all_iters_to_one_epoch"):
        train.parse_config(["--cfg_file", CAR_YAML, "--merge_all_iters_to_one_epoch"])
    with pytest.raises(NotImplementedError, match="merge_all_iters_to_one_epoch"):
        train_loop.train_model(None, None, [], None, None, None, 0, 1, 0, 0, ".", None, merge_all_iters_to_one_epoch=True)


# ------------------------------------------------------------------------------------------------ checkpoints on disk
def _touch(path, mtime):
    path.write_bytes(b"")
    os.utime(path, (mtime, mtime))


def test_not_evaluated_checkpoint_selection(tmp_path):
    now = time.time()
    for k, e in enumerate(("3", "1", "2", "10")):                      # written in this order: mtime, not name, decides
        _touch(tmp_path / ("checkpoint_epoch_%s.pth" % e), now - 100 + k)
    _touch(tmp_path / "checkpoint_epoch_4_optim.pth", now - 200)
    _touch(tmp_path / "other.pth", now - 300)
    record = tmp_path / "eval_list_val.txt"
    record.write_text("")
    pick = lambda start: evaluate.get_no_evaluated_ckpt(tmp_path, record, start)
    assert pick(0) == ("3", str(tmp_path / "checkpoint_epoch_3.pth"))
    record.write_text("3\n")
    assert pick(0)[0] == "1" and pick(2)[0] == "2" and pick(5)[0] == "10" and pick(11) == (-1, None)
    record.write_text("3\n1\n2\n10\n")
    assert pick(0) == (-1, None)
    assert train.newest_checkpoint(tmp_path).endswith("checkpoint_epoch_10.pth") and train.newest_checkpoint(tmp_path / "none") is None


def test_checkpoint_rotation_keeps_the_newest(tmp_path):
    now = time.time()
    for e in (1, 2, 3):
        _touch(tmp_path / ("checkpoint_epoch_%d.pth" % e), now - 100 + e)
    assert train_loop.rotate_checkpoints(tmp_path, 5) == []
    gone = train_loop.rotate_checkpoints(tmp_path, 2)                  # room for the one about to be written
    assert [os.path.basename(g) for g in gone] == ["checkpoint_epoch_1.pth", "checkpoint_epoch_2.pth"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["checkpoint_epoch_3.pth"]


def test_scalar_log_reads_once_per_interval(tmp_path):
    log = train_loop.ScalarLog(tmp_path / "scalars.jsonl", log_interval=2)
    for it in range(1, 4):
        log.add(it, 0.1 * it, torch.tensor(float(it)), {"loss_rpn": torch.tensor(2.0 * it), "host": 1.5})
    assert log.reads == 1 and log.lines[0]["it"] == 2 and log.lines[0]["losses"] == [1.0, 2.0] and log.lines[0]["loss_rpn"] == 4.0
    line = log.flush()
    assert log.reads == 2 and line["it"] == 3 and line["first_it"] == 3 and line["host"] == 1.5 and log.flush() is None
    import json
    rows = [json.loads(x) for x in open(tmp_path / "scalars.jsonl")]
    assert [r["it"] for r in rows] == [2, 3] and abs(rows[1]["lr"] - 0.3) < 1e-12
