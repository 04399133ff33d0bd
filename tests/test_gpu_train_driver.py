"""GPU: the epoch loader (prefetch against no prefetch), the training loop (determinism, prefetch, resume, synchronising calls,
checkpoint rotation) and the two commands, on the tiny KITTI tree of train_driver_cases: 6 train and 4 val frames, batch 2, 3
iterations an epoch, the full hvpr_car model."""
import glob
import json
import os
import pickle
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import train_driver_cases as C
from hvpr_amd import optim, train_loop
from hvpr_amd.detector import build_network
from hvpr_amd.epoch_loader import build_dataloader

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return C.write_tree_with_infos(tmp_path_factory.mktemp("kitti"))


@pytest.fixture(scope="module")
def tree_with_an_empty_frame(tmp_path_factory):
    """Train frame 2 has no box of its own: it is redrawn."""
    return C.write_tree_with_infos(tmp_path_factory.mktemp("kitti_empty"), empty_train_frame=2)


class _Quiet:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(str(s))


# ------------------------------------------------------------------------------------------------ loader
def _epochs_of(tree, cfg, prefetch, batch_size=4, epochs=2):
    ds, loader, sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size, root_path=tree, training=True, seed=3,
                                           prefetch=prefetch)
    out = []
    for e in range(epochs):
        sampler.set_epoch(e)
        for b in loader:
            torch.cuda.current_stream().synchronize()
            out.append({k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in b.items() if k not in ("calib", "permutations")})
            loader.step_done()
    return out, ds, loader


def _same_value(a, b, k):
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), k
        for x, y in zip(a, b):
            _same_value(x, y, k)
    elif isinstance(a, dict):
        assert sorted(a) == sorted(b), k
        for j in a:
            _same_value(a[j], b[j], k)
    else:
        assert a == b, k


@pytest.mark.parametrize("gt_sampling", [True, False])
def test_batches_with_prefetch_equal_those_without(tree_with_an_empty_frame, gt_sampling):
    tree = tree_with_an_empty_frame
    cfg = C.model_cfg(gt_sampling=gt_sampling)
    plain, ds, _ = _epochs_of(tree, cfg, False)
    ahead, _, loader = _epochs_of(tree, cfg, True)
    assert len(plain) == len(ahead) == 4 and [b["batch_size"] for b in plain] == [4, 2, 4, 2]        # the short last batch
    assert ds.point_feature_encoder.num_point_features == 4 and list(ds.grid_size[:2]) == [296, 248]
    for a, b in zip(plain, ahead):
        assert sorted(a) == sorted(b)
        for k in a:
            _same_value(a[k], b[k], k)
        assert a["points"].shape == (a["batch_size"] * C.NUM_POINTS, 5)
    assert plain[0]["points"].tobytes() != plain[2]["points"].tobytes()                            # epochs differ
    redrawn = [b["redraw_index"] for b in plain if b["redraw_index"]]
    assert len(redrawn) == 2 and all(len(r) == 1 for r in redrawn)          # the empty frame, once an epoch: its slot was drawn again
    assert all("000102" not in b["frame_id"] for b in plain)
    assert loader._stream is not None and loader._stream != torch.cuda.current_stream()


# ------------------------------------------------------------------------------------------------ loop
def _pieces(tree, prefetch, sched_epochs, seed=0):
    cfg = C.model_cfg()
    ds, loader, sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, root_path=tree, training=True, seed=seed, prefetch=prefetch)
    torch.manual_seed(0)
    np.random.seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda()
    opt = optim.build_optimizer(model, cfg.OPTIMIZATION)
    return cfg, loader, sampler, model, opt


def _train(tree, ckpt_dir, prefetch, start_stop, sched_epochs=2, resume=None, max_ckpt=50, log_interval=2):
    """Everything built anew, epochs start_stop[0] .. start_stop[1] - 1 of a schedule of sched_epochs epochs."""
    cfg, loader, sampler, model, opt = _pieces(tree, prefetch, sched_epochs)
    it = start_epoch = 0
    if resume is not None:
        it, start_epoch = model.load_params_with_optimizer(resume, optimizer=opt)
    assert start_epoch == start_stop[0]
    model.train()
    sched, _ = optim.build_scheduler(opt, len(loader), sched_epochs, start_epoch + 1 if resume else -1, cfg.OPTIMIZATION)
    Path(ckpt_dir).mkdir(parents=True, exist_ok=True)
    logger = _Quiet()
    n = train_loop.train_model(model, opt, loader, optim.model_fn_decorator(), sched, cfg.OPTIMIZATION, start_epoch, start_stop[1], int(it), 0,
                               Path(ckpt_dir), logger, train_sampler=sampler, max_ckpt_save_num=max_ckpt, log_interval=log_interval,
                               scalars_path=Path(ckpt_dir) / "scalars.jsonl")
    torch.cuda.synchronize()
    state = {"model." + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for i, st in opt.state_dict()["state"].items():
        for k, v in st.items():
            state["opt.%s.%s" % (i, k)] = v.detach().cpu().clone() if torch.is_tensor(v) else torch.tensor(v)
    return {"state": state, "it": n, "log": logger.lines, "global_step": int(model.global_step)}


def _run(tree, tmp, name, **kw):
    if name not in _RUNS:
        _RUNS[name] = _train(tree, tmp / name, **kw)
    return _RUNS[name]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("runs")


def _same_state(a, b):
    assert sorted(a["state"]) == sorted(b["state"]) and a["it"] == b["it"]
    worst = max(((a["state"][k].double() - b["state"][k].double()).abs().max().item(), k) for k in a["state"] if a["state"][k].numel())
    unequal = [k for k in a["state"] if not torch.equal(a["state"][k], b["state"][k])]
    assert not unequal, (len(unequal), worst)


def test_loop_is_deterministic_and_counts(tree, tmp):
    """(i) two identical runs end bit-identical; (vi) the loss is finite and the steps count."""
    a = _run(tree, tmp, "plain_a", prefetch=False, start_stop=(0, 2))
    b = _run(tree, tmp, "plain_b", prefetch=False, start_stop=(0, 2))
    _same_state(a, b)
    assert a["it"] == 6 and a["global_step"] == 6
    rows = [json.loads(x) for x in open(tmp / "plain_a" / "scalars.jsonl")]
    assert [r["it"] for r in rows] == [2, 3, 5, 6]                   # every second iteration, and the end of each epoch
    losses = [l for r in rows for l in r["losses"]]
    assert len(losses) == 6 and all(np.isfinite(l) for l in losses) and all("loss_rpn" in r and r["lr"] > 0 for r in rows)
    assert any("Epoch2 training finished" in s for s in a["log"]) and any(s.startswith("memory items(Epoch1)") for s in a["log"])
    assert all(torch.isfinite(v.double()).all() for v in a["state"].values())


def test_prefetch_changes_nothing(tree, tmp):
    """(ii)"""
    _same_state(_run(tree, tmp, "plain_a", prefetch=False, start_stop=(0, 2)), _run(tree, tmp, "ahead", prefetch=True, start_stop=(0, 2)))


def test_resume_continues_the_uninterrupted_run(tree, tmp):
    """(iii) two epochs in one go against one epoch, everything built anew, resume, one more epoch."""
    whole = _run(tree, tmp, "plain_a", prefetch=False, start_stop=(0, 2))
    first = _run(tree, tmp, "half", prefetch=False, start_stop=(0, 1))
    assert first["it"] == 3
    ckpt = train_loop_newest(tmp / "half")
    assert ckpt.endswith("checkpoint_epoch_1.pth")
    saved = torch.load(ckpt, map_location="cpu")
    assert (saved["epoch"], saved["it"]) == (1, 3) and saved["optimizer_state"] is not None
    second = _run(tree, tmp, "resumed", prefetch=False, start_stop=(1, 2), resume=ckpt)
    _same_state(whole, second)


def train_loop_newest(d):
    from hvpr_amd import train
    return train.newest_checkpoint(d)


def test_checkpoint_rotation_and_resume_choice(tree, tmp):
    """(v) max_ckpt_save_num = 2 over 3 epochs leaves epochs 2 and 3; resume picks 3."""
    r = _run(tree, tmp, "three", prefetch=True, start_stop=(0, 3), sched_epochs=3, max_ckpt=2)
    assert r["it"] == 9 and r["global_step"] == 9
    left = sorted(os.path.basename(p) for p in glob.glob(str(tmp / "three" / "checkpoint_epoch_*.pth")))
    assert left == ["checkpoint_epoch_2.pth", "checkpoint_epoch_3.pth"]
    assert train_loop_newest(tmp / "three").endswith("checkpoint_epoch_3.pth")


@pytest.mark.parametrize("prefetch", [False, True])
def test_the_loop_adds_no_synchronising_call(tree, prefetch):
    """(iv) an iteration that does not log warns as often as optim.train_step on the same batch plus the loader's two reads; one
    that logs warns once more."""
    cfg, loader, sampler, model, opt = _pieces(tree, prefetch, 4)
    sched, _ = optim.build_scheduler(opt, len(loader), 4, -1, cfg.OPTIMIZATION)
    fn = optim.model_fn_decorator()
    it, _ = train_loop.train_one_epoch(model, opt, loader, fn, sched, 0, cfg.OPTIMIZATION)        # lazy initialisation
    batch = loader.batch_loader.prepare_batch([0, 1], np.random.RandomState(0))
    optim.train_step(model, opt, sched, dict(batch), it, cfg.OPTIMIZATION.GRAD_NORM_CLIP)
    _, step = C.sync_warnings(lambda: optim.train_step(model, opt, sched, dict(batch), it + 1, cfg.OPTIMIZATION.GRAD_NORM_CLIP))
    it += 2
    torch.cuda.synchronize()
    counts = {}
    for epoch, interval in ((1, 1000), (2, 1)):
        sampler.set_epoch(epoch)
        log = train_loop.ScalarLog(None, interval)
        reads = loader.batch_loader.reads
        (it, _), counts[interval] = C.sync_warnings(lambda: train_loop.train_one_epoch(model, opt, loader, fn, sched, it, cfg.OPTIMIZATION,
                                                                                       scalar_log=log))
        assert loader.batch_loader.reads - reads == 2 * 3            # no redraw in these epochs
        assert log.reads == (1 if interval == 1000 else 3)
    assert counts[1000] == 3 * (step + 2) + 1, (counts, step)         # three quiet iterations and the read at the epoch's end
    assert counts[1] == 3 * (step + 2) + 3, (counts, step)            # every iteration logs: one more each


# ------------------------------------------------------------------------------------------------ commands
def _command(module, *args, timeout=600):
    r = subprocess.run([sys.executable, "-m", module] + [str(a) for a in args], cwd=ROOT, timeout=timeout, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_train_and_evaluate_commands(tree, tmp_path):
    cfg_file = C.write_cfg(tmp_path / "hvpr_car_tiny.yaml")
    out = tmp_path / "out"
    common = ["--cfg_file", cfg_file, "--batch_size", 2, "--data_path", tree, "--output_dir", out]
    _command("hvpr_amd.train", *common, "--epochs", 2, "--log_interval", 2)
    run = out / "hvpr_car_tiny" / "default"
    assert sorted(p.name for p in (run / "ckpt").iterdir()) == ["checkpoint_epoch_1.pth", "checkpoint_epoch_2.pth"]
    rows = [json.loads(x) for x in open(run / "scalars.jsonl")]
    assert [r["it"] for r in rows] == [2, 3, 5, 6] and all(np.isfinite(r["loss"]) for r in rows)
    assert len(list(run.glob("log_train_*.txt"))) == 1
    with_train = run / "eval" / "eval_with_train"
    assert (with_train / "eval_list_val.txt").read_text().split() == ["1", "2"]
    metrics = {}
    for e in (1, 2):
        with open(with_train / ("epoch_%d" % e) / "val" / "result.pkl", "rb") as f:
            annos = pickle.load(f)
        assert len(annos) == C.N_VAL and [a["frame_id"] for a in annos] == ["%06d" % (200 + i) for i in range(C.N_VAL)]
        metrics[e] = json.load(open(with_train / ("epoch_%d" % e) / "val" / "metrics.json"))
    assert any(k.startswith("recall/rcnn_") for k in metrics[2]) and any("3d" in k for k in metrics[2])
    # evaluate reproduces the last epoch's dict
    _command("hvpr_amd.evaluate", *common, "--ckpt", run / "ckpt" / "checkpoint_epoch_2.pth", "--save_to_file")
    single = run / "eval" / "epoch_2" / "val" / "default"
    assert json.load(open(single / "metrics.json")) == metrics[2] and (single / "result.pkl").exists()
    assert len(list((single / "final_result" / "data").glob("*.txt"))) == C.N_VAL
    # nothing left to do: resumes from epoch 2, trains nothing, evaluates nothing, exits cleanly
    text = _command("hvpr_amd.train", *common, "--epochs", 2)
    assert "Resumed from" in text and "checkpoint_epoch_2.pth" in text
    assert (with_train / "eval_list_val.txt").read_text().split() == ["1", "2"] and len(rows) == len(open(run / "scalars.jsonl").readlines())
