"""GPU: the flat forms of build_optimizer's 'adam' and 'sgd' — FusedAdam / FusedSGD against fixture G25 (the reference's own
optimisers under step decay) and against torch.optim on the device, the two C entry points on raw buffers against a float64
restatement, and one training-driver run with `OPTIMIZATION.OPTIMIZER sgd`."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import optim_cases as C
from hvpr_amd import optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1                      # HVPR_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ 1: fixture G25
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_fused_forms_reproduce_fixture_g25(golden_dir, case):
    want = optim.FusedAdam if C.CASES[case]["OPTIMIZER"] == "adam" else optim.FusedSGD
    opt = C.run_case(golden_dir, case, DEV, 1e-4, want)
    assert opt.steps == C.ITERS * C.EPOCHS and opt.param_groups[0]["initial_lr"] == C.CASES[case]["LR"]


# ------------------------------------------------------------------------------------------------ 2: torch.optim on the device
def _net():
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 17, 3, bias=False), torch.nn.BatchNorm2d(17), torch.nn.ReLU(),
                              torch.nn.Conv2d(17, 5, 1), torch.nn.Flatten(), torch.nn.Linear(5 * 6 * 6, 3)).to(DEV)
    net[3].bias.requires_grad_(False)          # a frozen parameter: keeps its index (4 of 7), has no state
    return net


@pytest.mark.parametrize("name", ["adam", "sgd", "sgd_plain"])
def test_fused_equals_torch_optim_with_clipping_and_checkpoint_interop(name):
    kw = {"adam": dict(lr=0.003, weight_decay=0.01), "sgd": dict(lr=0.01, weight_decay=0.01, momentum=0.9),
          "sgd_plain": dict(lr=0.01, weight_decay=0.01, momentum=0.0)}[name]
    fused_cls, torch_cls = (optim.FusedAdam, torch.optim.Adam) if name == "adam" else (optim.FusedSGD, torch.optim.SGD)

    def pair(net, fused):
        o = fused_cls(net, **kw) if fused else torch_cls(net.parameters(), **kw)
        return o, optim.StepDecayLR(o, [2, 4], 0.1, 1e-7, kw["lr"])
    a, b = _net(), _net()
    (oa, sa), (ob, sb) = pair(a, False), pair(b, True)
    assert ob.index == [0, 1, 2, 3, 5, 6]
    xs = torch.randn(8, 4, 3, 8, 8, device=DEV, generator=torch.Generator(DEV).manual_seed(0)) * 30   # large inputs: the 0.5 clip is active

    def step(m, o, s, it, x):
        s.step(it)
        m.train(); o.zero_grad()
        return float(C.clipped_step(m, o, m(x).pow(2).mean(), 0.5))
    for it in range(5):
        na, nb = step(a, oa, sa, it, xs[it]), step(b, ob, sb, it, xs[it])
        assert na > 0.5 and nb > 0.5                         # clipped
        assert float(ob.lr) == oa.param_groups[0]["lr"]
        for (k, v), (_, w) in zip(a.state_dict().items(), b.state_dict().items()):
            np.testing.assert_allclose(v.float().cpu().numpy(), w.float().cpu().numpy(), rtol=2e-5, atol=1e-7, err_msg=f"step {it} {k}")
    assert torch.equal(a[3].bias, b[3].bias) and torch.equal(b[3].bias, _net()[3].bias)          # frozen
    ta, tb = oa.state_dict(), ob.state_dict()
    assert sorted(ta["state"]) == sorted(tb["state"]) == ([] if name == "sgd_plain" else [0, 1, 2, 3, 5, 6])
    assert set(ta["param_groups"][0]) == set(tb["param_groups"][0]) and tb["param_groups"][0]["params"] == list(range(7))
    # checkpoints move between the two forms, both ways
    c, d = _net(), _net()
    c.load_state_dict(b.state_dict()); d.load_state_dict(b.state_dict())
    oc, od = torch_cls(c.parameters(), **kw), fused_cls(d, **kw)
    oc.load_state_dict(tb); od.load_state_dict(ta)
    assert oc.param_groups[0]["initial_lr"] == od.param_groups[0]["initial_lr"] == kw["lr"]
    sc, sd = (optim.StepDecayLR(o, [2, 4], 0.1, 1e-7, kw["lr"], last_epoch=4) for o in (oc, od))      # a resume: initial_lr came with the groups
    step(a, oa, sa, 5, xs[5]); step(c, oc, sc, 5, xs[5]); step(d, od, sd, 5, xs[5])
    assert name != "adam" or od.steps == 6                 # Adam's counter came with the state; SGD's format has none
    for (k, v), (_, w), (_, u) in zip(a.state_dict().items(), c.state_dict().items(), d.state_dict().items()):
        np.testing.assert_allclose(v.float().cpu().numpy(), w.float().cpu().numpy(), rtol=5e-5, atol=1e-7, err_msg="fused -> torch " + k)
        np.testing.assert_allclose(v.float().cpu().numpy(), u.float().cpu().numpy(), rtol=5e-5, atol=1e-7, err_msg="torch -> fused " + k)


# ------------------------------------------------------------------------------------------------ 3: the C entry points
GUARD = 8
SIZES = [0, 1, 3, 4, 5, 1027]


def _buffers(n, seed, count):
    g = torch.Generator().manual_seed(seed)
    out = []
    for j in range(count):
        t = torch.randn(n + GUARD, generator=g)
        out.append((t.abs() * 0.01 if j == 3 else t).to(DEV))          # slot 3: exp_avg_sq >= 0
    return out


def _adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step, scale):
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    b1, b2, lr, eps, wd, scale = (float(np.float32(x)) for x in (b1, b2, lr, eps, wd, scale))
    g = g * scale + wd * p
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps)
    return [x.astype(np.float32) for x in (p, m, v)]


def _sgd_ref(p, g, buf, lr, mom, wd, scale):
    p, g = p.astype(np.float64), g.astype(np.float64)
    lr, mom, wd, scale = (float(np.float32(x)) for x in (lr, mom, wd, scale))
    d = g * scale + wd * p
    if buf is not None:
        buf = mom * buf.astype(np.float64) + d
        d = buf
    return (p - lr * d).astype(np.float32), None if buf is None else buf.astype(np.float32)


def _check(got, want, n, before, what):
    """The first n elements against the restatement at (2)'s bar; the guard elements keep their bits."""
    got = got.cpu().numpy()
    np.testing.assert_allclose(got[:n], want[:n], rtol=2e-5, atol=1e-7, err_msg=what)
    assert got[n:].tobytes() == before[n:].tobytes(), what + ": guard elements"


@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_fused_adam_l2_entry_point_on_raw_buffers(n, with_scale, wd):
    from hvpr_amd._lib import lib
    from hvpr_amd.kernels import _stream
    p, g, m, v = _buffers(n, 100 + n, 4)
    before = [t.cpu().numpy().copy() for t in (p, g, m, v)]
    scale = torch.tensor([0.37], device=DEV) if with_scale else None
    lr, b1, b2, eps, step = 0.003, 0.9, 0.999, 1e-8, 3
    rc = lib().hvpr_fused_adam_l2_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, wd, step,
                                      None if scale is None else scale.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    want = _adam_ref(*before, lr, b1, b2, eps, wd, step, 0.37 if with_scale else 1.0)
    for t, w, b0, what in zip((p, m, v), want, (before[0], before[2], before[3]), ("p", "exp_avg", "exp_avg_sq")):
        _check(t, w, n, b0, "adam n=%d %s" % (n, what))
    assert g.cpu().numpy().tobytes() == before[1].tobytes()            # the gradients are read only
    if n:
        assert not np.array_equal(p.cpu().numpy()[:n], before[0][:n])


@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_fused_sgd_entry_point_on_raw_buffers(n, with_scale, momentum, wd):
    from hvpr_amd._lib import lib
    from hvpr_amd.kernels import _stream
    p, g, buf = _buffers(n, 200 + n, 3)
    before = [t.cpu().numpy().copy() for t in (p, g, buf)]
    scale = torch.tensor([0.37], device=DEV) if with_scale else None
    rc = lib().hvpr_fused_sgd_f32(p.data_ptr(), g.data_ptr(), buf.data_ptr() if momentum else None, n, 0.01, momentum, wd,
                                  None if scale is None else scale.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    wp, wb = _sgd_ref(before[0], before[1], before[2] if momentum else None, 0.01, momentum, wd, 0.37 if with_scale else 1.0)
    _check(p, wp, n, before[0], "sgd n=%d p" % n)
    if momentum:
        _check(buf, wb, n, before[2], "sgd n=%d buf" % n)
    else:
        assert buf.cpu().numpy().tobytes() == before[2].tobytes()
    assert g.cpu().numpy().tobytes() == before[1].tobytes()


def test_zeroed_momentum_buffer_gives_torchs_first_step():
    from hvpr_amd._lib import lib
    from hvpr_amd.kernels import _stream
    p, g, _ = _buffers(1027, 7, 3)
    buf = torch.zeros_like(p)
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    torch.optim.SGD([q], lr=0.01, momentum=0.9, weight_decay=0.0).step()
    assert lib().hvpr_fused_sgd_f32(p.data_ptr(), g.data_ptr(), buf.data_ptr(), 1027, 0.01, 0.9, 0.0, None, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:1027], g[:1027])                           # 0 * momentum + d == d
    np.testing.assert_allclose(p.cpu().numpy()[:1027], q.detach().cpu().numpy()[:1027], rtol=2e-5, atol=1e-7)


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from hvpr_amd._lib import lib
    from hvpr_amd.kernels import _stream
    L, s = lib(), _stream()
    n = 64
    bufs = _buffers(n, 3, 4)
    before = [t.clone() for t in bufs]
    p, g, m, v = (t.data_ptr() for t in bufs)
    good = dict(lr=0.003, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=1)

    def adam(p=p, g=g, m=m, v=v, n=n, **kw):
        a = dict(good, **kw)
        return L.hvpr_fused_adam_l2_f32(p, g, m, v, n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step"], None, s)

    def sgd(p=p, g=g, buf=m, n=n, momentum=0.9):
        return L.hvpr_fused_sgd_f32(p, g, buf, n, 0.01, momentum, 0.01, None, s)
    bad_adam = [dict(n=-1), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(p=p + 4), dict(g=g + 4), dict(m=m + 4),
                dict(v=v + 4), dict(step=0), dict(step=-3), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-0.1), dict(b1=float("nan"))]
    for kw in bad_adam:
        assert adam(**kw) == INVALID, kw
    bad_sgd = [dict(n=-1), dict(p=None), dict(g=None), dict(buf=None), dict(p=p + 4), dict(g=g + 4), dict(buf=m + 4), dict(momentum=1.0),
               dict(momentum=-0.1), dict(momentum=float("nan"))]
    for kw in bad_sgd:
        assert sgd(**kw) == INVALID, kw
    # n == 0 is fine, even with nothing to point at
    assert L.hvpr_fused_adam_l2_f32(None, None, None, None, 0, 0.003, 0.9, 0.999, 1e-8, 0.01, 1, None, s) == 0
    assert L.hvpr_fused_sgd_f32(None, None, None, 0, 0.01, 0.9, 0.01, None, s) == 0
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(t, b)                                       # nothing was launched
    assert adam() == 0 and sgd() == 0                                  # and the same calls without the fault go through
    torch.cuda.synchronize()
    assert not torch.equal(bufs[0], before[0])


# ------------------------------------------------------------------------------------------------ 4: the training driver
SET = ["OPTIMIZATION.OPTIMIZER", "sgd", "OPTIMIZATION.DECAY_STEP_LIST", "[1]"]
_RUNS = {}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import train_driver_cases as D
    return D.write_tree_with_infos(tmp_path_factory.mktemp("kitti"))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("runs")


class _Quiet:
    def info(self, s):
        pass


def _pieces(tree, set_cfgs):
    import train_driver_cases as D
    from hvpr_amd import config
    from hvpr_amd.detector import build_network
    from hvpr_amd.epoch_loader import build_dataloader
    cfg = D.model_cfg()
    if set_cfgs:
        config.cfg_from_list(list(set_cfgs), cfg)          # what `python -m hvpr_amd.train --set ...` applies
    ds, loader, sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, root_path=tree, training=True, seed=0, prefetch=False)
    torch.manual_seed(0)
    np.random.seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda()
    return cfg, loader, sampler, model, optim.build_optimizer(model, cfg.OPTIMIZATION)


def _train(tree, tmp, name, start_stop, resume=None):
    """As tests/test_gpu_train_driver.py's _train: everything built anew, epochs start_stop[0] .. start_stop[1] - 1 of two."""
    from hvpr_amd import train_loop
    if name in _RUNS:
        return _RUNS[name]
    cfg, loader, sampler, model, opt = _pieces(tree, SET)
    assert type(opt) is optim.FusedSGD
    it = start_epoch = 0
    if resume is not None:
        it, start_epoch = model.load_params_with_optimizer(resume, optimizer=opt)
    assert start_epoch == start_stop[0]
    model.train()
    sched, warm = optim.build_scheduler(opt, len(loader), 2, start_epoch + 1 if resume else -1, cfg.OPTIMIZATION)
    out = Path(tmp) / name
    out.mkdir(parents=True, exist_ok=True)
    n = train_loop.train_model(model, opt, loader, optim.model_fn_decorator(), sched, cfg.OPTIMIZATION, start_epoch, start_stop[1], int(it), 0,
                               out, _Quiet(), train_sampler=sampler, log_interval=1, scalars_path=out / "scalars.jsonl",
                               lr_warmup_scheduler=warm)
    torch.cuda.synchronize()
    _RUNS[name] = {"dir": out, "it": n, "cfg": cfg, "iters": len(loader)}
    return _RUNS[name]


def test_driver_with_sgd_logs_the_schedule(tree, tmp):
    run = _train(tree, tmp, "whole", (0, 2))
    o, iters = run["cfg"].OPTIMIZATION, run["iters"]
    assert run["it"] == 2 * iters == 6 and o.OPTIMIZER == "sgd" and o.DECAY_STEP_LIST == [1]
    rows = [json.loads(x) for x in open(run["dir"] / "scalars.jsonl")]
    assert [r["it"] for r in rows] == list(range(1, 7)) and all(np.isfinite(r["loss"]) for r in rows)
    # row `it` was trained at iteration it - 1: LR in epoch 0, LR * LR_DECAY from iteration 1 * iters on
    assert [r["lr"] for r in rows] == [o.LR * max(1, o.LR_CLIP / o.LR)] * iters + [o.LR * max(1 * o.LR_DECAY, o.LR_CLIP / o.LR)] * iters
    saved = torch.load(run["dir"] / "checkpoint_epoch_2.pth", map_location="cpu")
    group = saved["optimizer_state"]["param_groups"][0]
    assert group["initial_lr"] == o.LR and group["momentum"] == o.MOMENTUM and group["lr"] == rows[-1]["lr"]
    assert all(set(st) == {"momentum_buffer"} for st in saved["optimizer_state"]["state"].values())
    assert all(bool(torch.isfinite(v.double()).all()) for v in saved["model_state"].values())


def _flat(o, prefix=""):
    if torch.is_tensor(o):
        return {prefix: o}
    if isinstance(o, dict):
        return {k2: v2 for k, v in o.items() for k2, v2 in _flat(v, "%s.%s" % (prefix, k)).items()}
    if isinstance(o, (list, tuple)):
        return {k2: v2 for i, v in enumerate(o) for k2, v2 in _flat(v, "%s.%d" % (prefix, i)).items()}
    return {prefix: o}


def test_driver_resume_with_sgd_ends_on_the_same_checkpoint(tree, tmp):
    whole = _train(tree, tmp, "whole", (0, 2))
    half = _train(tree, tmp, "half", (0, 1))
    assert half["it"] == 3
    resumed = _train(tree, tmp, "resumed", (1, 2), resume=str(half["dir"] / "checkpoint_epoch_1.pth"))
    assert resumed["it"] == 6
    a = _flat(torch.load(whole["dir"] / "checkpoint_epoch_2.pth", map_location="cpu"))
    b = _flat(torch.load(resumed["dir"] / "checkpoint_epoch_2.pth", map_location="cpu"))
    assert sorted(a) == sorted(b) and len(a) > 100
    unequal = [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]
    assert not unequal, unequal[:10]
    rows = [json.loads(x) for x in open(resumed["dir"] / "scalars.jsonl")]
    assert [r["it"] for r in rows] == [4, 5, 6] and [r["lr"] for r in rows] == [json.loads(x)["lr"] for x in open(whole["dir"] / "scalars.jsonl")][3:]


def test_the_loop_synchronises_no_more_with_sgd_than_with_adam_onecycle(tree):
    """One quiet epoch (a single read at its end) under torch's sync debug mode, once per optimiser on the same batches."""
    import train_driver_cases as D
    from hvpr_amd import train_loop
    counts = {}
    for name, set_cfgs in (("adam_onecycle", None), ("sgd", SET), ("adam", ["OPTIMIZATION.OPTIMIZER", "adam"])):
        cfg, loader, sampler, model, opt = _pieces(tree, set_cfgs)
        sched, _ = optim.build_scheduler(opt, len(loader), 4, -1, cfg.OPTIMIZATION)
        fn = optim.model_fn_decorator()
        it, _ = train_loop.train_one_epoch(model, opt, loader, fn, sched, 0, cfg.OPTIMIZATION)        # lazy initialisation
        torch.cuda.synchronize()
        sampler.set_epoch(1)
        log = train_loop.ScalarLog(None, 1000)
        (it, _), counts[name] = D.sync_warnings(lambda: train_loop.train_one_epoch(model, opt, loader, fn, sched, it, cfg.OPTIMIZATION,
                                                                                   scalar_log=log))
        assert it == 6 and log.reads == 1
    assert counts["sgd"] <= counts["adam_onecycle"] and counts["adam"] <= counts["adam_onecycle"], counts
