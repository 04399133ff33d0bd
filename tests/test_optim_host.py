"""CPU: the 'adam' / 'sgd' branches of the training configuration against fixture G25 (the reference's own build_optimizer /
build_scheduler / CosineWarmupLR, tests/golden/make_golden_optim.py) — the schedules as Python floats, the per-tensor optimiser
forms, the dispatch, and the warm-up switch of train_model."""
import math

import numpy as np
import pytest
import torch

import optim_cases as C
from hvpr_amd import optim, train_loop


class _Opt:
    """What a schedule needs of an optimiser: param_groups."""

    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


def _lrs(sched, opt, n):
    out = []
    for it in range(n):
        sched.step(it)
        out.append(opt.param_groups[0]["lr"])
    return out


# ------------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_step_decay_equals_the_reference_as_floats(golden_dir, case):
    z = C.load(golden_dir)
    cfg = C.optim_cfg(**C.CASES[case])
    opt = _Opt(cfg.LR)
    sched, warm = optim.build_scheduler(opt, C.ITERS, C.EPOCHS, -1, cfg)
    assert warm is None and isinstance(sched, optim.StepDecayLR) and opt.param_groups[0]["initial_lr"] == cfg.LR
    got = _lrs(sched, opt, C.ITERS * C.EPOCHS)
    assert got == [float(v) for v in z[case + ".lr"]]
    # both sides of each boundary s * iters: the step before still has the old rate
    for s in cfg.DECAY_STEP_LIST:
        assert got[s * C.ITERS - 1] != got[s * C.ITERS] and got[s * C.ITERS - 1] == got[(s - 1) * C.ITERS]
    # a pure function of the iteration: out of order, and from a scheduler built for a resume
    again = optim.StepDecayLR(opt, [s * C.ITERS for s in cfg.DECAY_STEP_LIST], cfg.LR_DECAY, cfg.LR_CLIP, cfg.LR, last_epoch=2)
    for it in (11, 0, 4, 3, 8, 7):
        again.step(it)
        assert opt.param_groups[0]["lr"] == got[it]


def test_step_decay_of_the_issues_spot_check(golden_dir):
    """DECAY_STEP_LIST [2, 3] at 4 iterations an epoch: 3e-3 for iterations 0-7, 3e-4 for 8-11, 3e-5 for 12-15."""
    z = C.load(golden_dir)
    cfg = C.optim_cfg(**dict(C.CASES["a"], DECAY_STEP_LIST=[2, 3]))
    opt = _Opt(cfg.LR)
    sched, _ = optim.build_scheduler(opt, 4, 4, -1, cfg)
    got = _lrs(sched, opt, 16)
    assert got == [float(v) for v in z["decay23.lr"]]
    np.testing.assert_allclose(got, [3e-3] * 8 + [3e-4] * 4 + [3e-5] * 4, rtol=1e-12)
    assert got[7] == 3e-3 and got[8] != got[7] and got[11] != got[12]


def test_lr_clip_wins_over_a_small_decay():
    cfg = C.optim_cfg(**dict(C.CASES["a"], LR_DECAY=1e-3, LR_CLIP=1e-5))
    opt = _Opt(cfg.LR)
    sched, _ = optim.build_scheduler(opt, C.ITERS, C.EPOCHS, -1, cfg)
    got = _lrs(sched, opt, C.ITERS * C.EPOCHS)
    assert got[:4] == [0.003] * 4
    assert got[4:] == [0.003 * (1e-5 / 0.003)] * 8          # the reference's order: max(decay, LR_CLIP / LR), then * LR
    assert got[4] > 0.003 * 1e-3 > 0.003 * 1e-6              # one decay gives 3e-6, two 3e-9: both below the clip
    np.testing.assert_allclose(got[4:], 1e-5, rtol=1e-12)


def test_cosine_warmup_then_decay_equals_the_reference(golden_dir):
    z = C.load(golden_dir)
    cfg = C.optim_cfg(**dict(C.CASES["a"], LR_WARMUP=True))
    opt = _Opt(cfg.LR)
    sched, warm = optim.build_scheduler(opt, C.ITERS, C.EPOCHS, -1, cfg)
    assert isinstance(warm, optim.CosineWarmupLR) and warm.T_max == cfg.WARMUP_EPOCH * C.ITERS and warm.eta_min == cfg.LR / cfg.DIV_FACTOR
    got = []
    for it in range(C.ITERS * C.EPOCHS):
        (warm if it // C.ITERS < cfg.WARMUP_EPOCH else sched).step(it)
        got.append(opt.param_groups[0]["lr"])
    want = [float(v) for v in z["warmup.lr"]]
    np.testing.assert_allclose(got[:C.ITERS], want[:C.ITERS], rtol=1e-12)
    assert got[C.ITERS:] == want[C.ITERS:]
    eta = cfg.LR / cfg.DIV_FACTOR
    np.testing.assert_allclose(got[:C.ITERS], [eta + (cfg.LR - eta) * (1 - math.cos(math.pi * it / 4)) / 2 for it in range(4)], rtol=1e-12)
    assert got[0] == eta and got[0] < got[1] < got[2] < got[3] < cfg.LR


def test_build_scheduler_returns_a_warmup_scheduler_only_with_lr_warmup():
    for name in ("adam", "sgd"):
        for warmup in (False, True):
            cfg = C.optim_cfg(**dict(C.CASES["a"], OPTIMIZER=name, LR_WARMUP=warmup))
            sched, warm = optim.build_scheduler(_Opt(cfg.LR), 5, 3, -1, cfg)
            assert isinstance(sched, optim.StepDecayLR) and (warm is not None) == warmup

    class OneCycleOpt:
        lr = mom = 0.0
    cfg = C.optim_cfg(**dict(C.CASES["a"], OPTIMIZER="adam_onecycle", LR_WARMUP=True))
    sched, warm = optim.build_scheduler(OneCycleOpt(), 5, 3, -1, cfg)
    assert isinstance(sched, optim.OneCycle) and warm is None
    with pytest.raises(KeyError, match="initial_lr"):          # LambdaLR's rule on resume: the checkpoint's groups carry initial_lr
        optim.StepDecayLR(_Opt(0.1), [4], 0.1, 1e-7, 0.1, last_epoch=3)


# ------------------------------------------------------------------------------------------------ optimisers
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_per_tensor_forms_reproduce_fixture_g25(golden_dir, case):
    want = torch.optim.Adam if C.CASES[case]["OPTIMIZER"] == "adam" else torch.optim.SGD
    opt = C.run_case(golden_dir, case, "cpu", 2e-5, want, FUSED=False)
    g = opt.param_groups[0]
    assert len(opt.param_groups) == 1 and g["weight_decay"] == C.CASES[case]["WEIGHT_DECAY"] and g["initial_lr"] == C.CASES[case]["LR"]
    if want is torch.optim.SGD:
        assert g["momentum"] == C.CASES[case]["MOMENTUM"] and g["dampening"] == 0 and not g["nesterov"]
    else:
        assert tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8


def test_build_optimizer_dispatch():
    net = C.network()
    with pytest.raises(NotImplementedError):
        optim.build_optimizer(net, C.optim_cfg(**dict(C.CASES["a"], OPTIMIZER="rmsprop")))
    assert type(optim.build_optimizer(net, C.optim_cfg(**C.CASES["a"]))) is torch.optim.Adam          # a CPU model: per-tensor
    assert type(optim.build_optimizer(net, C.optim_cfg(**C.CASES["b"]))) is torch.optim.SGD
    assert type(optim.build_optimizer(net, C.optim_cfg(**dict(C.CASES["a"], OPTIMIZER="adam_onecycle")))) is optim.AdamOneCycle


def test_flat_forms_keep_torch_indices_groups_and_state_format():
    """The flat machinery needs no GPU up to the launch: one group in model.parameters() order, a frozen parameter keeps its
    index and has no state, the state dicts load into torch.optim and back."""
    for cls, ref_cls, kw, keys in ((optim.FusedAdam, torch.optim.Adam, dict(lr=0.003, weight_decay=0.01), {"step", "exp_avg", "exp_avg_sq"}),
                                   (optim.FusedSGD, torch.optim.SGD, dict(lr=0.01, weight_decay=0.01, momentum=0.9), {"momentum_buffer"})):
        net = C.network()
        net[1].bias.requires_grad_(False)                       # index 2 of 5
        ref_net = C.network()
        ref_net[1].bias.requires_grad_(False)
        opt, ref = cls(net, **kw), ref_cls(ref_net.parameters(), **kw)
        assert opt.index == [0, 1, 3, 4] and len(opt.params) == 4 and len(opt.param_groups) == 1
        assert [p.data_ptr() % 16 for p in opt.params] == [0] * 4 and opt.numel == 136 + 8 + 136 + 4
        assert float(opt.lr) == kw["lr"]
        opt.lr = 0.5
        assert opt.param_groups[0]["lr"] == 0.5
        opt.lr = kw["lr"]
        assert opt.state_dict()["state"] == {}                  # no step yet
        theirs, ours = ref.state_dict()["param_groups"][0], opt.state_dict()["param_groups"][0]
        assert set(theirs) == set(ours) and ours["params"] == theirs["params"] == [0, 1, 2, 3, 4]
        assert all(ours[k] == theirs[k] for k in theirs), (ours, theirs)
        # a stepped torch optimiser -> flat -> torch
        ref_net(torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(1))).pow(2).mean().backward()
        ref.step()
        opt.load_state_dict(ref.state_dict())
        assert opt.steps == 1
        back = opt.state_dict()
        assert sorted(back["state"]) == [0, 1, 3, 4] and all(set(st) == keys for st in back["state"].values())
        for i, st in ref.state_dict()["state"].items():
            for k, v in st.items():
                assert torch.equal(torch.as_tensor(back["state"][i][k]).float(), torch.as_tensor(v).float()), (i, k)
        fresh = ref_cls(C.network().parameters(), **kw)
        fresh.load_state_dict(back)
        assert sorted(fresh.state_dict()["state"]) == [0, 1, 3, 4]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step()
    plain = optim.FusedSGD(C.network(), lr=0.01, momentum=0.0)
    assert plain.momentum_buffer is None and plain.state_dict()["state"] == {}


# ------------------------------------------------------------------------------------------------ the loop
class _Counting:
    def __init__(self):
        self.its = []

    def step(self, it):
        self.its.append(it)


class _Logger:
    def info(self, s):
        pass


def test_train_model_steps_the_warmup_scheduler_before_warmup_epoch(tmp_path):
    net = torch.nn.Linear(3, 2)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    loader = [torch.randn(4, 3) for _ in range(3)]

    def model_func(model, batch):
        return model(batch).pow(2).mean(), {}, {}, None
    for warmup_epoch, with_warm in ((2, True), (1, True), (0, True), (2, False)):
        main, warm = _Counting(), _Counting()
        cfg = C.optim_cfg(**dict(C.CASES["b"], WARMUP_EPOCH=warmup_epoch))
        kw = dict(lr_warmup_scheduler=warm) if with_warm else {}
        n = train_loop.train_model(net, opt, loader, model_func, main, cfg, 0, 3, 0, 0, tmp_path, _Logger(), **kw)
        assert n == 9
        cut = 3 * warmup_epoch if with_warm else 0
        assert warm.its == list(range(cut)) and main.its == list(range(cut, 9)), (warmup_epoch, with_warm, warm.its, main.its)
    # a resume inside the warm-up: epoch 1 of 3, WARMUP_EPOCH 2
    main, warm = _Counting(), _Counting()
    train_loop.train_model(net, opt, loader, model_func, main, C.optim_cfg(**dict(C.CASES["b"], WARMUP_EPOCH=2)), 1, 3, 3, 0, tmp_path,
                           _Logger(), lr_warmup_scheduler=warm)
    assert warm.its == [3, 4, 5] and main.its == [6, 7, 8]
