"""Fixture G25 (tests/golden/g25_optim.npz): the reference's 'adam' and 'sgd' optimisers with step decay, and its CosineWarmupLR.

Runs ONLY in the build container (needs /root/reference; CPU torch), like make_golden.py, whose in-memory loader it uses: the
reference's tools/train_utils/optimization package is imported as `tools_opt` and its own build_optimizer / build_scheduler are
driven in train_one_epoch's order (tools/train_utils/train_utils.py:25-42): scheduler.step(it), zero_grad, backward,
clip_grad_norm_, step.  Only arrays and key names are written.

The network: Conv2d(3, 5, 3, stride=2, bias=False) -> BatchNorm2d(5) -> ReLU -> Flatten -> Linear(5 * 3 * 3, 3) on 8 x 8 inputs;
loss = w[it] * mean(out ** 2).  Parameter sizes 135, 5, 5, 135, 3: none is a multiple of 4, so every view of the flat buffer is padded.

Cases, 3 epochs x 4 iterations each, DECAY_STEP_LIST [1, 2], LR_DECAY 0.1, GRAD_NORM_CLIP 1.0 (the loss weight w alternates
between 0.3 and 3 so that some steps are clipped and some are not; `<case>.norm` records the norm of every step):
  a  adam, LR 0.003, WEIGHT_DECAY 0.01        b  sgd, LR 0.01, MOMENTUM 0.9, WEIGHT_DECAY 0.01
  c  sgd, MOMENTUM 0                            d  adam, WEIGHT_DECAY 0
Keys: x (12, 4, 3, 8, 8); w (12); init.<param>; <case>.lr (12); <case>.norm (12); <case>.clipped (12); <case>.after<step>.<param> and
<case>.after<step>.<state key>.<param index> for step in 1, 2, 6, 12; warmup.lr (12): CosineWarmupLR(T_max = 1 * 4) over epoch 0,
then the step decay — build_scheduler itself raises TypeError with LR_WARMUP (its T_max takes len() of an int), so the class is
built directly with the T_max the product uses.

Usage:  python tests/golden/make_golden_optim.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402

ITERS, EPOCHS, CLIP = 4, 3, 1.0
RECORD = (1, 2, 6, 12)
CASES = {"a": dict(OPTIMIZER="adam", LR=0.003, WEIGHT_DECAY=0.01, MOMENTUM=0.9),
         "b": dict(OPTIMIZER="sgd", LR=0.01, WEIGHT_DECAY=0.01, MOMENTUM=0.9),
         "c": dict(OPTIMIZER="sgd", LR=0.01, WEIGHT_DECAY=0.01, MOMENTUM=0.0),
         "d": dict(OPTIMIZER="adam", LR=0.003, WEIGHT_DECAY=0.0, MOMENTUM=0.9)}


def load_optimization():
    import collections
    import collections.abc
    collections.Iterable = collections.abc.Iterable           # fastai_optim.py:3 predates python 3.10
    pkg = types.ModuleType("tools_opt")
    pkg.__path__ = [os.path.join(G.REF, "tools/train_utils/optimization")]
    sys.modules["tools_opt"] = pkg
    G._load("tools_opt.fastai_optim", "tools/train_utils/optimization/fastai_optim.py")
    G._load("tools_opt.learning_schedules_fastai", "tools/train_utils/optimization/learning_schedules_fastai.py")
    src = open(os.path.join(G.REF, "tools/train_utils/optimization/__init__.py")).read()
    pkg.__file__ = os.path.join(G.REF, "tools/train_utils/optimization/__init__.py")
    pkg.__package__ = "tools_opt"
    exec(compile(src, pkg.__file__, "exec"), pkg.__dict__)
    return pkg


def network():
    torch.manual_seed(2501)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, stride=2, bias=False), torch.nn.BatchNorm2d(5), torch.nn.ReLU(),
                               torch.nn.Flatten(), torch.nn.Linear(5 * 3 * 3, 3))


def optim_cfg(**kw):
    return G.EasyDict(dict(dict(DECAY_STEP_LIST=[1, 2], LR_DECAY=0.1, LR_CLIP=1e-7, LR_WARMUP=False, WARMUP_EPOCH=1, DIV_FACTOR=10,
                                MOMS=[0.95, 0.85], PCT_START=0.4, GRAD_NORM_CLIP=CLIP), **kw))


def snapshot(net, opt):
    out = {k: v.detach().clone().numpy() for k, v in net.state_dict().items() if "num_batches" not in k}
    for i, st in opt.state_dict()["state"].items():
        for k, v in st.items():
            if v is not None:
                out["%s.%d" % (k, i)] = np.asarray(v.detach().clone().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
    return out


def main():
    opt_pkg = load_optimization()
    gen = torch.Generator().manual_seed(2502)
    xs = torch.randn(ITERS * EPOCHS, 4, 3, 8, 8, generator=gen)
    ws = torch.tensor([0.3, 3.0, 3.0, 0.3, 3.0, 0.3, 0.3, 3.0, 0.3, 3.0, 0.3, 3.0])
    out = {"x": xs.numpy(), "w": ws.numpy()}
    out.update({"init." + k: v.detach().clone().numpy() for k, v in network().state_dict().items() if "num_batches" not in k})
    for name, kw in CASES.items():
        cfg = optim_cfg(**kw)
        net = network()
        opt = opt_pkg.build_optimizer(net, cfg)
        sched, warm = opt_pkg.build_scheduler(opt, total_iters_each_epoch=ITERS, total_epochs=EPOCHS, last_epoch=-1, optim_cfg=cfg)
        assert warm is None and isinstance(opt, torch.optim.Optimizer)
        lrs, norms = [], []
        for it in range(ITERS * EPOCHS):
            sched.step(it)
            lrs.append(opt.param_groups[0]["lr"])
            net.train()
            opt.zero_grad()
            (net(xs[it]).pow(2).mean() * ws[it]).backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(net.parameters(), cfg.GRAD_NORM_CLIP)))
            opt.step()
            if it + 1 in RECORD:
                out.update({"%s.after%d.%s" % (name, it + 1, k): v for k, v in snapshot(net, opt).items()})
        clipped = np.array(norms) > CLIP
        assert clipped.any() and not clipped.all() and not any(abs(n - CLIP) < 0.05 * CLIP for n in norms), norms
        out[name + ".lr"], out[name + ".norm"], out[name + ".clipped"] = np.array(lrs, np.float64), np.array(norms, np.float64), clipped
        print("g25", name, "lr", lrs, "clipped", clipped.astype(int).tolist())
    # warm-up: the reference's CosineWarmupLR over epoch 0, its LambdaLR afterwards, switched as train_model does (:82-85)
    cfg = optim_cfg(**CASES["a"])
    try:
        opt_pkg.build_scheduler(opt_pkg.build_optimizer(network(), cfg), ITERS, EPOCHS, -1, optim_cfg(LR_WARMUP=True, **CASES["a"]))
        raise SystemExit("the reference's LR_WARMUP branch ran: the T_max deviation no longer holds")
    except TypeError as e:
        print("g25 LR_WARMUP in the reference:", repr(e))
    opt = opt_pkg.build_optimizer(network(), cfg)
    sched, _ = opt_pkg.build_scheduler(opt, ITERS, EPOCHS, -1, cfg)
    warm = opt_pkg.CosineWarmupLR(opt, T_max=cfg.WARMUP_EPOCH * ITERS, eta_min=cfg.LR / cfg.DIV_FACTOR)
    lrs = []
    for it in range(ITERS * EPOCHS):
        (warm if it // ITERS < cfg.WARMUP_EPOCH else sched).step(it)
        lrs.append(opt.param_groups[0]["lr"])
    out["warmup.lr"] = np.array(lrs, np.float64)
    print("g25 warmup lr", lrs)
    # the issue's spot check of the step decay: DECAY_STEP_LIST [2, 3], 4 iterations per epoch
    cfg = optim_cfg(**dict(CASES["a"], DECAY_STEP_LIST=[2, 3]))
    opt = opt_pkg.build_optimizer(network(), cfg)
    sched, _ = opt_pkg.build_scheduler(opt, 4, 4, -1, cfg)
    lrs = []
    for it in range(16):
        sched.step(it)
        lrs.append(opt.param_groups[0]["lr"])
    out["decay23.lr"] = np.array(lrs, np.float64)
    path = os.path.join(G.OUT, "g25_optim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
