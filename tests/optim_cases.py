"""Fixture G25 (tests/golden/make_golden_optim.py: the reference's 'adam' / 'sgd' optimisers under step decay) replayed through this
package's build_optimizer / build_scheduler: shared by the host tests (per-tensor torch.optim forms) and the GPU tests (fused flat
forms)."""
import os

import numpy as np
import torch

from hvpr_amd import optim
from hvpr_amd.config import AttrDict

ITERS, EPOCHS, CLIP = 4, 3, 1.0
RECORD = (1, 2, 6, 12)
CASES = {"a": dict(OPTIMIZER="adam", LR=0.003, WEIGHT_DECAY=0.01, MOMENTUM=0.9),
         "b": dict(OPTIMIZER="sgd", LR=0.01, WEIGHT_DECAY=0.01, MOMENTUM=0.9),
         "c": dict(OPTIMIZER="sgd", LR=0.01, WEIGHT_DECAY=0.01, MOMENTUM=0.0),
         "d": dict(OPTIMIZER="adam", LR=0.003, WEIGHT_DECAY=0.0, MOMENTUM=0.9)}
_Z = {}


def load(golden_dir):
    if golden_dir not in _Z:
        with np.load(os.path.join(golden_dir, "g25_optim.npz")) as z:
            _Z[golden_dir] = {k: z[k] for k in z.files}
    return _Z[golden_dir]


def optim_cfg(**kw):
    return AttrDict(dict(dict(DECAY_STEP_LIST=[1, 2], LR_DECAY=0.1, LR_CLIP=1e-7, LR_WARMUP=False, WARMUP_EPOCH=1, DIV_FACTOR=10,
                              MOMS=[0.95, 0.85], PCT_START=0.4, GRAD_NORM_CLIP=CLIP), **kw))


def network(z=None):
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, stride=2, bias=False), torch.nn.BatchNorm2d(5), torch.nn.ReLU(),
                              torch.nn.Flatten(), torch.nn.Linear(5 * 3 * 3, 3))
    if z is not None:
        net.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z if k.startswith("init.")}, strict=False)
    return net


def clipped_step(net, opt, loss, clip):
    """zero_grad was called before the forward pass; backward, clip, step (train_utils.py:40-42).  Returns the norm."""
    loss.backward()
    if hasattr(opt, "clip_grad_norm"):
        norm = opt.clip_grad_norm(clip)
    else:
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
    opt.step()
    return norm


def run_case(golden_dir, case, dev, rtol, expect_type, **cfg_kw):
    """Case `case` of G25 through build_optimizer / build_scheduler: lr equal as floats at every iteration, gradient norms,
    parameters and optimiser state at steps 1, 2, 6 and 12 within rtol (atol 1e-7, as run_g9)."""
    z = load(golden_dir)
    cfg = optim_cfg(**dict(CASES[case], **cfg_kw))
    net = network(z).to(dev)
    opt = optim.build_optimizer(net, cfg)
    assert type(opt) is expect_type, type(opt)
    sched, warm = optim.build_scheduler(opt, ITERS, EPOCHS, -1, cfg)
    assert warm is None
    xs, ws = torch.from_numpy(z["x"]).to(dev), torch.from_numpy(z["w"]).to(dev)
    seen = 0
    for it in range(ITERS * EPOCHS):
        sched.step(it)
        lr = float(opt.lr) if hasattr(opt, "lr") else opt.param_groups[0]["lr"]
        assert lr == float(z[case + ".lr"][it]), (it, lr)
        net.train()
        opt.zero_grad()
        norm = clipped_step(net, opt, net(xs[it]).pow(2).mean() * ws[it], cfg.GRAD_NORM_CLIP)
        np.testing.assert_allclose(float(norm), z[case + ".norm"][it], rtol=max(rtol, 1e-4))
        assert bool(float(norm) > CLIP) == bool(z[case + ".clipped"][it])
        if it + 1 not in RECORD:
            continue
        pre = "%s.after%d." % (case, it + 1)
        for k, v in net.state_dict().items():
            if "num_batches" not in k:
                np.testing.assert_allclose(v.detach().cpu().numpy(), z[pre + k], rtol=rtol, atol=1e-7, err_msg=pre + k)
        state = opt.state_dict()["state"]
        want = {k[len(pre):] for k in z if k.startswith(pre) and k[len(pre):].split(".")[0] in ("step", "exp_avg", "exp_avg_sq", "momentum_buffer")}
        got = {"%s.%d" % (k, i) for i, st in state.items() for k, v in st.items() if v is not None}
        assert got == want, (pre, sorted(got ^ want))
        for i, st in state.items():
            for k, v in st.items():
                if v is not None:
                    np.testing.assert_allclose(np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32),
                                               z["%s%s.%d" % (pre, k, i)], rtol=rtol, atol=1e-7, err_msg="%s%s.%d" % (pre, k, i))
        seen += 1
    assert seen == len(RECORD)
    assert z[case + ".clipped"].any() and not z[case + ".clipped"].all()
    return opt
