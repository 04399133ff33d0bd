"""Optimiser step of the training path: Adam with one-cycle lr / momentum and TRUE weight decay.

Restates build_optimizer 'adam_onecycle' (tools/train_utils/optimization/__init__.py:19-32), OptimWrapper.step
(fastai_optim.py:132-149: p *= 1 - wd*lr for every group, BatchNorm included, the optimiser's own weight_decay forced to 0),
OneCycle (learning_schedules_fastai.py:60-77) with cosine annealing (:53-57), and the clipped step of train_one_epoch
(tools/train_utils/train_utils.py:35-42).  Parameter updates use torch's foreach/fused kernels instead of the reference's
per-tensor python loops.

The other two branches of build_optimizer / build_scheduler (__init__.py:12-18, 40-61) are here as well: 'adam' and 'sgd' as
torch.optim.Adam / SGD or, on the GPU, their flat forms FusedAdam / FusedSGD, with step decay (StepDecayLR, the reference's
LambdaLR) and the cosine warm-up (CosineWarmupLR)."""
import math

import torch
import torch.nn as nn


def annealing_cos(start, end, pct):
    return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)


class OneCycle:
    """lr: low -> max over the first pct_start of the steps, then max -> low/1e4; momentum: moms[0] -> moms[1] -> moms[0]."""

    def __init__(self, optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.optimizer, self.total_step = optimizer, total_step
        low = lr_max / div_factor
        bounds = [0, int(pct_start * total_step), total_step]
        self.lr_phases = [(bounds[0], bounds[1], low, lr_max), (bounds[1], bounds[2], lr_max, low / 1e4)]
        self.mom_phases = [(bounds[0], bounds[1], moms[0], moms[1]), (bounds[1], bounds[2], moms[1], moms[0])]
        optimizer.lr, optimizer.mom = low, moms[0]

    def step(self, step):
        for start, end, a, b in self.lr_phases:
            if step >= start:
                self.optimizer.lr = annealing_cos(a, b, (step - start) / (end - start))
        for start, end, a, b in self.mom_phases:
            if step >= start:
                self.optimizer.mom = annealing_cos(a, b, (step - start) / (end - start))


def split_bn_params(model):
    """(non-BatchNorm, BatchNorm) trainable parameters in the order the reference's flattened leaf-module list gives them
    (tools/train_utils/optimization/__init__.py:26-27, fastai_optim.py:13-24)."""
    bn_types = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)
    bn, rest = [], []
    for m in model.modules():
        if next(m.children(), None) is not None:
            continue            # leaves only (the reference flattens the model into leaf modules, __init__.py:26-27)
        for p in m.parameters(recurse=False):
            if p.requires_grad:
                (bn if isinstance(m, bn_types) else rest).append(p)
    owned = {id(p) for p in bn + rest}
    rest += [p for p in model.parameters() if p.requires_grad and id(p) not in owned]   # parameters held by non-leaf modules
    return rest, bn


class AdamOneCycle:
    """Adam(betas=(mom, 0.99)) over two parameter groups (non-BatchNorm / BatchNorm), decoupled weight decay on both."""

    def __init__(self, model, wd, lr=3e-3, beta2=0.99):
        rest, bn = split_bn_params(model)
        self.opt = torch.optim.Adam([{"params": rest}, {"params": bn}], lr=lr, betas=(0.9, beta2), weight_decay=0.0)
        self.wd, self._lr, self._mom, self.beta2 = wd, lr, 0.9, beta2

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, v):
        self._lr = float(v)
        for g in self.opt.param_groups:
            g["lr"] = self._lr

    @property
    def mom(self):
        return self._mom

    @mom.setter
    def mom(self, v):
        self._mom = float(v)
        for g in self.opt.param_groups:
            g["betas"] = (self._mom, self.beta2)

    @property
    def param_groups(self):
        return self.opt.param_groups

    def zero_grad(self):
        self.opt.zero_grad(set_to_none=True)

    @torch.no_grad()
    def step(self):
        for g in self.opt.param_groups:          # true weight decay first, on every trainable tensor, BN included
            ps = [p for p in g["params"] if p.requires_grad]
            if ps:
                torch._foreach_mul_(ps, 1.0 - self.wd * self._lr)
        self.opt.step()

    def state_dict(self):
        """Inner Adam state (step counters + both moments per parameter) plus the wrapper's own scalars, so that a resumed
        run continues with the same lr / momentum until the scheduler's next step."""
        sd = self.opt.state_dict()
        sd["hvpr_onecycle"] = {"lr": self._lr, "mom": self._mom, "wd": self.wd, "beta2": self.beta2}
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        extra = sd.pop("hvpr_onecycle", None)
        self.opt.load_state_dict(sd)
        if extra is not None:
            self.wd, self.beta2 = float(extra["wd"]), float(extra["beta2"])
            self.lr, self.mom = extra["lr"], extra["mom"]


class _FlatOptimizer:
    """What the flat optimisers share: every parameter of `params` becomes a view into ONE fp32 buffer `flat_p`, its gradient a
    view into `flat_g`; zero_grad / _collect_grads keep the gradient addresses fixed, clip_grad_norm leaves the coefficient on the
    device, and step() is one launch (`_launch`, the subclass's kernel) over the whole buffer."""

    def _flatten(self, params):
        from . import kernels
        name = type(self).__name__
        self.params = list(params)
        assert self.params and all(p.dtype == torch.float32 for p in self.params), name + ": fp32 parameters"
        assert len({p.device for p in self.params}) == 1, name + ": one device"
        dev = self.params[0].device
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4                     # every view starts 16-byte aligned
        self.numel = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat_p[o:o + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
        self._grad_views = [self.flat_g[o:o + p.numel()].view_as(p) for p, o in zip(self.params, self.offsets)]
        self._point_grads()
        from . import conv_train
        conv_train.weights_changed()        # every parameter has just moved into the flat buffer
        self.steps = 0
        self._scale = None
        self._kernels = kernels

    def _point_grads(self):
        for p, g in zip(self.params, self._grad_views):
            p.grad = g

    def _views(self, flat):
        """The per-parameter views of a flat state buffer, in `params` order."""
        return [flat[o:o + p.numel()].view_as(p) for p, o in zip(self.params, self.offsets)]

    def zero_grad(self):
        """Gradients are zeroed, never set to None: autograd then accumulates in place into the flat views, and p.grad keeps its
        address from step to step.  distributed.wrap_ddp builds DistributedDataParallel with gradient_as_bucket_view=False (torch's
        default, what the reference's train.py gets): DDP copies each reduced bucket back into the EXISTING p.grad tensors, i.e.
        into the flat buffer — one extra device copy of the gradient set (~62 MB, ~25 us at HBM speed) per step in exchange for
        addresses that never move.  The other mode (gradient_as_bucket_view=True: DDP owns p.grad, a view into its all-reduce
        bucket) is still handled — such a gradient is zeroed where it lives instead of being re-pointed (re-pointing made DDP
        copy the whole gradient set into its buckets and re-point back every step) and _collect_grads copies the reduced values
        in — and covered by tests/test_distributed_gloo.py in both modes; it saves nothing measurable here (the copy it avoids is
        replaced by the copy into the flat buffer)."""
        self.flat_g.zero_()
        for p, g in zip(self.params, self._grad_views):
            if p.grad is None:
                p.grad = g
            elif p.grad.data_ptr() != g.data_ptr():
                p.grad.zero_()
        self._scale = None

    @torch.no_grad()
    def _collect_grads(self):
        """Gradients normally accumulate straight into the flat buffer (also under DDP's default gradient_as_bucket_view=False,
        which copies the reduced bucket back into the existing p.grad); a gradient that lives elsewhere (DDP bucket views) is
        copied in."""
        for p, g in zip(self.params, self._grad_views):
            if p.grad is None:
                g.zero_()
            elif p.grad.data_ptr() != g.data_ptr():
                g.copy_(p.grad)

    @torch.no_grad()
    def clip_grad_norm(self, max_norm):
        """clip_grad_norm_ (train_utils.py:41) without touching the gradients: the coefficient stays on the device and the step
        kernel applies it.  Returns the total norm (device scalar)."""
        self._collect_grads()
        total = torch.linalg.vector_norm(self.flat_g)
        self._scale = torch.clamp(max_norm / (total + 1e-6), max=1.0).to(torch.float32).reshape(1)
        return total

    @torch.no_grad()
    def step(self):
        if self._scale is None:
            self._collect_grads()
        self.steps += 1
        self._launch()
        self._scale = None

    def _call(self, name, *args):
        """ONE launch of the step kernel `name` over the flat buffers: (params, grads, *args, grad scale, stream)."""
        from ._lib import call
        call(name, self.flat_p, self.flat_g, *args, self._scale, self._kernels._stream())
        # the kernel writes the parameters through a raw pointer: torch's version counters do not see it, so whatever is derived from
        # the weights and cached by version (conv_train's packed Winograd filters) is told here
        from . import conv_train
        conv_train.weights_changed()


class FusedAdamOneCycle(_FlatOptimizer):
    """The same optimiser as AdamOneCycle on ONE flat fp32 buffer: every trainable parameter becomes a view into `flat_p`, its
    gradient a view into `flat_g`, and a step is one launch of hvpr_fused_adam_truewd_f32 (decay + Adam + the gradient-norm
    clip as a device-side scale) instead of hundreds of small kernels per tensor (the reference: per-tensor python loops,
    fastai_optim.py:132-149).  state_dict() / load_state_dict() speak torch.optim.Adam's format in AdamOneCycle's parameter
    order, so checkpoints move between the two."""

    def __init__(self, model, wd, lr=3e-3, beta2=0.99, eps=1e-8):
        rest, bn = split_bn_params(model)
        self.n_rest = len(rest)
        self._flatten(rest + bn)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat_p), torch.zeros_like(self.flat_p)
        self.wd, self._lr, self._mom, self.beta2, self.eps = wd, lr, 0.9, beta2, eps

    lr = property(lambda self: self._lr, lambda self, v: setattr(self, "_lr", float(v)))
    mom = property(lambda self: self._mom, lambda self, v: setattr(self, "_mom", float(v)))

    @property
    def param_groups(self):
        return [{"params": self.params[:self.n_rest], "lr": self._lr, "betas": (self._mom, self.beta2)},
                {"params": self.params[self.n_rest:], "lr": self._lr, "betas": (self._mom, self.beta2)}]

    def _launch(self):
        """ONE launch of hvpr_fused_adam_truewd_f32 over the flat buffers."""
        self._call("hvpr_fused_adam_truewd_f32", self.exp_avg, self.exp_avg_sq, self.numel, self._lr, self._mom,
                   self.beta2, self.eps, self.wd, self.steps)

    def state_dict(self):
        state = {}
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            if self.steps > 0:
                state[i] = {"step": torch.tensor(float(self.steps)), "exp_avg": self.exp_avg[o:o + p.numel()].view_as(p).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + p.numel()].view_as(p).clone()}
        base = {"lr": self._lr, "betas": (self._mom, self.beta2), "eps": self.eps, "weight_decay": 0.0, "amsgrad": False,
                "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                "decoupled_weight_decay": False}
        groups = [dict(base, params=list(range(self.n_rest))), dict(base, params=list(range(self.n_rest, len(self.params))))]
        return {"state": state, "param_groups": groups,
                "hvpr_onecycle": {"lr": self._lr, "mom": self._mom, "wd": self.wd, "beta2": self.beta2}}

    def load_state_dict(self, sd):
        with torch.no_grad():
            steps = 0
            for i, st in sd["state"].items():
                i = int(i)
                p, o = self.params[i], self.offsets[i]
                self.exp_avg[o:o + p.numel()].view_as(p).copy_(st["exp_avg"])
                self.exp_avg_sq[o:o + p.numel()].view_as(p).copy_(st["exp_avg_sq"])
                steps = max(steps, int(float(st["step"])))
            self.steps = steps
        extra = sd.get("hvpr_onecycle")
        if extra is not None:
            self.wd, self.beta2, self._lr, self._mom = float(extra["wd"]), float(extra["beta2"]), float(extra["lr"]), float(extra["mom"])


class _FlatTorchOptimizer(_FlatOptimizer):
    """The flat form of a plain torch optimiser over `model.parameters()` (tools/train_utils/optimization/__init__.py:12-18): ONE
    parameter group in that order, no BatchNorm split.  State indices count EVERY parameter, as torch's do: one with
    requires_grad=False keeps its index, is not in the flat buffer and has no state.  `param_groups` is one dict with torch's keys
    (a schedule writes `lr` and `initial_lr` into it), `lr` reads and writes it — the loop's `float(optimizer.lr)`
    (train_utils.py:28) works.  state_dict() / load_state_dict() speak the torch optimiser's own format, so checkpoints move
    between this class, the per-tensor form and the reference; one step counter serves the whole buffer.

    An ABSENT gradient is a ZERO gradient (FusedAdamOneCycle's convention): a trainable parameter that took no part in the
    backward pass is still stepped — decay and momentum act on it — where torch skips it and gives it no state."""
    _STATE = ()                          # (state-dict key, attribute holding the flat buffer)

    def __init__(self, model, defaults):
        every = list(model.parameters())
        self.index = [i for i, p in enumerate(every) if p.requires_grad]          # state-dict index of each flat parameter
        self._flatten([every[i] for i in self.index])
        self.param_groups = [dict(defaults, params=every)]

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.param_groups[0]["lr"] = float(v)

    def _has_state(self):
        return self.steps > 0

    def state_dict(self):
        state = {}
        if self._has_state():
            bufs = [(k, self._views(getattr(self, a))) for k, a in self._STATE]
            for j, i in enumerate(self.index):
                state[i] = {"step": torch.tensor(float(self.steps))} if self._STEP else {}
                state[i].update((k, v[j].clone()) for k, v in bufs)
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.param_groups[0]["params"])))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.param_groups[0]["params"]):
            raise ValueError("%s: the state dict holds %d group(s) of %s parameters, this optimiser one of %d" % (
                type(self).__name__, len(groups), [len(g["params"]) for g in groups], len(self.param_groups[0]["params"])))
        slot = {i: j for j, i in enumerate(self.index)}
        with torch.no_grad():
            bufs = [(k, getattr(self, a), self._views(getattr(self, a))) for k, a in self._STATE]
            for _, flat, _ in bufs:
                flat.zero_()
            steps = 0
            for i, st in sd["state"].items():
                j = slot.get(int(i))
                if j is None:
                    continue
                for k, _, views in bufs:
                    if st.get(k) is not None:
                        views[j].copy_(st[k])
                        steps = max(steps, 1)
                if "step" in st:
                    steps = max(steps, int(float(st["step"])))
            self.steps = steps
        self.param_groups[0].update({k: v for k, v in groups[0].items() if k != "params"})


_TORCH_GROUP = {"maximize": False, "foreach": None, "differentiable": False, "fused": None}


class FusedAdam(_FlatTorchOptimizer):
    """torch.optim.Adam(model.parameters(), lr, weight_decay) — build_optimizer's 'adam', coupled (L2) decay — as one launch of
    hvpr_fused_adam_l2_f32 per step.  State per index: {"step", "exp_avg", "exp_avg_sq"}."""
    _STATE, _STEP = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq")), True

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(model, dict(_TORCH_GROUP, lr=float(lr), betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                     capturable=False, decoupled_weight_decay=False))
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat_p), torch.zeros_like(self.flat_p)

    def _launch(self):
        g = self.param_groups[0]
        self._call("hvpr_fused_adam_l2_f32", self.exp_avg, self.exp_avg_sq, self.numel, g["lr"], g["betas"][0],
                   g["betas"][1], g["eps"], g["weight_decay"], self.steps)


class FusedSGD(_FlatTorchOptimizer):
    """torch.optim.SGD(model.parameters(), lr, momentum, weight_decay) — build_optimizer's 'sgd', dampening 0, no Nesterov — as one
    launch of hvpr_fused_sgd_f32 per step.  State per index: {"momentum_buffer"}; none at momentum 0.  The buffer starts zeroed,
    which reproduces torch's first step (buf = d) with no step counter."""
    _STEP = False

    def __init__(self, model, lr=1e-3, momentum=0.0, weight_decay=0.0):
        super().__init__(model, dict(_TORCH_GROUP, lr=float(lr), momentum=momentum, dampening=0, weight_decay=weight_decay,
                                     nesterov=False))
        self.momentum_buffer = torch.zeros_like(self.flat_p) if momentum != 0 else None
        self._STATE = (("momentum_buffer", "momentum_buffer"),) if momentum != 0 else ()

    def _has_state(self):
        return self.steps > 0 and self.momentum_buffer is not None

    def _launch(self):
        g = self.param_groups[0]
        if (g["momentum"] != 0) != (self.momentum_buffer is not None):
            raise ValueError("FusedSGD: momentum changed between zero and non-zero after construction")
        self._call("hvpr_fused_sgd_f32", self.momentum_buffer, self.numel, g["lr"],
                   g["momentum"], g["weight_decay"])


class _IterationSchedule:
    """A learning rate that is a pure function of the iteration: step(it) writes lr(it) into every parameter group, so a resumed
    run gets what the uninterrupted one got.  Own classes, since torch's schedulers refuse an object that is not a
    torch.optim.Optimizer; like them, the constructor records `initial_lr` in each group and takes one step (to last_epoch + 1)."""

    def __init__(self, optimizer, last_epoch=-1):
        self.optimizer = optimizer
        for g in optimizer.param_groups:
            if last_epoch == -1:
                g.setdefault("initial_lr", g["lr"])
            elif "initial_lr" not in g:
                raise KeyError("param 'initial_lr' is not specified in param_groups when resuming an optimizer")
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self.step(last_epoch + 1)

    def step(self, it):
        self.last_epoch = it
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = self.lr_at(it, base)


class StepDecayLR(_IterationSchedule):
    """LambdaLR(lr_lbmd) of build_scheduler (tools/train_utils/optimization/__init__.py:40-55), in its operation order:
    lr(it) = LR * max(LR_DECAY multiplied once per passed decay step, LR_CLIP / LR)."""

    def __init__(self, optimizer, decay_steps, lr_decay, lr_clip, lr, last_epoch=-1):
        self.decay_steps, self.lr_decay, self.floor = list(decay_steps), lr_decay, lr_clip / lr
        super().__init__(optimizer, last_epoch)

    def factor(self, it):
        cur_decay = 1
        for decay_step in self.decay_steps:
            if it >= decay_step:
                cur_decay = cur_decay * self.lr_decay
        return max(cur_decay, self.floor)

    def lr_at(self, it, base_lr):
        return base_lr * self.factor(it)


class CosineWarmupLR(_IterationSchedule):
    """learning_schedules_fastai.py:80-89: eta_min -> base lr over T_max iterations along half a cosine."""

    def __init__(self, optimizer, T_max, eta_min=0, last_epoch=-1):
        self.T_max, self.eta_min = T_max, eta_min
        super().__init__(optimizer, last_epoch)

    def lr_at(self, it, base_lr):
        return self.eta_min + (base_lr - self.eta_min) * (1 - math.cos(math.pi * it / self.T_max)) / 2


def build_optimizer(model, optim_cfg):
    """tools/train_utils/optimization/__init__.py:11-36: 'adam', 'sgd' and 'adam_onecycle'.  On the GPU the flat fused optimisers;
    FUSED: False in the OPTIMIZATION config (or a CPU model) keeps the per-tensor torch.optim forms, built as the reference builds
    them."""
    ps = [p for p in model.parameters() if p.requires_grad]
    fused = optim_cfg.get("FUSED", True) and ps and all(p.is_cuda and p.dtype == torch.float32 for p in ps)
    if optim_cfg.OPTIMIZER == "adam":
        if fused:
            return FusedAdam(model, lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY)
        return torch.optim.Adam(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY)
    if optim_cfg.OPTIMIZER == "sgd":
        if fused:
            return FusedSGD(model, lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY, momentum=optim_cfg.MOMENTUM)
        return torch.optim.SGD(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY, momentum=optim_cfg.MOMENTUM)
    if optim_cfg.OPTIMIZER != "adam_onecycle":
        raise NotImplementedError("OPTIMIZATION.OPTIMIZER %r: adam, sgd or adam_onecycle" % (optim_cfg.OPTIMIZER,))
    if fused:
        return FusedAdamOneCycle(model, wd=optim_cfg.WEIGHT_DECAY)
    return AdamOneCycle(model, wd=optim_cfg.WEIGHT_DECAY)


def build_scheduler(optimizer, total_iters_each_epoch, total_epochs, last_epoch, optim_cfg):
    """(lr_scheduler, lr_warmup_scheduler) of tools/train_utils/optimization/__init__.py:39-63; the second is None unless LR_WARMUP.
    The reference's T_max, WARMUP_EPOCH * len(total_iters_each_epoch), raises TypeError on the int (:59); here it is
    WARMUP_EPOCH * total_iters_each_epoch."""
    total = total_iters_each_epoch * total_epochs
    if optim_cfg.OPTIMIZER == "adam_onecycle":
        return OneCycle(optimizer, total, optim_cfg.LR, list(optim_cfg.MOMS), optim_cfg.DIV_FACTOR, optim_cfg.PCT_START), None
    decay_steps = [x * total_iters_each_epoch for x in optim_cfg.DECAY_STEP_LIST]
    lr_scheduler = StepDecayLR(optimizer, decay_steps, optim_cfg.LR_DECAY, optim_cfg.LR_CLIP, optim_cfg.LR, last_epoch=last_epoch)
    lr_warmup_scheduler = None
    if optim_cfg.LR_WARMUP:
        lr_warmup_scheduler = CosineWarmupLR(optimizer, T_max=optim_cfg.WARMUP_EPOCH * total_iters_each_epoch,
                                             eta_min=optim_cfg.LR / optim_cfg.DIV_FACTOR)
    return lr_scheduler, lr_warmup_scheduler


def checkpoint_state(model=None, optimizer=None, epoch=None, it=None):
    """The dict tools/train_utils/train_utils.py:124-140 writes: {'epoch', 'it', 'model_state', 'optimizer_state', 'version'}.
    A DDP wrapper is unwrapped (its `.module` holds the reference's key names) and every tensor goes to the CPU, so a file
    written by one rank loads anywhere."""
    model_state = None
    if model is not None:
        inner = model.module if hasattr(model, "module") else model
        model_state = type(inner.state_dict())((k, v.detach().cpu()) for k, v in inner.state_dict().items())

    def to_cpu(o):
        if torch.is_tensor(o):
            return o.detach().cpu()
        if isinstance(o, dict):
            return {k: to_cpu(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(to_cpu(v) for v in o)
        return o
    return {"epoch": epoch, "it": it, "model_state": model_state,
            "optimizer_state": None if optimizer is None else to_cpu(optimizer.state_dict()), "version": "hvpr_amd"}


def save_checkpoint(state, filename="checkpoint"):
    """train_utils.py:143-150: one file `<filename>.pth`."""
    path = "{}.pth".format(filename)
    torch.save(state, path)
    return path


def model_fn_decorator():
    """pcdet/models/__init__.py (absent upstream file) with the 4-tuple HVPR's driver expects (train_utils.py:38)."""
    from .detector import load_data_to_gpu

    def model_func(model, batch_dict):
        load_data_to_gpu(batch_dict)
        ret, tb_dict, disp_dict = model(batch_dict)
        loss = ret["loss"].mean()
        (model.module if hasattr(model, "module") else model).update_global_step()
        # the memory items travel as the fourth value (train_utils.py:38, printed once per epoch :100-101), NOT inside disp_dict:
        # the loop hands disp_dict to tqdm's set_postfix (:45-51), and a (2000, 64) tensor does not belong in a progress bar
        items = disp_dict.pop("items", None)
        return loss, tb_dict, disp_dict, items

    return model_func


def prefetching(model, batches):
    """Iterate `batches` (dicts) one ahead: before batch i is handed out, the point stream's index tensors of batch i + 1 are
    enqueued on a side stream (MixAnchor_Memory.prefetch_point_indices) — so they are computed beside step i.  What a
    maintainer wraps around the data loader in train_one_epoch (tools/train_utils/train_utils.py:25-42)."""
    m = model.module if hasattr(model, "module") else model
    pre = getattr(m, "prefetch_point_indices", lambda b: b)
    it = iter(batches)
    try:
        nxt = pre(next(it))
    except StopIteration:
        return
    for b in it:
        cur, nxt = nxt, pre(b)
        yield cur
    yield nxt


def train_step(model, optimizer, scheduler, batch_dict, it, grad_norm_clip):
    """One iteration of train_one_epoch (train_utils.py:25-42): schedule, zero_grad, forward, backward, clip, step."""
    scheduler.step(it)
    model.train()
    optimizer.zero_grad()
    ret, tb_dict, disp_dict = model(batch_dict)
    loss = ret["loss"].mean()
    loss.backward()
    if hasattr(optimizer, "clip_grad_norm"):          # flat optimiser: the clip coefficient stays on the device
        optimizer.clip_grad_norm(grad_norm_clip)
    else:
        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_norm_clip)
    optimizer.step()
    (model.module if hasattr(model, "module") else model).update_global_step()
    return loss.detach(), tb_dict
