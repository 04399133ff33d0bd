"""GPU: rows a12 + a13 as the library's own kernels (hvpr_assign_targets_f32, hvpr_rpn_losses_f32, hvpr_mse_loss_f32) against the
torch forms of tests/torch_forms.py — which the CPU suite pins to the reference's own AxisAlignedTargetAssigner / loss_utils /
get_loss through fixtures G8 and G16 (tests/test_train_host_logic.py); the kernels themselves also run against G8 and G16 directly
(tests/test_gpu_train_fixtures.py).  Here: full-size anchor sets, three classes, padded / foreign-class / degenerate ground truths,
and the gradients of every loss against torch autograd.  Below those: the assigner against the reference's own outputs at its edges
(fixture G18) and at its size limit, the loss kernels element by element against the torch forms in FLOAT64 on the CPU (every
num_class / direction-head / beta branch, block edges, the full-size grid), the direction bin on its borders, bit-reproducibility,
and the status codes of the three entry points."""
import copy

import numpy as np
import pytest
import torch

import torch_forms
from hvpr_amd import anchor_head
from hvpr_amd.config import hvpr_3class_cfg, hvpr_car_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _heads(which, nx=296, ny=248):
    cfg = hvpr_car_cfg() if which == "car" else hvpr_3class_cfg()
    rng = np.array(cfg.DATA_CONFIG.POINT_CLOUD_RANGE, np.float32)
    rng[3] = rng[0] + nx * 0.16
    rng[4] = rng[1] + ny * 0.16
    mk = lambda: anchor_head.AnchorHeadSingle(model_cfg=cfg.MODEL.DENSE_HEAD, input_channels=64, num_class=len(cfg.CLASS_NAMES),
                                              class_names=cfg.CLASS_NAMES, grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
    hip = mk().to(DEV).train()
    ref = copy.deepcopy(hip)
    hip.anchors = [a.to(DEV) for a in hip.anchors]
    ref.anchors = [a.to(DEV) for a in ref.anchors]
    torch_forms.patch(ref)
    return cfg, hip, ref, rng


def _gt(rng_np, B, G, n_class, pcr, seed):
    r = np.random.default_rng(seed)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
    g = np.zeros((B, G, 8), np.float32)
    for b in range(B):
        k = int(r.integers(0, G + 1)) if b else G // 2           # frame 0: half the rows; another frame may have none or all
        cls = r.integers(0, n_class, k)
        g[b, :k, 0] = r.uniform(pcr[0] + 2, pcr[3] - 2, k)
        g[b, :k, 1] = r.uniform(pcr[1] + 2, pcr[4] - 2, k)
        g[b, :k, 2] = r.uniform(-1.2, -0.6, k)
        g[b, :k, 3:6] = sizes[cls] * r.uniform(0.85, 1.15, (k, 3))
        g[b, :k, 6] = r.uniform(-np.pi, np.pi, k)
        g[b, :k, 7] = cls + 1
        if k > 3:
            g[b, 1] = 0.0                                         # an all-zero row INSIDE the valid range: class 0 wraps to the last class
            g[b, 2, 6] = np.pi / 4                                # heading exactly on the axis-snapping border
    return torch.from_numpy(g).to(DEV)


@pytest.mark.parametrize("which,B,G", [("car", 3, 12), ("3class", 4, 30), ("car", 1, 1), ("3class", 2, 0)])
def test_target_assigner_kernels_equal_the_torch_form(which, B, G):
    cfg, hip, ref, pcr = _heads(which)
    if G == 0:
        gt = torch.zeros((B, 1, 8), device=DEV)                   # only padding
    else:
        gt = _gt(None, B, G, len(cfg.CLASS_NAMES), pcr, seed=B * 100 + G)
    got = hip.assign_targets(gt.clone())
    want = ref.assign_targets(gt.clone())
    assert got["box_cls_labels"].dtype == torch.int32
    assert torch.equal(got["box_cls_labels"], want["box_cls_labels"].to(torch.int32))            # labels: exact
    assert torch.equal(got["reg_weights"], want["reg_weights"])
    torch.testing.assert_close(got["box_reg_targets"], want["box_reg_targets"], rtol=1e-5, atol=1e-6)
    assert torch.equal(got["positives_per_frame"].long(), (want["box_cls_labels"] > 0).sum(dim=1))
    if G > 1:
        lab = want["box_cls_labels"]
        assert int((lab > 0).sum()) >= G // 2 and int((lab == -1).sum()) > 0 and int((lab == 0).sum()) > 0


@pytest.mark.parametrize("which", ["car", "3class"])
def test_loss_kernels_values_and_gradients_equal_torch_autograd(which):
    cfg, hip, ref, pcr = _heads(which, nx=96, ny=80)
    B, n_class = 3, len(cfg.CLASS_NAMES)
    gt = _gt(None, B, 10, n_class, pcr, seed=5)
    gen = torch.Generator(device="cpu").manual_seed(7)
    na = hip.num_anchors_per_location
    shapes = {"cls_preds": na * n_class, "box_preds": na * 7, "dir_cls_preds": na * 2}
    preds = {}
    for sfx in ("", "_point"):
        for k, c in shapes.items():
            scale = 3.0 if k == "cls_preds" else (0.4 if k == "box_preds" else 1.5)
            preds[k + sfx] = (torch.randn(B, 80, 96, c, generator=gen) * scale).to(DEV)
    pos_p = torch.randn(500, 64, generator=gen).to(DEV)
    pos_m = torch.randn(500, 64, generator=gen).to(DEV)
    res = {}
    for name, head in (("hip", hip), ("ref", ref)):
        leaves = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
        pm = pos_m.clone().requires_grad_(True)
        fr = head.forward_ret_dict
        fr.clear()
        fr.update(leaves)
        fr.update(pos_point_feas=pos_p, pos_memory_feas=pm, memory_items=None)
        fr.update(head.assign_targets(gt.clone()))
        rpn, rpn_pt, mem, tb, _ = head.get_loss()
        cot = torch.tensor([0.7, 1.3, 2.1], device=DEV)
        (rpn * cot[0] + rpn_pt * cot[1] + mem * cot[2]).backward()
        res[name] = (dict(rpn=rpn.detach(), rpn_pt=rpn_pt.detach(), mem=mem.detach(), **tb), {k: v.grad for k, v in leaves.items()}, pm.grad)
    (vh, gh, mh), (vr, gr, mr) = res["hip"], res["ref"]
    for k in vr:
        torch.testing.assert_close(vh[k], vr[k], rtol=2e-5, atol=1e-7, msg=k)
    for k in gr:
        err = float((gh[k] - gr[k]).norm() / gr[k].norm())
        assert err < 2e-5, (k, err)
        # element-wise too: no gradient where the reference has none (don't-care anchors, negatives of the box / direction losses)
        assert bool(((gr[k] == 0) == (gh[k] == 0)).float().mean() > 0.9999), k
        # ... and exactly, on every element, from the labels alone (NaN targets: test_rpn_loss_kernel_against_float64_elementwise)
        lab = hip.forward_ret_dict["box_cls_labels"]
        g = gh[k].reshape(B, lab.shape[1], -1)
        assert bool(torch.isfinite(g).all()), k
        assert not bool(g[lab == -1].any()), k
        if not k.startswith("cls_preds"):
            assert not bool(g[lab <= 0].any()), k
    assert float((mh - mr).norm() / mr.norm()) < 1e-6


def test_assigner_and_losses_refuse_cpu_tensors():
    cfg = hvpr_car_cfg()
    head = anchor_head.AnchorHeadSingle(model_cfg=cfg.MODEL.DENSE_HEAD, input_channels=64, num_class=1, class_names=cfg.CLASS_NAMES,
                                        grid_size=np.array([16, 16, 1]), point_cloud_range=np.array([0, -1.28, -3, 2.56, 1.28, 1], np.float32))
    head.anchors = [a.cpu() for a in head.anchors]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.assign_targets(torch.zeros(1, 2, 8))
    from hvpr_amd import losses
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.memory_loss(torch.zeros(4, 64), torch.zeros(4, 64), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.rpn_losses(torch.zeros(1, 4, 1), torch.zeros(1, 4, 7), None, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, 7),
                          torch.zeros(4), torch.zeros(1, dtype=torch.int32), 1, {"code_weights": [1.0] * 7, "cls_weight": 1.0,
                                                                                 "loc_weight": 2.0, "dir_weight": 0.2}, 0.78539, 2)


# ================================================================================================ the assigner at its edges and limits
import ctypes  # noqa: E402
import itertools  # noqa: E402

import train_fixture_cases as C  # noqa: E402
from hvpr_amd import _lib, kernels, losses  # noqa: E402

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3         # include/hvpr_amd.h:30-33
UNSUPPORTED_TEXT = "unsupported shape for this build of the kernels"


def test_g18_assigner_edges_equal_the_reference_on_gpu(golden_dir):
    """hvpr_assign_targets_f32 against the reference's OWN assigner at its edges (fixture G18, train_fixture_cases.run_g18): every
    frame alone and all frames as one batch, labels and weights exact, targets 1e-5; the batch bit for bit what the frames alone
    gave (frames share the LDS staging code, not data)."""
    assert C.run_g18(golden_dir, DEV) == {"car": 21, "3c": 24}


def _gt_full(G, n_valid, pcr, seed):
    r = np.random.default_rng(seed)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
    g = np.zeros((G, 8), np.float32)
    cls = r.integers(0, 3, n_valid)
    g[:n_valid, 0] = r.uniform(pcr[0] + 2, pcr[3] - 2, n_valid)
    g[:n_valid, 1] = r.uniform(pcr[1] + 2, pcr[4] - 2, n_valid)
    g[:n_valid, 2] = r.uniform(-1.2, -0.6, n_valid)
    g[:n_valid, 3:6] = sizes[cls] * r.uniform(0.85, 1.15, (n_valid, 3))
    g[:n_valid, 6] = r.uniform(-np.pi, np.pi, n_valid)
    g[:n_valid, 7] = cls + 1
    return g


def test_target_assigner_at_256_ground_truths_and_refusal_at_257():
    """n_gt at kMaxGt = 256 (every LDS slot of GtLds in use), three classes, the full 296 x 248 grid: labels exactly those of the
    torch form run on the CPU (which G18 pins to the reference), one frame and one anchor set at a time — the (G, A) IoU matrix of
    one frame fits, (B, G, A) does not.  Frame 0 has 256 real rows, frame 1 200 real rows and 56 rows of padding.  257 rows are
    refused through kernels.check with the UNSUPPORTED text before anything is launched: a labels buffer pre-filled with a sentinel
    stays as it was."""
    cfg, hip, ref, pcr = _heads("3class")
    gt = np.stack([_gt_full(256, 256, pcr, 2560), _gt_full(256, 200, pcr, 2561)])
    got = hip.assign_targets(torch.from_numpy(gt).to(DEV))
    cpu = copy.deepcopy(hip).cpu()
    cpu.anchors = [a.cpu() for a in cpu.anchors]
    cpu.target_assigner = None
    torch_forms.patch(cpu)
    for b in range(2):
        want = cpu.assign_targets(torch.from_numpy(gt[b:b + 1].copy()))
        lab = want["box_cls_labels"][0].to(torch.int32)
        assert int((lab > 0).sum()) >= 256 and set(lab.unique().tolist()) == {-1, 0, 1, 2, 3}
        assert torch.equal(got["box_cls_labels"][b].cpu(), lab), b                                       # labels: exact
        assert torch.equal(got["reg_weights"][b].cpu(), want["reg_weights"][0])
        torch.testing.assert_close(got["box_reg_targets"][b].cpu(), want["box_reg_targets"][0], rtol=1e-5, atol=1e-6)
        assert int(got["positives_per_frame"][b]) == int((lab > 0).sum())
    with pytest.raises(RuntimeError, match=UNSUPPORTED_TEXT):
        hip.assign_targets(torch.zeros(1, 257, 8, device=DEV))
    a = _AssignArgs(n_gt=257)
    assert a.call() == UNSUPPORTED
    a.assert_untouched()


class _AssignArgs:
    """Valid device buffers and arguments for a direct hvpr_assign_targets_f32 call (2 locations x 2 rotations, one class), the
    outputs pre-filled with sentinels.  Keyword arguments replace single arguments."""

    def __init__(self, n_gt=4, **over):
        self.anchors = torch.tensor([[1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 1.57],
                                     [3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 1.57]], device=DEV)
        self.gt = torch.zeros(1, max(n_gt, 1), 8, device=DEV)
        self.gt[0, 0] = torch.tensor([1.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0, 1.0])
        self.labels = torch.full((1, 4), 77, dtype=torch.int32, device=DEV)
        self.targets = torch.full((1, 4, 7), 77.0, device=DEV)
        self.weights = torch.full((1, 4), 77.0, device=DEV)
        self.pos = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        self.ws = torch.full((4096,), 77, dtype=torch.uint8, device=DEV)
        self.v = dict(n_anchors=4, batch=1, n_gt=n_gt, class_index=0, n_classes=1, matched=0.6, unmatched=0.45, rots=2, loc_stride=2,
                      loc_offset=0, anchors_total=4, ws_bytes=self.ws.numel())
        self.v.update(over)

    def call(self):
        v = self.v
        rc = kernels.lib().hvpr_assign_targets_f32(
            self.anchors.data_ptr(), v["n_anchors"], self.gt.data_ptr(), v["batch"], v["n_gt"], v["class_index"], v["n_classes"],
            v["matched"], v["unmatched"], v["rots"], v["loc_stride"], v["loc_offset"], v["anchors_total"], self.labels.data_ptr(),
            self.targets.data_ptr(), self.weights.data_ptr(), self.pos.data_ptr(), self.ws.data_ptr(), v["ws_bytes"], kernels._stream())
        torch.cuda.synchronize()
        return rc

    def assert_untouched(self):
        assert bool((self.labels == 77).all()) and bool((self.targets == 77).all()) and bool((self.weights == 77).all())
        assert bool((self.pos == 77).all()) and bool((self.ws == 77).all())


def test_assign_targets_status_codes():
    """The entry point's refusals, by direct calls with valid device buffers: each returns its status from the host checks that sit
    above the first launch and writes nothing.  The same arguments without the fault run (status 0) and label the anchor that IS
    the ground truth."""
    need = int(kernels.lib().hvpr_assign_targets_workspace_bytes(1, 4))
    assert need == 256
    for over, status in ((dict(ws_bytes=need - 1), WORKSPACE), (dict(loc_stride=3, loc_offset=2, anchors_total=6), INVALID_ARG),
                         (dict(rots=3, loc_stride=3), INVALID_ARG), (dict(class_index=1), INVALID_ARG),
                         (dict(class_index=3, n_classes=3), INVALID_ARG), (dict(n_gt=-1), INVALID_ARG)):
        a = _AssignArgs(**over)
        assert a.call() == status, over
        a.assert_untouched()
    a = _AssignArgs(ws_bytes=need)
    a.pos.zero_()
    assert a.call() == OK
    assert a.labels.tolist() == [[1, 0, 0, 0]] and a.pos.tolist() == [1] and a.weights.tolist() == [[1.0, 0.0, 0.0, 0.0]]


# ================================================================================================ the loss kernels against float64
CODE_W = [1.0, 0.5, 2.0, 1.0, 1.5, 1.0, 0.75]
LOSS_W = {"code_weights": CODE_W, "cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2}
DIR_OFFSET = 0.78539
CLS_SPECIALS = [0.0, 1e-4, -1e-4, 20.0, -20.0, 40.0, -40.0, 90.0, -90.0]


def _frame_labels(kind, A, nc, r):
    if kind == "none":                                             # no positive: the pos_norm clamp
        return r.choice(np.array([0, -1], np.int32), A, p=[0.8, 0.2])
    if kind == "dontcare":
        return np.full(A, -1, np.int32)
    if kind == "all":
        return r.integers(1, nc + 1, A).astype(np.int32)
    lab = r.choice(np.array([0, -1, 1], np.int32), A, p=[0.6, 0.1, 0.3])                     # mixed
    lab[lab > 0] = r.integers(1, nc + 1, int((lab > 0).sum()))
    lab[:min(A, 7)] = np.array([1, 0, -1, nc, 1, 0, 1], np.int32)[:min(A, 7)]
    return lab


def _loss_inputs(B, A, nc, nb, beta, seed=0):
    """fp32 CPU inputs of one prediction stream, labels / targets / positives made by hand (no assigner), with the edges the kernel
    has branches for; what was planted is asserted here.  nb = 0: no direction head."""
    r = np.random.default_rng(1000 * seed + 17 * A + 5 * nc + nb)
    kinds = {1: ["mixed"], 2: ["mixed", "none"], 3: ["none", "dontcare", "all"]}[B]
    labels = np.stack([_frame_labels(k, A, nc, r) for k in kinds])
    cls = (r.standard_normal((B, A, nc)) * 3).astype(np.float32)
    box = (r.standard_normal((B, A, 7)) * 0.4).astype(np.float32)
    tgt = (r.standard_normal((B, A, 7)) * 0.4).astype(np.float32)
    tgt[labels <= 0] = 0.0                                         # as the assigner leaves them
    arot = np.tile(np.array([0.0, 1.57], np.float32), (A + 1) // 2)[:A]
    # headings: reg_target[6] + anchor_rot well inside a bin for 1, 2 and 8 bins (the borders of 8 bins contain the others')
    k8, u = r.integers(-8, 16, (B, A)), r.uniform(0.05, 0.95, (B, A))
    rot_gt = np.float32(DIR_OFFSET) + ((k8 + u) * (2 * np.pi / 8)).astype(np.float32)
    tgt[..., 6] = np.where(labels > 0, rot_gt - arot[None], 0.0).astype(np.float32)
    v = (tgt[..., 6].astype(np.float64) + arot[None].astype(np.float64) - DIR_OFFSET) / (2 * np.pi / 8)
    assert np.abs(v - np.round(v))[labels > 0].min(initial=1.0) * (2 * np.pi / 8) >= 1e-3
    planted = dict(cls_specials=0, beta_edge=0, nan=0)
    bb = np.float32(beta if beta >= 1e-5 else 0.25)
    for b in range(B):
        cared = np.nonzero(labels[b] >= 0)[0]
        pos = np.nonzero(labels[b] > 0)[0]
        if len(cared) >= 2 * len(CLS_SPECIALS):
            for i, s in enumerate(CLS_SPECIALS):                   # on a cared anchor; every channel in turn
                cls[b, cared[i], i % nc] = s
            planted["cls_specials"] += 1
        if len(pos) >= 40:
            for i, s in enumerate(CLS_SPECIALS):                   # and on the TARGET channel of a positive
                cls[b, pos[i], labels[b, pos[i]] - 1] = s
            # slots 0 and 3 have code weight 1; target 0 makes pred - target exact in fp32 and in float64 alike
            edge = [bb, np.nextafter(bb, np.float32(0)), np.nextafter(bb, np.float32(1)), np.float32(0.0), -bb]
            for i, e in enumerate(edge):
                for j in (0, 3):
                    tgt[b, pos[10 + i], j] = 0.0
                    box[b, pos[10 + i], j] = e
            box[b, pos[15]] = tgt[b, pos[15]]                      # every residual exactly 0, the sin-difference slot included
            planted["beta_edge"] += 1
            # NaN targets, slots 0..5.  Slot 6 is left out: with a NaN heading the reference's own add_sin_difference makes the
            # PREDICTION side (sin a cos b) NaN as well, and the direction bin of a NaN heading is undefined
            for i in range(6):
                tgt[b, pos[20 + i], i] = np.nan
            tgt[b, pos[26], 0:6] = np.nan
            planted["nan"] += 1
    t = lambda a: torch.from_numpy(a)
    ins = dict(cls=t(cls), box=t(box), dir=t((r.standard_normal((B, A, nb)) * 1.5).astype(np.float32)) if nb else None, labels=t(labels),
               targets=t(tgt), arot=t(arot), pos_count=t((labels > 0).sum(1).astype(np.int32)))
    return ins, kinds, planted


def _loss_form(ins, nc, nb, beta, dtype):
    """torch_forms.rpn_losses on the CPU with autograd in `dtype`: ([cls, loc, dir] values, {tensor name: gradient})."""
    up = lambda a: a.detach().clone().to(dtype).requires_grad_(True)
    leaves = {"cls": up(ins["cls"]), "box": up(ins["box"])}
    if nb:
        leaves["dir"] = up(ins["dir"])
    anchors = torch.zeros(ins["arot"].shape[0], 7, dtype=dtype)
    anchors[:, 6] = ins["arot"].to(dtype)
    _, _, parts = torch_forms.rpn_losses(leaves["cls"], leaves["box"], leaves.get("dir"), ins["labels"], ins["targets"].to(dtype), anchors,
                                         nc, 1, LOSS_W, DIR_OFFSET, max(nb, 1), beta=beta)
    sum(parts.values()).backward()                                 # every leaf receives the gradient of its own loss only
    return [float(parts[k].detach()) for k in ("cls", "loc", "dir") if k in parts], {k: v.grad for k, v in leaves.items()}


def _loss_kernel(ins, nc, nb, beta, dir_offset=DIR_OFFSET):
    leaves = {k: ins[k].to(DEV).requires_grad_(True) for k in ("cls", "box", "dir") if ins[k] is not None}
    _, _, parts = losses.rpn_losses(leaves["cls"], leaves["box"], leaves.get("dir"), ins["labels"].to(DEV), ins["targets"].to(DEV),
                                    ins["arot"].to(DEV), ins["pos_count"].to(DEV), nc, LOSS_W, dir_offset, nb, beta=beta)
    sum(parts.values()).backward()
    return [float(parts[k].detach()) for k in ("cls", "loc", "dir") if k in parts], {k: v.grad.cpu() for k, v in leaves.items()}


def _check_zero_pattern(ins, grads):
    """Exact and total, derived from the labels alone: no class gradient on don't-care anchors, no box / direction gradient off the
    positives, no box gradient in a slot whose target is NaN; nothing NaN or inf anywhere."""
    lab = ins["labels"]
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
    assert not bool(grads["cls"][lab == -1].any())
    assert not bool(grads["box"][lab <= 0].any())
    assert not bool(grads["box"][torch.isnan(ins["targets"])].any())
    if "dir" in grads:
        assert not bool(grads["dir"][lab <= 0].any())


def _check_against_float64(ins, nc, nb, beta, observed, tag, got=None):
    v64, g64 = _loss_form(ins, nc, nb, beta, torch.float64)
    _, g32 = _loss_form(ins, nc, nb, beta, torch.float32)
    vk, gk = got if got is not None else _loss_kernel(ins, nc, nb, beta)
    np.testing.assert_allclose(vk, v64, rtol=2e-5, atol=0, err_msg=tag)
    _check_zero_pattern(ins, gk)
    for k in g64:
        e32 = float((g32[k].double() - g64[k]).abs().max())        # the reference forms only: fp32 torch against float64 torch
        ek = float((gk[k].double() - g64[k]).abs().max())
        bound = 4 * e32 + 2.0 ** -23 * float(g64[k].abs().max())
        observed(f"test_gpu_assign_loss {tag} g_{k}: kernel {ek:.3e}, fp32 torch form e32 {e32:.3e}, bound {bound:.3e}")
        assert ek <= bound, (tag, k, ek, e32, bound)


_COMBOS = list(itertools.product((1, 2, 3), (0, 1, 2, 8), (1.0 / 9.0, 0.0)))


@pytest.mark.parametrize("nc,nb,beta", _COMBOS, ids=[f"nc{c}-bins{b}-{'smooth' if be else 'l1'}" for c, b, be in _COMBOS])
def test_rpn_loss_kernel_against_float64_elementwise(nc, nb, beta, observed):
    """hvpr_rpn_losses_f32 against torch_forms.rpn_losses run on the CPU in FLOAT64 with autograd on the same fp32 inputs upcast,
    (B, A) = (3, 46 080): a frame with no positive (pos_norm clamp), a frame that is all don't-care, a frame that is all positive;
    class logits at 0, +-1e-4, +-20, +-40, +-90; box residuals with |diff| exactly beta, one ulp either side, exactly 0; NaN targets
    in slots 0..5 (slot 6 excluded: with a NaN heading the reference's add_sin_difference makes the prediction side NaN too and
    the direction bin is undefined); headings >= 1e-3 rad inside their direction bin; code weights that are not all 1.
    num_class 1 / 2 / 3 (the <2> instantiation included), direction head absent or with 1 / 2 / 8 bins, smooth-L1 and the plain-L1
    branch (beta 0).
      * values: rtol 2e-5;
      * gradients ELEMENT-wise: max |kernel - float64| <= 4 * e32 + 2^-23 * max |g64| per tensor, e32 = the largest element-wise
        error of the fp32 torch form on the CPU against the float64 form (never taken from the kernel).  The factor 4 covers the
        kernel's different but equally valid operation order (sigmoid as 1 / (1 + expf(-x)), log-sum-exp) and the device's
        expf / logf / sinf at 1-2 ulp; the floor is one ulp of the largest gradient;
      * zero pattern exact and total, from the labels (_check_zero_pattern).
    Seen on the MI355X (largest over the 24 combinations; kernel error / e32 / bound): g_cls 3.5e-7 / 3.2e-7 / 1.3e-6, g_box
    1.0e-11 / 6.7e-12 / 3.0e-11, g_dir 5.4e-13 / 2.8e-13 / 1.3e-12; the kernel never used more than 0.42 of a bound.  Before the
    kernel took autograd's value at a logit of exactly 0 (1 - t, not p - t) the planted zeros missed the class bound by 4.7e-2."""
    ins, kinds, planted = _loss_inputs(3, 46080, nc, nb, beta)
    lab = ins["labels"]
    assert kinds == ["none", "dontcare", "all"]
    assert not bool((lab[0] > 0).any()) and bool((lab[0] == 0).any()) and bool((lab[1] == -1).all()) and bool((lab[2] > 0).all())
    assert ins["pos_count"].tolist() == [0, 0, 46080]
    assert planted == dict(cls_specials=2, beta_edge=1, nan=1) and int(torch.isnan(ins["targets"]).sum()) == 12
    for s in CLS_SPECIALS:
        assert bool(((ins["cls"] == s).any(-1) & (lab >= 0)).any()), s
    _check_against_float64(ins, nc, nb, beta, observed, f"(3, 46080) nc {nc} bins {nb} beta {beta:.3f}")


@pytest.mark.parametrize("B,A", [(1, 255), (1, 257), (2, 7)])
@pytest.mark.parametrize("nc,nb,beta", [(3, 2, 1.0 / 9.0), (2, 8, 0.0), (1, 0, 1.0 / 9.0)])
def test_rpn_loss_kernel_against_float64_block_edges(B, A, nc, nb, beta, observed):
    """The same check one anchor short of a block, one anchor into the second block (its other 255 threads idle) and at 14 anchors in
    all: mixed frames (positives, negatives, don't-cares), the second frame of B = 2 without a positive.  Seen on the MI355X: at most
    0.56 of a bound (g_dir, (1, 255), 8 bins: 8.2e-10 against e32 2.9e-10)."""
    ins, kinds, planted = _loss_inputs(B, A, nc, nb, beta, seed=1)
    assert kinds[0] == "mixed" and int(ins["pos_count"][0]) >= 3 and bool((ins["labels"][0] == 0).any()) and bool((ins["labels"][0] == -1).any())
    if A >= 255:
        assert planted["nan"] == 1 and planted["beta_edge"] == 1
    if B == 2:
        assert int(ins["pos_count"][1]) == 0
    _check_against_float64(ins, nc, nb, beta, observed, f"({B}, {A}) nc {nc} bins {nb} beta {beta:.3f}")


FULL = (2, 440448, 3, 2, 1.0 / 9.0)       # the three-class head on the 296 x 248 grid, 6 anchors per location: 3 441 loss blocks


@pytest.fixture(scope="module")
def full_size_case():
    """Inputs, the float64 and fp32 CPU forms (the slow part: once per module) of the full-size case."""
    B, A, nc, nb, beta = FULL
    ins, kinds, planted = _loss_inputs(B, A, nc, nb, beta, seed=2)
    assert kinds == ["mixed", "none"] and planted == dict(cls_specials=2, beta_edge=1, nan=1)
    return ins


def test_rpn_loss_kernel_full_size_against_float64_and_bit_reproducible(full_size_case, observed):
    """(2, 440 448): cdiv(2 * 440 448, 256) = 3 441 partial sums, so k_loss_sum's strided loop runs 14 rounds (the op-level test has
    180 blocks: none).  Values and element-wise gradients against float64 as above; and the same call twice on fresh output buffers
    gives the same bits in the losses and all three gradient tensors (fixed-order sums, no float atomics).  Seen on the MI355X
    (kernel / e32 / bound): g_cls 5.6e-7 / 5.3e-7 / 2.2e-6, g_box 4.7e-12 / 3.8e-12 / 1.7e-11, g_dir 2.8e-13 / 1.0e-13 / 5.1e-13."""
    B, A, nc, nb, beta = FULL
    ins = full_size_case
    assert kernels.lib().hvpr_rpn_losses_workspace_bytes(B, A) == 3441 * 3 * 4

    def raw():
        d = {k: (v.to(DEV) if v is not None else None) for k, v in ins.items()}
        out = torch.full((3,), 77.0, device=DEV)
        g = [torch.full_like(d[k], 77.0) for k in ("cls", "box", "dir")]
        ws = torch.empty(3441 * 12, dtype=torch.uint8, device=DEV)
        cw = (ctypes.c_float * 7)(*CODE_W)
        rc = kernels.lib().hvpr_rpn_losses_f32(d["cls"].data_ptr(), d["box"].data_ptr(), d["dir"].data_ptr(), d["labels"].data_ptr(),
                                               d["targets"].data_ptr(), d["arot"].data_ptr(), d["pos_count"].data_ptr(), B, A, nc, nb, 0.25, 2.0,
                                               beta, ctypes.cast(cw, ctypes.c_void_p), 1.0, 2.0, 0.2, DIR_OFFSET, out.data_ptr(),
                                               g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
        torch.cuda.synchronize()
        assert rc == OK
        return out.cpu(), [t.cpu() for t in g]
    (o1, g1), (o2, g2) = raw(), raw()
    assert torch.equal(o1, o2)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    vk, gk = _loss_kernel(ins, nc, nb, beta)
    assert vk == o1.tolist() and all(torch.equal(gk[k], g) for k, g in zip(("cls", "box", "dir"), g1))     # the wrapper adds nothing
    _check_against_float64(ins, nc, nb, beta, observed, f"(2, 440448) nc {nc} bins {nb} beta {beta:.3f}", got=(vk, gk))


@pytest.mark.parametrize("nb", [2, 8])
@pytest.mark.parametrize("dir_offset", [0.75, DIR_OFFSET])
def test_direction_bin_on_the_bin_borders(nb, dir_offset):
    """v = reg_target[6] + anchor_rot - dir_offset at the bin borders 0, pi, 2 pi, -pi and the fp32 values next to them: the bin is a
    rounding decision of fp32 arithmetic, so the judge is the FP32 torch form on the CPU (direction_targets, which G16 pins to the
    reference), not float64.  Headings: fl(border + dir_offset) and the three fp32 numbers on either side.  With dir_offset 0.75
    the subtraction is exact, so v takes the border itself and both its neighbours (asserted); with the configuration's 0.78539 the
    exact difference falls half way between two fp32 numbers and v takes every other one, on both sides of the border (asserted).
    Half the anchors have rotation 0, the other half 1.57 and a heading moved by it.  The sign pattern of g_dir gives the kernel's
    bin: softmax - 1 < 0 on the bin, softmax > 0 elsewhere."""
    off = np.float32(dir_offset)
    tg6, side = [], []
    for base in (0.0, np.pi, 2 * np.pi, -np.pi):
        b32 = np.float32(base)
        t = np.float32(b32 + off)
        for _ in range(3):
            t = np.nextafter(t, np.float32(-100))
        vs = []
        for _ in range(7):
            tg6.append(t)
            vs.append(np.float32(t - off))
            t = np.nextafter(t, np.float32(100))
        assert min(vs) < b32 < max(vs)
        if dir_offset == 0.75:
            assert b32 in vs and len(set(vs)) == 7
            if base != 0.0:
                assert np.nextafter(b32, np.float32(-100)) in vs and np.nextafter(b32, np.float32(100)) in vs
    n = len(tg6)
    tg6 = np.array(tg6 + [np.float32(t - np.float32(1.57)) for t in tg6], np.float32)
    A = 2 * n
    arot = np.zeros(A, np.float32)
    arot[n:] = 1.57
    tgt = torch.zeros(1, A, 7)
    tgt[0, :, 6] = torch.from_numpy(tg6)
    anchors = torch.zeros(A, 7)
    anchors[:, 6] = torch.from_numpy(arot)
    want = torch_forms.direction_targets(anchors[None], tgt, dir_offset, nb).argmax(-1)[0]
    assert set(want.tolist()) == ({0, 1} if nb == 2 else {0, 3, 4, 7})          # the borders do separate bins
    gen = torch.Generator().manual_seed(3)
    ins = dict(cls=torch.randn(1, A, 1, generator=gen), box=torch.randn(1, A, 7, generator=gen) * 0.3, dir=torch.randn(1, A, nb, generator=gen),
               labels=torch.ones(1, A, dtype=torch.int32), targets=tgt, arot=torch.from_numpy(arot), pos_count=torch.tensor([A], dtype=torch.int32))
    _, gk = _loss_kernel(ins, 1, nb, 1.0 / 9.0, dir_offset=dir_offset)
    neg = gk["dir"][0] < 0
    assert bool((neg.sum(-1) == 1).all())
    assert torch.equal(neg.float().argmax(-1), want), (neg.float().argmax(-1).tolist(), want.tolist())


@pytest.mark.parametrize("M,C_", [(1, 1), (500, 64), (3, 7), (16385, 64), (40000, 64)])
def test_memory_loss_kernel_against_float64(M, C_, observed):
    """hvpr_mse_loss_f32 against torch_forms.memory_loss on the CPU in float64: (16 385, 64) is the first row count past the
    1024-block x 1024-element cap, where k_mse_partial's grid-stride loop starts to loop; (40 000, 64) loops 2-3 times.  Value
    rtol 2e-5, gradient element-wise by the 4 * e32 + one-ulp rule of the loss test.  Seen on the MI355X (kernel / e32 / bound):
    (1, 1) 4.5e-8 / 4.5e-8 / 4.0e-7, (500, 64) 9.9e-14 / 1.5e-13 / 7.6e-13, (3, 7) 6.4e-9 / 6.4e-9 / 4.2e-8, (16 385, 64)
    1.0e-16 / 1.2e-16 / 6.4e-16, (40 000, 64) 2.0e-17 / 2.6e-17 / 1.3e-16."""
    gen = torch.Generator().manual_seed(M + C_)
    x, y = torch.randn(M, C_, generator=gen), torch.randn(M, C_, generator=gen)
    res = {}
    for name, dt, dev in (("f64", torch.float64, "cpu"), ("f32", torch.float32, "cpu")):
        leaf = x.clone().to(dt).requires_grad_(True)
        v = torch_forms.memory_loss(leaf, y.to(dt), 1.5)
        v.backward()
        res[name] = (float(v), leaf.grad)
    leaf = x.to(DEV).requires_grad_(True)
    v = losses.memory_loss(leaf, y.to(DEV), 1.5)
    v.backward()
    gk = leaf.grad.cpu()
    np.testing.assert_allclose(float(v), res["f64"][0], rtol=2e-5, atol=0)
    g64 = res["f64"][1]
    e32 = float((res["f32"][1].double() - g64).abs().max())
    ek = float((gk.double() - g64).abs().max())
    bound = 4 * e32 + 2.0 ** -23 * float(g64.abs().max())
    observed(f"test_gpu_assign_loss memory loss ({M}, {C_}) gradient: kernel {ek:.3e}, fp32 torch form e32 {e32:.3e}, bound {bound:.3e}")
    assert bool(torch.isfinite(gk).all()) and ek <= bound, (ek, e32, bound)


def test_memory_loss_of_no_rows_is_zero_with_a_gradient_path():
    leaf = torch.zeros(0, 64, device=DEV, requires_grad=True)
    v = losses.memory_loss(leaf, torch.zeros(0, 64, device=DEV), 1.0)
    assert float(v) == 0.0 and v.requires_grad
    v.backward()
    assert leaf.grad is not None and leaf.grad.shape == (0, 64)


def test_loss_entry_points_status_codes():
    """hvpr_rpn_losses_f32 / hvpr_mse_loss_f32 refuse on the host, above their first launch: outputs pre-filled with a sentinel stay
    as they were."""
    L = kernels.lib()
    B, A = 1, 300
    ins, _, _ = _loss_inputs(B, A, 3, 8, 1.0 / 9.0, seed=4)
    d = {k: (v.to(DEV) if v is not None else None) for k, v in ins.items()}
    need = int(L.hvpr_rpn_losses_workspace_bytes(B, A))
    assert need == 2 * 3 * 4
    cw = (ctypes.c_float * 7)(*CODE_W)

    def call(nc=3, nb=8, gamma=2.0, ws_bytes=need, grad_dir=True, dir_preds=True):
        out = torch.full((3,), 77.0, device=DEV)
        g = [torch.full((B, A, n), 77.0, device=DEV) for n in (3, 7, 9)]
        ws = torch.full((256,), 77, dtype=torch.uint8, device=DEV)
        rc = L.hvpr_rpn_losses_f32(d["cls"].data_ptr(), d["box"].data_ptr(), d["dir"].data_ptr() if dir_preds else None, d["labels"].data_ptr(),
                                   d["targets"].data_ptr(), d["arot"].data_ptr(), d["pos_count"].data_ptr(), B, A, nc, nb, 0.25, gamma, 1.0 / 9.0,
                                   ctypes.cast(cw, ctypes.c_void_p), 1.0, 2.0, 0.2, DIR_OFFSET, out.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                                   g[2].data_ptr() if grad_dir else None, ws.data_ptr(), ws_bytes, kernels._stream())
        torch.cuda.synchronize()
        untouched = bool((out == 77).all()) and all(bool((t == 77).all()) for t in g) and bool((ws == 77).all())
        return rc, untouched
    assert call(gamma=1.5) == (UNSUPPORTED, True)
    assert call(nc=4) == (UNSUPPORTED, True)
    assert call(nb=9) == (UNSUPPORTED, True)
    assert call(ws_bytes=need - 1) == (WORKSPACE, True)
    assert call(grad_dir=False) == (INVALID_ARG, True)
    assert call() == (OK, False)
    assert call(dir_preds=False, grad_dir=False)[0] == OK          # no direction head: grad_dir may be NULL
    assert kernels.lib().hvpr_status_string(UNSUPPORTED).decode() == UNSUPPORTED_TEXT
    # the memory loss
    x, y = torch.randn(5, 4, device=DEV), torch.randn(5, 4, device=DEV)
    out, gx = torch.full((), 77.0, device=DEV), torch.full((5, 4), 77.0, device=DEV)
    ws = torch.full((4096,), 77, dtype=torch.uint8, device=DEV)
    need = int(L.hvpr_mse_loss_workspace_bytes())
    for rows, cols, wsb, status in ((5, 4, need - 1, WORKSPACE), (0, 4, need, INVALID_ARG), (5, 0, need, INVALID_ARG)):
        assert L.hvpr_mse_loss_f32(x.data_ptr(), y.data_ptr(), rows, cols, 1.0, out.data_ptr(), gx.data_ptr(), ws.data_ptr(), wsb,
                                   kernels._stream()) == status
        torch.cuda.synchronize()
        assert float(out) == 77.0 and bool((gx == 77).all()) and bool((ws == 77).all())
