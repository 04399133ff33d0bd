"""GPU parity of the training convolutions: the library's forward / data-gradient / weight-gradient
kernels, train-mode BatchNorm + ReLU and the whole two-stream backbone training forward + backward against torch fp32 autograd
of the same modules (the form the reference runs: base_bev_backbone.py:228-279).  Tolerance: north_star's 1e-3 relative,
element-wise with the absolute term tied to the tensor's own rms."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hvpr_amd import conv_train as ct
from hvpr_amd import detector, synthetic_weights
from hvpr_amd.config import hvpr_car_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, ref, rtol=1e-3, what=""):
    got, ref = got.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy()
    rms = float(np.sqrt(np.mean(np.square(ref, dtype=np.float64))))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * max(rms, 1e-30), err_msg=what)


# the three level shapes of hvpr_car (trunk / SFM 3x3, the two strided level entries, the scale stream) + odd sizes
CONV_CASES = [
    (1, 248, 296, 128, 128, 1), (1, 248, 296, 128, 256, 2), (1, 124, 148, 256, 256, 1), (1, 124, 148, 256, 512, 2),
    (1, 62, 74, 512, 512, 1), (2, 248, 296, 32, 32, 1), (2, 248, 296, 32, 64, 2), (1, 124, 148, 64, 128, 2),
    (3, 31, 45, 32, 64, 1), (3, 31, 45, 64, 32, 2), (2, 8, 8, 128, 128, 1), (1, 5, 3, 32, 32, 2),
]


@pytest.mark.parametrize("N,H,W,cin,cout,stride", CONV_CASES)
def test_conv3x3_forward_dgrad_wgrad_match_torch(N, H, W, cin, cout, stride):
    g = torch.Generator().manual_seed(H * 7 + cin + stride)
    x = torch.randn(N, H, W, cin, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(DEV).requires_grad_(True)
    z = ct.conv(x, w, stride)
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    zr = F.conv2d(xr.permute(0, 3, 1, 2), wr, stride=stride, padding=1).permute(0, 2, 3, 1)
    assert z.shape == zr.shape
    _close(z, zr, what="forward")
    dz = torch.randn(z.shape, generator=g).to(DEV)
    dx, dw = torch.autograd.grad(z, (x, w), dz)
    dxr, dwr = torch.autograd.grad(zr, (xr, wr), dz)
    _close(dx, dxr, what="dgrad")
    _close(dw, dwr, what="wgrad")


# 1x1 layers: the detection head (384 -> 24: the few-output-rows form of the weight gradient, all four waves along ci), the same with
# ragged channel counts / sizes, and the 128 x 128 block form on either side of the switch (Cout <= 32 and Cin > 256)
@pytest.mark.parametrize("N,H,W,cin,cout", [(1, 248, 296, 384, 24), (2, 31, 45, 384, 8), (1, 9, 7, 512, 32), (2, 13, 5, 264, 16),
                                            (1, 31, 45, 256, 24), (1, 31, 45, 384, 40), (1, 62, 74, 512, 128)])
def test_conv1x1_forward_dgrad_wgrad_match_float64(N, H, W, cin, cout):
    g = torch.Generator().manual_seed(H + cin + cout)
    x = torch.randn(N, H, W, cin, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(DEV).requires_grad_(True)
    z = ct.conv(x, w, 1)
    xr, wr = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    zr = F.conv2d(xr.permute(0, 3, 1, 2), wr).permute(0, 2, 3, 1)
    _close(z, zr, rtol=2e-5, what="forward")
    dz = torch.randn(z.shape, generator=g).to(DEV)
    dx, dw = torch.autograd.grad(z, (x, w), dz)
    dxr, dwr = torch.autograd.grad(zr, (xr, wr), dz.double())
    _close(dx, dxr, rtol=2e-5, what="dgrad")
    _close(dw, dwr, rtol=2e-5, what="wgrad")
    assert torch.equal(dw, ct.conv_wgrad(x.detach(), dz, 1, 1, cout, cin))          # deterministic


@pytest.mark.parametrize("N,H,W,cin,cout,s", [(1, 248, 296, 128, 128, 1), (1, 124, 148, 256, 128, 2), (1, 62, 74, 512, 128, 4),
                                               (2, 9, 7, 128, 128, 2), (2, 5, 6, 64, 128, 4)])
def test_deconv_forward_and_backward_match_torch(N, H, W, cin, cout, s):
    g = torch.Generator().manual_seed(H + s)
    x = torch.randn(N, H, W, cin, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(cin, cout, s, s, generator=g) / cin ** 0.5).to(DEV).requires_grad_(True)
    z = ct.deconv(x, w)
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    zr = F.conv_transpose2d(xr.permute(0, 3, 1, 2), wr, stride=s).permute(0, 2, 3, 1)
    assert z.shape == zr.shape == (N, H * s, W * s, cout)
    _close(z, zr, what="forward")
    dz = torch.randn(z.shape, generator=g).to(DEV)
    dx, dw = torch.autograd.grad(z, (x, w), dz)
    dxr, dwr = torch.autograd.grad(zr, (xr, wr), dz)
    _close(dx, dxr, what="dgrad")
    _close(dw, dwr, what="wgrad")


@pytest.mark.parametrize("shape,relu", [((2, 62, 74, 512), True), ((1, 248, 296, 128), True), ((3, 31, 45, 32), True), ((2, 40, 40, 384), False),
                                        ((4, 3, 5, 64), True)])
def test_bn_relu_train_mode_matches_torch(shape, relu):
    g = torch.Generator().manual_seed(shape[1])
    C = shape[-1]
    z = (torch.randn(shape, generator=g) * 2 + 0.5).to(DEV).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5); bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    ref = copy.deepcopy(bn)
    y = ct.bn_relu(z, bn, relu=relu)
    zr = z.detach().clone().requires_grad_(True)
    yr = ref(zr.permute(0, 3, 1, 2))
    yr = (torch.relu(yr) if relu else yr).permute(0, 2, 3, 1)
    _close(y, yr, what="forward")
    _close(bn.running_mean, ref.running_mean, rtol=1e-5, what="running_mean")
    _close(bn.running_var, ref.running_var, rtol=1e-5, what="running_var")
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    dy = torch.randn(shape, generator=g).to(DEV)
    dz, dg, db = torch.autograd.grad(y, (z, bn.weight, bn.bias), dy)
    dzr, dgr, dbr = torch.autograd.grad(yr, (zr, ref.weight, ref.bias), dy)
    _close(dz, dzr, what="dz")
    _close(dg, dgr, what="dgamma")
    _close(db, dbr, what="dbeta")


@contextlib.contextmanager
def _without_miopen():
    """torch's native convolution / BatchNorm kernels instead of MIOpen's."""
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = was


def test_backbone_training_forward_backward_hip_equals_torch_autograd():
    """The whole BaseBEVBackbone_Scale training forward (two streams through shared weights, SFM steps with the shared gate,
    multi-call BatchNorm running statistics) and its backward: own kernels vs torch autograd of the same module."""
    cfg = copy.deepcopy(hvpr_car_cfg())
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = [0, -5.12, -3, 12.8, 5.12, 1]          # 80 x 64 canvas
    model = detector.build_network(cfg.MODEL, 1, detector.SyntheticDataset(cfg, training=True))
    synthetic_weights.load_synthetic(model, seed=11)
    a = model.backbone_2d.to(DEV).train()
    b = copy.deepcopy(a)
    g = torch.Generator().manual_seed(3)

    def canvas(c):
        t = torch.randn(2, 64, 80, c, generator=g).to(DEV)
        t = t * (torch.rand(2, 64, 80, 1, generator=g).to(DEV) < 0.3)           # sparse, like a BEV canvas
        return t.permute(0, 3, 1, 2)                                            # (B,C,H,W) channels_last
    sp, spp, sc = canvas(128), canvas(128), canvas(32)
    outs = {}
    ref64 = copy.deepcopy(a).double()                      # the yardstick: the same module in float64 through torch autograd
    import torch_forms
    for name, m, mode, dt in (("hip", a, "hip", torch.float32), ("torch", b, "torch", torch.float32), ("f64", ref64, "torch", torch.float64)):
        # the torch passes run on torch's native convolutions (MIOpen off): MIOpen picks its solvers by timing them, and the winner
        # moved torch fp32's distance to float64 on this chain — the bar below — by up to 9x from run to run
        native = _without_miopen() if mode == "torch" else contextlib.nullcontext()
        with (torch_forms.patched(m) if mode == "torch" else contextlib.nullcontext()), native:
            ins = [t.detach().clone().to(dt).requires_grad_(True) for t in (sp, spp, sc)]
            d = m({"spatial_features": ins[0], "spatial_features_point": ins[1], "spatial_scale_features": ins[2]})
            f, fp = d["spatial_features_2d"], d["spatial_features_point_2d"]
            loss = (f * torch.linspace(0.5, 1.5, f.shape[1], device=DEV, dtype=dt).view(1, -1, 1, 1)).pow(2).mean() + fp.abs().mean()
            loss.backward()
            outs[name] = (f.detach(), fp.detach(), [t.grad for t in ins], {k: p.grad for k, p in m.named_parameters()},
                          {k: v.detach().clone() for k, v in m.named_buffers()})
    h, t, r = outs["hip"], outs["torch"], outs["f64"]
    assert h[0].shape == (2, 384, 64, 80)
    _close(h[0], r[0], what="spatial_features_2d")                  # forward: element-wise 1e-3 against float64
    _close(h[1], r[1], what="spatial_features_point_2d")

    def nerr(x, ref):
        return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-300))
    # Gradients come out of a 25-layer chain of train-mode BatchNorm backward passes on a sparse canvas — an ill-conditioned
    # chain: torch's fp32 kernels land between 4e-4 and 3.5e-3 (median) of float64 on it depending on the solvers MIOpen picks, and
    # at 9.6e-4 (median) .. 6.7e-3 (max) on torch's native convolutions, the yardstick used here.  Norm-wise bounds: 5e-3 for
    # parameter gradients, 1e-2 for the canvas gradients at the far end of the chain, never worse than 3x torch fp32.  The
    # element-wise 1e-3 parity of every single operator is in the tests above.
    rows = [(f"input grad {k}", nerr(gh, gr), nerr(gt, gr)) for k, (gh, gt, gr) in enumerate(zip(h[2], t[2], r[2]))]
    assert set(h[3]) == set(r[3])
    for k in r[3]:
        assert h[3][k] is not None, k
        if float(r[3][k].norm()) < 1e-9 * float(r[3][k].numel()) ** 0.5:
            # a bias in front of a train-mode BatchNorm: its exact gradient is zero, fp32 leaves round-off on both sides
            assert float(h[3][k].abs().max()) < 1e-5, k
            continue
        rows.append(("grad " + k, nerr(h[3][k], r[3][k]), nerr(t[3][k], r[3][k])))
    eh, et = np.array([x[1] for x in rows]), np.array([x[2] for x in rows])
    print("backbone training parity vs float64 (norm-wise): own kernels median %.2e max %.2e | torch fp32 median %.2e max %.2e" %
          (np.median(eh), eh.max(), np.median(et), et.max()))
    for name, a_, b_ in sorted(rows, key=lambda x: -x[1])[:5]:
        print("   %-55s own %.2e torch %.2e" % (name, a_, b_))
    # a ReLU network in fp32: any two implementations disagree on a few of the millions of ReLU decisions (a pre-activation within
    # round-off of zero), and every flipped decision moves the gradients behind it by a finite amount.  Each operator on its own is
    # at fp32 round-off of float64 (1e-7 .. 1e-6 norm-wise, tools/train_precision_probe.py — the same as torch fp32); on this
    # 25-layer chain torch's native fp32 kernels sit at 9.6e-4 (median) .. 6.7e-3 (max) of float64.  The bar: the same regime as torch
    # fp32 — within 3x of its median and of its maximum — and no tensor beyond 3e-2.
    assert np.median(eh) < 3 * np.median(et) + 1e-3, (np.median(eh), np.median(et))
    assert eh.max() < 3 * et.max() + 2e-3 and eh.max() < 3e-2, (eh.max(), et.max())
    for k in r[4]:          # running statistics, incl. the shared SFM / gate BatchNorms updated once per call
        _close(h[4][k].float(), r[4][k].float(), rtol=1e-4, what="buffer " + k)


def test_packed_filter_cache_follows_the_weights():
    """conv_train keeps the packed Winograd filters of a parameter between calls: an in-place update (version counter), a write behind
    torch's back announced by weights_changed() (the flat fused optimiser), a re-pointed .data and a NEW tensor must all be seen."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 9, 11, 64, generator=g).to(DEV)
    w = torch.nn.Parameter((torch.randn(64, 64, 3, 3, generator=g) / 24).to(DEV))

    def ref(wt):
        return F.conv2d(x.permute(0, 3, 1, 2).double(), wt.detach().double(), padding=1).permute(0, 2, 3, 1)
    _close(ct.conv(x, w, 1), ref(w), rtol=2e-5, what="first call")
    _close(ct.conv(x, w, 1), ref(w), rtol=2e-5, what="cached call")
    with torch.no_grad():
        w.mul_(-0.5)                                            # version counter
    _close(ct.conv(x, w, 1), ref(w), rtol=2e-5, what="after an in-place update")
    w2 = w.detach().clone() * 3.0
    torch.cuda.synchronize()
    import ctypes
    ver = w._version
    hip = ctypes.CDLL("libamdhip64.so")                          # a write the version counter does not see (the fused optimiser's kind)
    assert hip.hipMemcpy(ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(w2.data_ptr()), ctypes.c_size_t(w.numel() * 4), 3) == 0
    torch.cuda.synchronize()
    assert w._version == ver and torch.equal(w.detach(), w2)
    ct.weights_changed()
    _close(ct.conv(x, w, 1), ref(w), rtol=2e-5, what="after a raw write + weights_changed()")
    w.data = (w.detach() * 0.25 + 0.01).clone()                 # same object, new storage
    _close(ct.conv(x, w, 1), ref(w), rtol=2e-5, what="after re-pointing .data")
    for _ in range(3):                                          # new tensors, possibly at a recycled address
        wn = torch.nn.Parameter((torch.randn(64, 64, 3, 3, generator=g) / 24).to(DEV))
        _close(ct.conv(x, wn, 1), ref(wn), rtol=2e-5, what="a new parameter")
        del wn


@pytest.mark.parametrize("N,H,W,Cs", [(2, 31, 45, (128, 128, 128)), (1, 9, 7, (32, 64, 16)), (3, 5, 6, (256,))])
def test_bn_relu_cat_equals_the_concatenation_of_bn_relu(N, H, W, Cs):
    """bn_relu_cat (every branch normalised into / differentiated out of its channel slice) against torch.cat of the plain bn_relu
    calls: output, running statistics and all gradients bit for bit — the same kernels on the same values, only the addresses differ."""
    g = torch.Generator().manual_seed(H * 3 + len(Cs))
    zs = [(torch.randn(N, H, W, C, generator=g) * 1.5 + 0.2).to(DEV) for C in Cs]
    def make():
        bns = [torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV).train() for C in Cs]
        gg = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for bn in bns:
                bn.weight.copy_(torch.rand(bn.weight.shape, generator=gg) + 0.5); bn.bias.copy_(torch.randn(bn.bias.shape, generator=gg) * 0.1)
        return bns
    bns_a, bns_b = make(), make()
    za = [z.clone().requires_grad_(True) for z in zs]
    zb = [z.clone().requires_grad_(True) for z in zs]
    ya = ct.bn_relu_cat(za, bns_a)
    yb = torch.cat([ct.bn_relu(z, bn) for z, bn in zip(zb, bns_b)], dim=-1)
    assert torch.equal(ya, yb)
    dy = torch.randn(ya.shape, generator=g).to(DEV)
    pa = [p for bn in bns_a for p in (bn.weight, bn.bias)]
    pb = [p for bn in bns_b for p in (bn.weight, bn.bias)]
    ga = torch.autograd.grad(ya, za + pa, dy)
    gb = torch.autograd.grad(yb, zb + pb, dy)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    for a, b in zip(bns_a, bns_b):
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 1


@pytest.mark.parametrize("shape", [(2, 40, 48, 128), (1, 31, 45, 256), (2, 9, 7, 512), (3, 5, 6, 32)])
def test_bn_relu_with_fused_sfm_gate_matches_torch(shape):
    """gate * relu(BN_train(z)) + resid in one forward / one backward kernel pair (the SFM step, base_bev_backbone.py:250-255):
    output and the gradients of z, gamma, beta, gate and resid vs torch autograd."""
    g = torch.Generator().manual_seed(shape[2])
    C = shape[-1]
    z = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(DEV).requires_grad_(True)
    gate = torch.rand(shape[:3] + (1,), generator=g).to(DEV).requires_grad_(True)
    resid = torch.randn(shape, generator=g).to(DEV).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5); bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    ref = copy.deepcopy(bn)
    y = ct.bn_relu(z, bn, gate=gate, resid=resid)
    zr, gr, rr = (t.detach().clone().requires_grad_(True) for t in (z, gate, resid))
    yr = gr * torch.relu(ref(zr.permute(0, 3, 1, 2))).permute(0, 2, 3, 1) + rr
    _close(y, yr, what="forward")
    dy = torch.randn(shape, generator=g).to(DEV)
    got = torch.autograd.grad(y, (z, bn.weight, bn.bias, gate, resid), dy)
    want = torch.autograd.grad(yr, (zr, ref.weight, ref.bias, gr, rr), dy)
    for a_, b_, what in zip(got, want, ("dz", "dgamma", "dbeta", "dgate", "dresid")):
        _close(a_, b_, what=what)


def test_packed_filter_cache_debug_check_catches_a_write_behind_torchs_back(monkeypatch):
    """conv_train keeps packed filters per (parameter object, version, data pointer).  A write through `.data` keeps all three: without
    conv_train.weights_changed() the cached image is stale.  With HVPR_DEBUG_PACK_CACHE=1 every hit re-checks a checksum of the weight:
    a silent stale-weights forward becomes an error; an announced write (weights_changed) and a versioned in-place write pass."""
    import torch
    from hvpr_amd import conv_train as ct
    monkeypatch.setattr(ct, "_DEBUG_PACK_CACHE", True)
    ct.weights_changed()
    w = torch.nn.Parameter(torch.randn(64, 32, 3, 3, device="cuda:0") * 0.1)
    x = torch.randn(1, 24, 40, 32, device="cuda:0")
    y0 = ct.conv_fwd_raw(x, w)
    assert torch.equal(ct.conv_fwd_raw(x, w), y0)                      # hit, checksum agrees
    w.data.mul_(2.0)                                                    # behind torch's back: same object, version, pointer
    import pytest
    with pytest.raises(RuntimeError, match="stale"):
        ct.conv_fwd_raw(x, w)
    ct.weights_changed()                                                # announced: re-packed
    torch.testing.assert_close(ct.conv_fwd_raw(x, w), 2.0 * y0, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        w.mul_(0.5)                                                     # versioned in-place write: detected by the version
    torch.testing.assert_close(ct.conv_fwd_raw(x, w), y0, rtol=1e-5, atol=1e-6)
    # entries go with their tensors
    n0 = len(ct._wino_pack_cache)
    for _ in range(5):
        ct.conv_fwd_raw(x, torch.randn(64, 32, 3, 3, device="cuda:0"))
    assert len(ct._wino_pack_cache) <= n0 + 1
