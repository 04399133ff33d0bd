"""The direct fp32 convolution kernels (hvpr_conv2d_nhwc_f32, hvpr_conv2d_s2_dgrad_nhwc_f32, hvpr_conv2d_wgrad_nhwc_f32) against
float64 at their edges, element by element inside the derived rounding bound of conv_direct_cases.py: no element excluded, no
tolerance added.  test_conv_direct_host.py shows on the CPU that an honest fp32 convolution uses a small part of that bound and
that a lost chunk, tile or single product falls outside it.  Every test reports max(err / bound) under "observed margins"."""
import pytest
import torch

import conv_direct_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status


def _d(t):
    return None if t is None else t.to(DEV)


def _pack(op, cfg):
    from hvpr_amd import kernels
    if isinstance(op, C.Deconv):
        return kernels.pack_deconv(_d(op.w), _d(op.scale), _d(op.shift), relu=op.relu, tile_cfg=cfg)
    return kernels.pack_conv(_d(op.w), _d(op.scale), _d(op.shift), stride=op.stride, relu=op.relu, tile_cfg=cfg)


def _run(op, cfg, sliced):
    """The op through kernels.conv2d_nhwc at one tile configuration -> (N,OH,OW,cout) on the CPU; sliced: written at SLICE_OFF
    into a tensor SLICE_EXTRA channels wider that must keep its sentinel on both sides."""
    from hvpr_amd import kernels
    pc = _pack(op, cfg)
    kw = dict(gate=_d(getattr(op, "gate", None)), resid=_d(getattr(op, "resid", None)))
    if not sliced:
        return kernels.conv2d_nhwc(_d(op.x), pc, **kw).cpu()
    N, H, W = op.x.shape[:3]
    OH, OW = (H * op.s, W * op.s) if isinstance(op, C.Deconv) else (op.OH, op.OW)
    wide = torch.full((N, OH, OW, op.cout + C.SLICE_EXTRA), C.SENTINEL, device=DEV)
    kernels.conv2d_nhwc(_d(op.x), pc, out=wide, out_coff=C.SLICE_OFF, **kw)
    wide = wide.cpu()
    lo, hi = C.SLICE_OFF, C.SLICE_OFF + op.cout
    assert bool((wide[..., :lo] == C.SENTINEL).all()) and bool((wide[..., hi:] == C.SENTINEL).all()), (op.dims, cfg, "sentinel")
    return wide[..., lo:hi]


def _all_cfgs(op, sliced, cfgs=C.TILE_CFGS):
    ref, S = op.reference()
    worst = 0.0
    for cfg in cfgs:
        frac = C.used_fraction(_run(op, cfg, sliced), ref, S, op.K)
        assert frac <= 1.0, (op.dims, "tile_cfg", cfg, frac)
        worst = max(worst, frac)
    return worst


@pytest.mark.parametrize("row", C.FWD3x3, ids=str)
def test_conv3x3_within_the_bound(row, observed):
    observed(f"conv direct 3x3 {row}: max err / bound {_all_cfgs(C.Fwd(*row, k=3), False):.4f} over tile_cfg 0, 1, 2")


@pytest.mark.parametrize("row", C.FWD1x1, ids=str)
def test_conv1x1_within_the_bound(row, observed):
    observed(f"conv direct 1x1 {row}: max err / bound {_all_cfgs(C.Fwd(*row, stride=1, k=1), False):.4f} over tile_cfg 0, 1, 2")


@pytest.mark.parametrize("variant", list(C.EPILOGUES))
@pytest.mark.parametrize("row", C.EPILOGUE_ROWS, ids=str)
def test_epilogue_variants_within_the_bound(row, variant, observed):
    kw, sliced = C.EPILOGUES[variant]
    op = C.Fwd(*row[:6], k=row[6], **kw)
    if op.gate is not None:
        assert op.resid.shape[-1] == op.cout + 12 and op.gate.shape == (row[0], op.OH, op.OW)
    observed(f"conv direct epilogue {variant} {row}: max err / bound {_all_cfgs(op, sliced):.4f} over tile_cfg 0, 1, 2")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("row", C.DECONV, ids=str)
def test_deconv_within_the_bound(row, relu, observed):
    observed(f"conv direct deconv {row} relu={relu}: max err / bound {_all_cfgs(C.Deconv(*row, relu=relu), True):.4f} over tile_cfg 0, 1, 2")


@pytest.mark.parametrize("row", C.WALK, ids=str)
def test_persistent_walk_within_the_bound(row, observed):
    """4096 tiles of 8 x 8 pixels: every workgroup of the persistent grid walks several, border and interior in turn."""
    observed(f"conv direct walk {row}: max err / bound {_all_cfgs(C.Fwd(*row[:6], k=row[6]), False, cfgs=(C.WALK_CFG,)):.4f}")


@pytest.mark.parametrize("row", C.S2DGRAD, ids=str)
def test_s2_dgrad_within_the_bound(row, observed):
    from hvpr_amd import kernels
    op = C.S2Dgrad(*row)
    ref, S = op.reference()
    dx = kernels.conv2d_s2_dgrad_nhwc(_d(op.dz), _d(op.w), op.H, op.W).cpu()
    frac = C.used_fraction(dx, ref, S, op.K)
    observed(f"conv direct s2 dgrad {row}: max err / bound {frac:.4f}")
    assert frac <= 1.0, (row, frac)


def test_conv_backward_zero_upsample_form_within_the_bound(observed, monkeypatch):
    """conv_train.conv at stride 2 with 12 output channels: the data gradient cannot take the parity-class gather (cout % 8 != 0) and
    runs as a stride-1 convolution over the zero-upsampled gradient."""
    from hvpr_amd import conv_train, kernels

    def gather(*a, **k):
        raise AssertionError("the parity-class gather ran: this test is about _Conv.backward's zero-upsample form")
    monkeypatch.setattr(kernels, "conv2d_s2_dgrad_nhwc", gather)
    N, H, W, ci, co, s = C.CONV_BACKWARD
    fwd, dgrad, wgrad = C.families()["conv_backward"]
    assert co % 8 != 0
    fracs = {}                  # (the three rows have inputs of their own: one forward / backward each, zeros where a row has no say)
    for name, op, x, w, dz in (("y", fwd, fwd.x, fwd.w, None), ("dx", dgrad, None, dgrad.w, dgrad.dz), ("dw", wgrad, wgrad.x, None, wgrad.dz)):
        xg = _d(x if x is not None else torch.zeros(N, H, W, ci)).requires_grad_(True)
        wg = _d(w if w is not None else torch.zeros(co, ci, 3, 3)).requires_grad_(True)
        y = conv_train.conv(xg, wg, stride=s)
        if dz is not None:
            y.backward(_d(dz))
        got = {"y": y.detach(), "dx": xg.grad, "dw": wg.grad}[name].cpu()
        ref, S = op.reference()
        fracs[name] = C.used_fraction(got, ref, S, op.K)
    observed("conv direct _Conv backward (2,5,7,8,12,s2): max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fracs.items()))
    assert max(fracs.values()) <= 1.0, fracs


@pytest.mark.parametrize("row", C.WGRAD, ids=str)
def test_wgrad_within_the_bound(row, observed, monkeypatch):
    from hvpr_amd import conv_train
    from hvpr_amd._lib import lib
    monkeypatch.setenv("HVPR_CONV_ALGO", "direct")
    op = C.Wgrad(*row)
    N, H, W, ci, co, taps, s = row
    OH, OW = op.dz.shape[1:3]
    assert lib().hvpr_conv2d_wgrad_workspace_bytes(N, OH, OW, ci, co, taps, s) == op.n_chunks * taps * co * ci * 4   # the K of the bound
    x, dz = _d(op.x), _d(op.dz)
    dw = conv_train.conv_wgrad(x, dz, taps, s, co, ci)
    again = conv_train.conv_wgrad(x, dz, taps, s, co, ci)
    assert torch.equal(dw, again), "the split-K reduction is not deterministic"
    ref, S = op.reference()
    frac = C.used_fraction(dw.cpu(), ref, S, op.K)
    observed(f"conv direct wgrad {row} ({op.n_chunks} chunks): max err / bound {frac:.4f}")
    assert frac <= 1.0, (row, frac)


@pytest.mark.parametrize("row", C.DECONV_TRAIN, ids=str)
def test_deconv_train_within_the_bound(row, observed):
    from hvpr_amd import conv_train
    fwd, gdx, gdw = C.Deconv(*row, fold=False), C.DeconvGrad(*row, "dx"), C.DeconvGrad(*row, "dw")
    y = conv_train.deconv(_d(fwd.x), _d(fwd.w)).cpu()
    xg, wg = _d(gdx.x).requires_grad_(True), _d(gdx.w).requires_grad_(True)       # (dx and dw rows share their inputs)
    assert torch.equal(gdx.x, gdw.x) and torch.equal(gdx.dy, gdw.dy)
    conv_train.deconv(xg, wg).backward(_d(gdx.dy))
    fracs = {}
    for name, op, got in (("y", fwd, y), ("dx", gdx, xg.grad.cpu()), ("dw", gdw, wg.grad.cpu())):
        ref, S = op.reference()
        fracs[name] = C.used_fraction(got, ref, S, op.K)
    observed(f"conv direct deconv train {row}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fracs.items()))
    assert max(fracs.values()) <= 1.0, fracs


# ------------------------------------------------------------------------------------------------ refusals
# Every buffer is far larger than any launch these small dimensions could address, rounded-up channel counts included, so a missing
# refusal would show as a wrong status and a changed sentinel, not as a write outside a buffer.
class _Buffers:
    def __init__(self):
        self.src = torch.randn(1 << 16, device=DEV)              # input / gradient images
        self.w = torch.randn(1 << 18, device=DEV)                # packed weights (9 taps x 2 chunks x 2 x 128 x 4 = 18432 floats at most)
        self.bias = torch.randn(1 << 10, device=DEV)
        self.gate = torch.rand(1 << 12, device=DEV)
        self.resid = torch.randn(1 << 16, device=DEV)
        self.ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        self.out = torch.full((1 << 16,), C.SENTINEL, device=DEV)

    def untouched(self):
        return bool((self.out.cpu() == C.SENTINEL).all())


@pytest.fixture(scope="module")
def bufs():
    return _Buffers()


_CONV_OK = dict(N=1, H=4, W=4, Cin=8, taps=9, stride=1, cout=4, cout_pad=64, up=1, relu=0, gate=False, resid=False, resid_cstride=0,
                out_cstride=8, out_coff=0, tile_cfg=1)


def _conv_call(b, **over):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    a = dict(_CONV_OK, **over)
    return lib().hvpr_conv2d_nhwc_f32(b.src.data_ptr(), a["N"], a["H"], a["W"], a["Cin"], b.w.data_ptr(), b.bias.data_ptr(), a["taps"], a["stride"],
                                      a["cout"], a["cout_pad"], a["up"], a["relu"], b.gate.data_ptr() if a["gate"] else None,
                                      b.resid.data_ptr() if a["resid"] else None, a["resid_cstride"], b.out.data_ptr(), a["out_cstride"],
                                      a["out_coff"], a["tile_cfg"], kernels._stream())


_GATED = dict(gate=True, resid=True, resid_cstride=8)
CONV_REFUSALS = {
    "cin_not_multiple_of_8": (dict(Cin=12), UNSUPPORTED),
    "taps_4": (dict(taps=4), UNSUPPORTED),
    "stride_3": (dict(stride=3), UNSUPPORTED),
    "1x1_at_stride_2": (dict(taps=1, stride=2), UNSUPPORTED),
    "up_with_9_taps": (dict(up=2), UNSUPPORTED),
    "up_with_gate": (dict(taps=1, up=2, **_GATED), UNSUPPORTED),
    "gate_without_residual": (dict(gate=True), INVALID),
    "residual_without_gate": (dict(resid=True, resid_cstride=8), INVALID),
    "cout_not_multiple_of_4": (dict(cout=6), UNSUPPORTED),
    "out_cstride_not_multiple_of_4": (dict(out_cstride=10), UNSUPPORTED),
    "out_coff_not_multiple_of_4": (dict(out_cstride=16, out_coff=2), UNSUPPORTED),
    "resid_cstride_not_multiple_of_4": (dict(_GATED, resid_cstride=6), UNSUPPORTED),
    "cout_pad_below_cout": (dict(cout=68, out_cstride=68), INVALID),
    "cout_pad_below_deconv_columns": (dict(taps=1, up=2, cout=20, out_cstride=20), INVALID),      # 80 live columns
    "cout_pad_not_multiple_of_128_tile": (dict(tile_cfg=0, cout_pad=64), INVALID),
    "cout_pad_not_multiple_of_64_tile": (dict(tile_cfg=2, cout_pad=96), INVALID),
    "tile_cfg_3": (dict(tile_cfg=3), INVALID),
}


def test_conv_accepts_the_base_call(bufs):
    """The call every refusal below is one step away from is accepted and writes: a refusal cannot pass because the template is wrong."""
    for over in (dict(), dict(taps=1), dict(taps=1, up=2), _GATED, dict(stride=2), dict(tile_cfg=0, cout_pad=128), dict(tile_cfg=2)):
        bufs.out.fill_(C.SENTINEL)
        assert _conv_call(bufs, **over) == OK, over
        assert not bufs.untouched(), over
    bufs.out.fill_(C.SENTINEL)


@pytest.mark.parametrize("name", list(CONV_REFUSALS))
def test_conv_refuses(name, bufs):
    over, status = CONV_REFUSALS[name]
    bufs.out.fill_(C.SENTINEL)
    assert _conv_call(bufs, **over) == status
    assert bufs.untouched()


def _s2_call(b, H=2, W=2, Cin=8, cout=4, cout_pad=64, OH=4, OW=4):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    return lib().hvpr_conv2d_s2_dgrad_nhwc_f32(b.src.data_ptr(), 1, H, W, Cin, b.w.data_ptr(), b.bias.data_ptr(), cout, cout_pad, OH, OW,
                                               b.out.data_ptr(), 8, 0, kernels._stream())


@pytest.mark.parametrize("over,status", [(dict(H=3), INVALID), (dict(W=1), INVALID), (dict(cout_pad=96), UNSUPPORTED)], ids=str)
def test_s2_dgrad_refuses(over, status, bufs):
    bufs.out.fill_(C.SENTINEL)
    assert _s2_call(bufs) == OK and not bufs.untouched()
    bufs.out.fill_(C.SENTINEL)
    assert _s2_call(bufs, **over) == status
    assert bufs.untouched()


def _wgrad_call(b, Cin=8, Cout=8, taps=9, stride=1, short=0):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    N, H, W = 2, 4, 4
    OH, OW = C.out_hw(H, W, stride, 3 if taps == 9 else 1)
    need = lib().hvpr_conv2d_wgrad_workspace_bytes(N, OH, OW, Cin, Cout, taps, stride)
    assert 0 < need <= b.ws.numel()
    return lib().hvpr_conv2d_wgrad_nhwc_f32(b.src.data_ptr(), N, H, W, Cin, b.resid.data_ptr(), Cout, taps, stride, b.out.data_ptr(),
                                            b.ws.data_ptr(), need - short, kernels._stream())


@pytest.mark.parametrize("over,status", [(dict(Cin=6), UNSUPPORTED), (dict(Cout=6), UNSUPPORTED), (dict(taps=1, stride=2), UNSUPPORTED),
                                         (dict(short=1), WORKSPACE)], ids=str)
def test_wgrad_refuses(over, status, bufs):
    bufs.out.fill_(C.SENTINEL)
    assert _wgrad_call(bufs) == OK and not bufs.untouched()
    bufs.out.fill_(C.SENTINEL)
    assert _wgrad_call(bufs, **over) == status
    assert bufs.untouched()
