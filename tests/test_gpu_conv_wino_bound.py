"""The Winograd training kernels against float64, element by element inside the derived rounding bound of conv_wino_cases.py: the
weight gradient hvpr_conv2d_wino_wgrad_nhwc_f32 (k_wgrad_wino's tile pipeline at every depth, its channel and image edges, the
workspace contract, the refusals) and hvpr_conv2d_wino_nhwc_f32 as conv_train calls it, on plain and on adjoint-packed filters (the
data gradient).  No element is excluded and no tolerance added.  test_conv_wino_host.py shows on the CPU that honest fp32 arithmetic
uses a small part of the bound and that a lost tile, chunk, channel group, sign, flip or block term falls outside it.  Every test
reports max(err / bound) under "observed margins"."""
import pytest
import torch

import conv_wino_cases as C
from conv_direct_cases import SENTINEL, SLICE_EXTRA, SLICE_OFF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
TAIL = 4096                                                  # guard floats behind the workspace and behind dw


def _ops(family):
    return {op.dims: op for op in C.families()[family]}


def _wgrad_call(op, x, dz):
    """One direct call: the workspace is exactly the reported bytes, NaN all through, inside a buffer whose tail holds a sentinel; dw
    likewise ends in a sentinel tail.  -> dw (cout, cin, 3, 3) on the device."""
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    N, H, W, ci, co = op.dims
    need = lib().hvpr_conv2d_wino_wgrad_workspace_bytes(N, H, W, ci, co)
    assert need == op.n_chunks * 16 * co * ci * 4, (op.dims, need, op.n_chunks)          # n_chunks is part of the bound's n
    ws = torch.full((need // 4 + TAIL,), float("nan"), device=DEV)
    ws[need // 4:] = SENTINEL
    out = torch.full((co * ci * 9 + TAIL,), SENTINEL, device=DEV)
    status = lib().hvpr_conv2d_wino_wgrad_nhwc_f32(x.data_ptr(), N, H, W, ci, dz.data_ptr(), co, out.data_ptr(), ws.data_ptr(), need,
                                                   kernels._stream())
    assert status == OK, (op.dims, status)
    torch.cuda.synchronize()
    assert bool((ws[need // 4:] == SENTINEL).all()), (op.dims, "written past the reported workspace")
    assert bool((out[co * ci * 9:] == SENTINEL).all()), (op.dims, "written past dw")
    # every partial the reducer reads was written first: a NaN left in [n_chunks][16][Cout][Cin] would have reached dw
    assert not bool(torch.isnan(ws[:need // 4]).any()), (op.dims, "the workspace is not fully overwritten")
    return out[:co * ci * 9].reshape(co, ci, 3, 3).clone()


@pytest.mark.parametrize("family,row", [("wgrad_pipe", r) for r in C.WGRAD_PIPE] + [("wgrad_edge", r) for r in C.WGRAD_EDGE], ids=str)
def test_wino_wgrad_within_the_bound(family, row, observed, monkeypatch):
    from hvpr_amd import conv_train
    monkeypatch.delenv("HVPR_CONV_ALGO", raising=False)
    op = _ops(family)[row]
    N, H, W, ci, co = row
    x, dz = op.x.to(DEV), op.dz.to(DEV)
    dw = _wgrad_call(op, x, dz)
    assert bool(torch.isfinite(dw).all()), row
    assert torch.equal(dw, _wgrad_call(op, x, dz)), "the split-K reduction is not deterministic"
    assert conv_train._wino_wgrad_fits(H, W, ci, co)
    assert torch.equal(dw, conv_train.conv_wgrad(x, dz, 9, 1, co, ci)), "conv_train.conv_wgrad gives other bits than the direct call"
    ref, S = op.reference()
    op._cache.clear()
    frac = C.used_fraction(dw.cpu(), ref, S, op.K)
    g = op.geo
    observed(f"conv wino wgrad {row} ({g['n_pt']} tiles, {g['n_chunks']} chunks, {g['tiles_min']}-{g['tiles_max']} tiles a workgroup, n = {op.n}): "
             f"max err / bound {frac:.4f}")
    assert frac <= 1.0, (row, frac)


def _sliced(x, pc, like, **kw):
    """The same launch into a channel slice of a wider tensor: the same bits, the sentinel channels on both sides kept."""
    from hvpr_amd import kernels
    cout = like.shape[-1]
    wide = torch.full(tuple(like.shape[:3]) + (cout + SLICE_EXTRA,), SENTINEL, device=DEV)
    kernels.conv2d_wino_nhwc(x, pc, out=wide, out_coff=SLICE_OFF, **kw)
    lo, hi = SLICE_OFF, SLICE_OFF + cout
    assert bool((wide[..., :lo] == SENTINEL).all()) and bool((wide[..., hi:] == SENTINEL).all()), "sentinel"
    assert torch.equal(wide[..., lo:hi], like), "the sliced launch gives other bits"


def _no_direct_kernel(monkeypatch):
    from hvpr_amd import kernels

    def direct(*a, **k):
        raise AssertionError("the direct kernel ran: this test is about the Winograd kernel")
    monkeypatch.delenv("HVPR_CONV_ALGO", raising=False)
    monkeypatch.setattr(kernels, "conv2d_nhwc", direct)


@pytest.mark.parametrize("row", C.DGRAD_WINO, ids=str)
def test_wino_dgrad_within_the_bound(row, observed, monkeypatch):
    """conv_fwd_raw(dz, w, 1, adjoint=True): k_wino_pack's w[i][o][2-u][2-v] indexing and the forward kernel on a non-square layer
    whose output channels are padded to 64, on ragged images that pair their edge tiles and on one that cannot."""
    from hvpr_amd import conv_train, kernels
    from hvpr_amd._lib import lib
    _no_direct_kernel(monkeypatch)
    N, H, W, cin_w, cout_w = row
    op = C.dgrad_op(row)
    assert tuple(op.w.shape) == (cout_w, cin_w, 3, 3) and op.x.shape[-1] == cout_w
    w, dz = op.w.to(DEV), op.x.to(DEV)
    assert conv_train._winograd(w, 1, adjoint=True)
    tiles = N * -(-H // C.TH) * -(-W // C.TW) * -(-cin_w // 64)
    assert (lib().hvpr_conv2d_wino_items(N, H, W, cin_w, conv_train._wino_groups()) < tiles) == C.DGRAD_PAIRS[row]
    pc = conv_train._pack_wino(w, True)
    assert (pc.cin, pc.cout) == (cout_w, cin_w)
    if row in C.DGRAD_SFM:               # _SfmStep.backward: 1 * conv_adjoint(dz) + dy
        kw = dict(gate=conv_train._ones((N, H, W), dz.device), resid=op.resid.to(DEV))
        dx = kernels.conv2d_wino_nhwc(dz, pc, **kw)
    else:
        kw = {}
        dx = conv_train.conv_fwd_raw(dz, w, 1, adjoint=True)
    _sliced(dz, pc, dx, **kw)
    ref, S = op.reference()
    frac = C.used_fraction(dx.cpu(), ref, S, op.K)
    observed(f"conv wino dgrad {row} (n = {op.n}): max err / bound {frac:.4f}")
    assert frac <= 1.0, (row, frac)


@pytest.mark.parametrize("row", C.FWD_TRAIN, ids=str)
def test_wino_train_forward_within_the_bound(row, observed, monkeypatch):
    """conv_fwd_raw(x, w, 1) and its stats=True form: the same bits, and per-tile sums that are the sums of that output."""
    from hvpr_amd import conv_train
    from hvpr_amd._lib import lib
    _no_direct_kernel(monkeypatch)
    N, H, W, cin, cout = row
    op = C.FwdWino(*row, sparse=row in C.FWD_SPARSE)
    x, w = op.x.to(DEV), op.w.to(DEV)
    z = conv_train.conv_fwd_raw(x, w, 1)
    zs, part = conv_train.conv_fwd_raw(x, w, 1, stats=True)
    assert torch.equal(zs, z), "the statistics launch gives other bits"
    assert part is not None and tuple(part.shape) == (lib().hvpr_conv2d_wino_stats_rows(N, H, W), 2, cout)
    assert bool(torch.isfinite(part).all())
    # a tile's fp32 sum is a chain of at most 32 + 3 additions (and one rounding of the square): |error| <= 36 * 2^-24 * sum |v|
    zd = z.double()
    s1, s2, a1 = zd.sum((0, 1, 2)), (zd ** 2).sum((0, 1, 2)), zd.abs().sum((0, 1, 2))
    e1, e2 = (part[:, 0].double().sum(0) - s1).abs(), (part[:, 1].double().sum(0) - s2).abs()
    assert bool((e1 <= 36 * C.U * a1).all()) and bool((e2 <= 37 * C.U * s2).all()), (row, float((e1 / a1).max()) / C.U, float((e2 / s2).max()) / C.U)
    _sliced(x, conv_train._pack_wino(w, False), z)
    ref, S = op.reference()
    frac = C.used_fraction(z.cpu(), ref, S, op.K)
    observed(f"conv wino train forward {row} (n = {op.n}): max err / bound {frac:.4f}; statistics use "
             f"{float((e1 / (36 * C.U * a1)).max()):.3f} / {float((e2 / (37 * C.U * s2)).max()):.3f} of their bounds")
    assert frac <= 1.0, (row, frac)


# ------------------------------------------------------------------------------------------------ refusals
# Every buffer is far larger than any launch these small dimensions could address, so a missing refusal would show as a wrong status
# and a changed sentinel, not as a write outside a buffer.
class _Buffers:
    def __init__(self):
        self.x = torch.randn(1 << 16, device=DEV)
        self.dz = torch.randn(1 << 16, device=DEV)
        self.ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        self.out = torch.full((1 << 16,), SENTINEL, device=DEV)

    def untouched(self):
        return bool((self.out.cpu() == SENTINEL).all())


@pytest.fixture(scope="module")
def bufs():
    return _Buffers()


def _refusal_call(b, Cin=8, Cout=8, short=0, null_ws=False):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    N, H, W = 2, 4, 4
    need = lib().hvpr_conv2d_wino_wgrad_workspace_bytes(N, H, W, Cin, Cout)
    assert 0 < need <= b.ws.numel()
    return lib().hvpr_conv2d_wino_wgrad_nhwc_f32(b.x.data_ptr(), N, H, W, Cin, b.dz.data_ptr(), Cout, b.out.data_ptr(),
                                                 None if null_ws else b.ws.data_ptr(), need - short, kernels._stream())


@pytest.mark.parametrize("over,status", [(dict(Cin=6), UNSUPPORTED), (dict(Cout=6), UNSUPPORTED), (dict(short=1), WORKSPACE),
                                         (dict(null_ws=True), INVALID)], ids=str)
def test_wino_wgrad_refuses(over, status, bufs):
    bufs.out.fill_(SENTINEL)
    assert _refusal_call(bufs) == OK and not bufs.untouched()          # the call each refusal is one step away from is accepted and writes
    bufs.out.fill_(SENTINEL)
    assert _refusal_call(bufs, **over) == status
    assert bufs.untouched()


@pytest.mark.parametrize("H,W,cin,cout", [
    (1, 1 << 27, 4, 4), (1, (1 << 27) - 1, 4, 4),                 # H W C 4 = 2^31 and one pixel less
    (1 << 13, 1 << 14, 4, 4), ((1 << 13) - 1, 1 << 14, 4, 4),
    (1, 1 << 20, 512, 4), (1, 1 << 20, 4, 512),                   # the larger channel count decides, whichever it is
    (1, 1 << 20, 508, 4), (1, 1 << 20, 4, 508), (1, 1 << 20, 508, 512),
    (248, 296, 128, 128), (1, 1, 4, 4),
])
def test_wino_wgrad_dispatch_is_the_kernels_own_size_check(H, W, cin, cout):
    """An image of 2 GB and more is refused by the kernel (32-bit offsets) and no device buffer could hold one here: conv_wgrad's
    dispatch condition is held to the kernel's expression on its boundary instead (no launch)."""
    from hvpr_amd import conv_train
    kernel_accepts = not (H * W * (cin if cin > cout else cout) * 4 >= (1 << 31))          # csrc/conv_wino_wgrad.hip, restated
    assert conv_train._wino_wgrad_fits(H, W, cin, cout) is kernel_accepts
    assert C.wgrad_fits(H, W, cin, cout) is kernel_accepts
