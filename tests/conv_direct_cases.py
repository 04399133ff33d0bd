"""Float64 references, the per-element rounding bound and the case tables of the direct fp32 convolution kernels
(csrc/conv_igemm.hip, csrc/conv_train.hip), shared by test_conv_direct_host.py (torch's fp32 CPU convolution stands in for the
kernel: the bound proves itself) and test_gpu_conv_direct.py (the kernels against the same bound).  Plain torch, no GPU.

The bound.  An output element whose exact value is a sum of K products plus an epilogue is computed with at most 2K + 4
roundings on its path: one per product and one per accumulate (a matrix-core step that rounds its two products separately from
the accumulate is covered), the bias add, the gate's fused multiply-add, and one to spare for the split-K / slice meetings of the
weight gradient, whose chunk count is part of its K.  The standard summation result (Higham, Accuracy and Stability of Numerical
Algorithms, §3.1, §4.2), valid for ANY order of summation, gives

    |got - ref| <= gamma(2K + 4) * S + K * 2**-126,     gamma(n) = n u / (1 - n u),  u = 2**-24

with S the same expression evaluated on absolute values in float64; the additive term covers a unit that flushes a subnormal
product or partial sum to zero (each of the K terms loses at most the smallest normal number).  ReLU is 1-Lipschitz, so it is
applied to both sides after the bound is formed.  Nothing here is fitted to what a kernel returns.

The float64 side widens exactly the fp32 numbers the kernel is handed: a folded layer's weight is weight.float() * scale in fp32,
the way kernels.pack_conv / pack_deconv form it, THEN widened, so the fold's own rounding is not part of the error."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def bound(K, S):
    return gamma(2 * K + 4) * S + K * 2.0 ** -126


def used_fraction(got, ref, S, K):
    """max over ALL elements of |got - ref| / bound: <= 1 means inside the bound everywhere.  Only an exact match counts as 0 (0 / 0
    included); an element that is not a number, infinite, or off where the bound is zero counts as inf."""
    err = (got.double() - ref).abs()
    b = bound(K, S)
    assert err.shape == b.shape, (err.shape, b.shape)
    frac = torch.where(err == 0, torch.zeros_like(err), err / b)
    frac = torch.where(torch.isnan(frac), torch.full_like(frac, float("inf")), frac)       # (max() would not see a NaN reliably)
    return float(frac.max()) if frac.numel() else 0.0


def caught_share(ref, S, bad, S_bad, K):
    """Share of the elements a lost term touches (their absolute sum shrank) on which `bad` is outside the bound around `ref`."""
    touched = (S - S_bad) > 1e-12 * S
    assert bool(touched.any()), "the lost term touches no element"
    out = ~((bad - ref).abs() <= bound(K, S))          # "not inside": a NaN is outside
    return float(out[touched].double().mean())


def _seed(*row):
    return int(sum((v + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


def _cast(dt, absval):
    return (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def out_hw(H, W, stride, k):
    return ((H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1) if k == 3 else (H, W)


def wgrad_chunks(N, OH, OW, cin, cout, taps, stride):
    """The split-K chunk count of hvpr_conv2d_wgrad_nhwc_f32 (csrc/conv_train.hip wgrad_chunks), restated: the GPU test pins it
    against hvpr_conv2d_wgrad_workspace_bytes."""
    th, tw = (8 if taps == 9 and stride == 1 else 4), 8
    n_pt = N * (-(-OH // th)) * (-(-OW // tw))
    few = taps == 1 and cout <= 32 and cin > 256
    bm = 32 if few else (64 if taps == 9 else 128)
    bn = 384 if few else bm
    n_ot = (-(-cin // bn)) * (-(-cout // bm))
    return max(1, min(-(-512 // n_ot), n_pt))


def wgrad_tile(taps, stride):
    return (8 if taps == 9 and stride == 1 else 4), 8


class Op:
    """One case: its fp32 inputs, K, and `_eval(dtype, absval, drop)` = the operation in plain torch at `dtype`, on absolute values
    for S, with the term `drop` names removed (the lost-term variants)."""
    drops = {}

    def reference(self, drop=None):
        """-> (ref, S) in float64."""
        d = None if drop is None else self.drops[drop]
        return self._eval(torch.float64, False, d), self._eval(torch.float64, True, d)

    def standin(self):
        """torch's own fp32 CPU kernels on the same fp32 inputs."""
        return self._eval(torch.float32, False, None)


class Fwd(Op):
    """hvpr_conv2d_nhwc_f32 with up == 1: kxk (pad (k-1)/2) convolution, folded scale (fold) + bias, ReLU, gate * y + resid with the
    residual 12 channels wider than cout (gate and residual at output resolution)."""

    def __init__(self, N, H, W, cin, cout, stride=1, k=3, relu=False, bias=True, gated=False, fold=True):
        g = torch.Generator().manual_seed(_seed(N, H, W, cin, cout, stride, k))
        self.dims = (N, H, W, cin, cout, stride, k)
        self.cin, self.cout, self.stride, self.k, self.relu = cin, cout, stride, k, relu
        self.x = torch.randn(N, H, W, cin, generator=g)
        self.w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
        self.scale = torch.rand(cout, generator=g) + 0.5 if fold else None
        shift = torch.randn(cout, generator=g) * 0.3
        self.shift = shift if bias else None
        self.OH, self.OW = out_hw(H, W, stride, k)
        gate = torch.rand(N, self.OH, self.OW, generator=g) * 1.5 - 0.25
        resid = torch.randn(N, self.OH, self.OW, cout + 12, generator=g)
        self.gate, self.resid = (gate, resid) if gated else (None, None)
        self.K = k * k * cin
        c = k // 2                      # the centre tap touches every output pixel
        self.drops = {"chunk": (slice(None), slice(cin - 8, cin), c, c), "single": (slice(None), cin - 1, c, c)}

    def folded(self):
        return self.w.float() * self.scale.view(-1, 1, 1, 1) if self.scale is not None else self.w.float()

    def _eval(self, dt, absval, drop):
        f = _cast(dt, absval)
        wf = self.folded().clone()
        if drop is not None:
            wf[drop] = 0
        z = _nhwc(F.conv2d(_nchw(f(self.x)), f(wf), stride=self.stride, padding=self.k // 2))
        if self.shift is not None:
            z = z + f(self.shift)
        if self.relu and not absval:
            z = torch.relu(z)
        if self.gate is not None:
            z = f(self.gate).unsqueeze(-1) * z + f(self.resid[..., :self.cout])
        return z


class Deconv(Op):
    """ConvTranspose2d with kernel == stride == s (hvpr_conv2d_nhwc_f32 with up == s): K = cin products per output element."""

    def __init__(self, N, H, W, cin, cout, s, relu=False, fold=True):
        g = torch.Generator().manual_seed(_seed(N, H, W, cin, cout, s, 77))
        self.dims = (N, H, W, cin, cout, s)
        self.cin, self.cout, self.s, self.relu = cin, cout, s, relu
        self.x = torch.randn(N, H, W, cin, generator=g)
        self.w = torch.randn(cin, cout, s, s, generator=g) / math.sqrt(cin)
        self.scale = torch.rand(cout, generator=g) + 0.5 if fold else None
        self.shift = torch.randn(cout, generator=g) * 0.3 if fold else None
        self.K = cin
        self.drops = {"chunk": (slice(cin - 8, cin), slice(None), s - 1, s - 1), "single": (cin - 1, slice(None), s - 1, s - 1)}

    def folded(self):
        return self.w.float() * self.scale.view(1, -1, 1, 1) if self.scale is not None else self.w.float()

    def _eval(self, dt, absval, drop):
        f = _cast(dt, absval)
        wf = self.folded().clone()
        if drop is not None:
            wf[drop] = 0
        z = _nhwc(F.conv_transpose2d(_nchw(f(self.x)), f(wf), stride=self.s))
        if self.shift is not None:
            z = z + f(self.shift)
        if self.relu and not absval:
            z = torch.relu(z)
        return z


class S2Dgrad(Op):
    """Data gradient of a 3x3 stride-2 (pad 1) layer (N,H,W,cin) -> cout channels, by autograd: dz (N,OH,OW,cout) -> dx (N,H,W,cin).
    K = 4 * cout: the four-tap parity class is the worst."""

    def __init__(self, N, H, W, cin, cout):
        g = torch.Generator().manual_seed(_seed(N, H, W, cin, cout, 2, 55))
        self.dims = (N, H, W, cin, cout)
        self.N, self.H, self.W, self.cin, self.cout = N, H, W, cin, cout
        OH, OW = out_hw(H, W, 2, 3)
        self.dz = torch.randn(N, OH, OW, cout, generator=g)
        self.w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cout * 9)
        self.K = 4 * cout
        # the centre tap: the one-tap class of even rows and columns, present in every image
        self.drops = {"chunk": (slice(cout - 8, cout), slice(None), 1, 1), "single": (cout - 1, slice(None), 1, 1)}

    def _eval(self, dt, absval, drop):
        f = _cast(dt, absval)
        w = self.w.clone()
        if drop is not None:
            w[drop] = 0
        x0 = torch.zeros(self.N, self.cin, self.H, self.W, dtype=dt, requires_grad=True)
        y = F.conv2d(x0, f(w), stride=2, padding=1)
        (dx,) = torch.autograd.grad(y, x0, _nchw(f(self.dz)))
        return _nhwc(dx)


class Wgrad(Op):
    """Weight gradient of a kxk (pad (k-1)/2) layer by autograd: x (N,H,W,cin), dz (N,OH,OW,cout) -> dw (cout,cin,k,k).
    K = pixels + split-K chunks (every chunk's partial sum is one more term of the final sum).  drops: every product of one pixel tile
    of the kernel's walk ("chunk"), the products of one pixel ("single": each dw element loses one)."""

    def __init__(self, N, H, W, cin, cout, taps, stride):
        g = torch.Generator().manual_seed(_seed(N, H, W, cin, cout, taps, stride, 33))
        self.dims = (N, H, W, cin, cout, taps, stride)
        self.cin, self.cout, self.taps, self.stride, self.k = cin, cout, taps, stride, 3 if taps == 9 else 1
        OH, OW = out_hw(H, W, stride, self.k)
        self.x = torch.randn(N, H, W, cin, generator=g)
        self.dz = torch.randn(N, OH, OW, cout, generator=g)
        self.n_chunks = wgrad_chunks(N, OH, OW, cin, cout, taps, stride)
        self.K = N * OH * OW + self.n_chunks
        th, tw = wgrad_tile(taps, stride)
        self.drops = {"chunk": (N - 1, slice(0, th), slice(0, tw)), "single": (N - 1, min(1, OH - 1), min(1, OW - 1))}

    def _eval(self, dt, absval, drop):
        f = _cast(dt, absval)
        dz = self.dz.clone()
        if drop is not None:
            dz[drop] = 0
        w0 = torch.zeros(self.cout, self.cin, self.k, self.k, dtype=dt, requires_grad=True)
        y = F.conv2d(_nchw(f(self.x)), w0, stride=self.stride, padding=self.k // 2)
        (dw,) = torch.autograd.grad(y, w0, _nchw(f(dz)))
        return dw


class DeconvGrad(Op):
    """Gradients of the k == s ConvTranspose2d by autograd: x (N,H,W,cin), w (cin,cout,s,s), dy (N,H*s,W*s,cout).
    which = "dx": a 1x1 convolution over the s*s*cout space-to-depth columns, K = s*s*cout; "dw": the 1x1 weight gradient over
    (columns, cin), K = N*H*W + its split-K chunks."""

    def __init__(self, N, H, W, cin, cout, s, which):
        g = torch.Generator().manual_seed(_seed(N, H, W, cin, cout, s, 99))
        self.dims = (N, H, W, cin, cout, s, which)
        self.which, self.s = which, s
        self.x = torch.randn(N, H, W, cin, generator=g)
        self.w = torch.randn(cin, cout, s, s, generator=g) / math.sqrt(cin)
        self.dy = torch.randn(N, H * s, W * s, cout, generator=g)
        cols = s * s * cout
        if which == "dx":
            self.K = cols
            c8 = min(8, cout)
            self.drops = {"chunk": (slice(None), slice(cout - c8, cout), s - 1, s - 1), "single": (slice(None), cout - 1, s - 1, s - 1)}
        else:
            self.n_chunks = wgrad_chunks(N, H, W, cin, cols, 1, 1)
            self.K = N * H * W + self.n_chunks
            th, tw = wgrad_tile(1, 1)
            self.drops = {"chunk": (N - 1, slice(0, th * s), slice(0, tw * s)), "single": (N - 1, s - 1, s - 1)}

    def _eval(self, dt, absval, drop):
        f = _cast(dt, absval)
        w, dy = self.w.clone(), self.dy.clone()
        if drop is not None:
            if self.which == "dx":
                w[drop] = 0
            else:
                dy[drop] = 0
        xv, wv = _nchw(f(self.x)).requires_grad_(True), f(w).requires_grad_(True)
        y = F.conv_transpose2d(xv, wv, stride=self.s)
        dx, dw = torch.autograd.grad(y, (xv, wv), _nchw(f(dy)))
        return _nhwc(dx) if self.which == "dx" else dw


# ------------------------------------------------------------------------------------------------ the tables
TILE_CFGS = (0, 1, 2)          # 128 px x 128 ch, 64 x 64, 128 x 64

# (N, H, W, cin, cout, stride), each at the three tile configurations
FWD3x3 = [
    (1, 1, 1, 8, 4, 1),          # one pixel, one chunk
    (1, 1, 1, 8, 4, 2),          # one pixel at stride 2
    (1, 2, 2, 16, 8, 2),         # smallest even stride-2 image
    (3, 5, 3, 8, 20, 1),         # 3 pixel tiles: not a multiple of the 8-way XCD split
    (2, 9, 17, 16, 68, 1),       # one past an 8 x 16 tile both ways, two chunks, one channel group past 64
    (3, 17, 33, 24, 132, 2),     # odd sizes, three chunks (the odd tail step), one group past 128
    (2, 16, 32, 40, 64, 2),      # even sizes at stride 2, five chunks
]
# (N, H, W, cin, cout)
FWD1x1 = [
    (1, 1, 1, 8, 4),             # one pixel
    (2, 9, 17, 24, 20),          # one-chunk-per-stage form, three chunks
    (2, 9, 17, 40, 68),          # Cin % 32 != 0 at five chunks
    (1, 7, 5, 32, 4),            # four-chunk-per-stage form, one stage
    (1, 8, 16, 64, 64),          # ... two stages
    (3, 9, 17, 96, 132),         # ... three stages
]
# (N, H, W, cin, cout, stride, k) the epilogue variants run on
EPILOGUE_ROWS = [(2, 9, 17, 16, 68, 1, 3), (3, 17, 33, 24, 132, 2, 3), (2, 9, 17, 40, 68, 1, 1)]
# name -> (Fwd keywords, written into a channel slice of a wider sentinel tensor)
EPILOGUES = {
    "relu": (dict(relu=True), False),
    "plain": (dict(relu=False), False),
    "no_bias": (dict(relu=True, bias=False), False),
    "gated": (dict(relu=True, gated=True), False),
    "sliced": (dict(relu=True), True),
    "gated_sliced": (dict(relu=True, gated=True), True),
}
SLICE_OFF, SLICE_EXTRA, SENTINEL = 12, 24, -7.0
# (N, H, W, cin, cout, s), always into a sentinel slice
DECONV = [
    (2, 7, 9, 8, 4, 1),          # smallest
    (2, 7, 9, 24, 20, 2),        # 80 columns: a sub-pixel block straddles the 64-column tile edge
    (1, 3, 5, 32, 12, 4),        # 192 columns
    (3, 1, 1, 40, 36, 4),        # 576 columns on the one-chunk form
]
# 4096 tiles at tile_cfg 1: more than any resident grid, so every workgroup walks several tiles, border and interior in turn
WALK = [(4, 256, 256, 8, 4, 1, 3), (4, 256, 256, 8, 4, 1, 1)]      # (N, H, W, cin, cout, stride, k)
WALK_CFG = 1
# the layer's (N, H, W, cin, cout)
S2DGRAD = [(1, 1, 1, 4, 8), (2, 2, 2, 4, 8), (3, 3, 4, 20, 24), (2, 16, 16, 64, 8), (1, 17, 33, 68, 16), (2, 32, 18, 8, 72)]
CONV_BACKWARD = (2, 5, 7, 8, 12, 2)       # (N, H, W, cin, cout, stride): cout % 8 != 0 takes _Conv.backward's zero-upsample form

# 3x3 stride 1 with cin, cout <= 64 is one output tile, so n_chunks = n_pt = 1, 3, 4, 5, 12, 13, 16, 17, 29: the trip-count edges of
# k_wgrad_reduce's 16-way unrolled chunk loop
_WGRAD_NPT = [(1, 8, 8), (3, 5, 7), (1, 16, 16), (5, 8, 3), (3, 16, 9), (13, 1, 1), (1, 32, 32), (17, 2, 3), (29, 1, 2)]
WGRAD_NPT_CHUNKS = [1, 3, 4, 5, 12, 13, 16, 17, 29]
_CI, _CO = (4, 12, 64), (4, 36, 64)
# (N, H, W, cin, cout, taps, stride).  A single lost product has to be caught for every row with K <= 400; past that one product in K
# sinks into the rounding of the other K - 1 (product / bound ~ 1 / (2 K^2 u): 52 at K = 400, 1 at K = 2900).  Three rows between
# (K = 444, 486, 1040) are still held to it; the uneven-walk row alone is held to the lost-tile form only.
WGRAD = [(n, h, w, _CI[i % 3], _CO[(i + i // 3) % 3], 9, 1) for i, (n, h, w) in enumerate(_WGRAD_NPT)]   # (3,16,9): K = 444, (1,32,32): K = 1040
WGRAD += [
    (2, 31, 45, 256, 256, 9, 1),     # 48 tiles on 32 chunks: the uneven walk.  K = 2822 > 400: the lost-tile form alone
    (1, 1, 1, 8, 8, 9, 2),           # one pixel
    (2, 5, 3, 4, 36, 9, 2),          # small odd sizes
    (3, 17, 33, 68, 12, 9, 2),       # odd sizes at stride 2.  K = 486 > 400
    (2, 16, 32, 12, 68, 9, 2),       # even sizes at stride 2
    (2, 9, 7, 4, 4, 1, 1),           # smallest block form
    (2, 9, 7, 132, 132, 1, 1),       # one group past the 128 block
    (1, 13, 5, 256, 32, 1, 1),       # block side of the few-rows switch (cin)
    (1, 13, 5, 260, 36, 1, 1),       # block side of the few-rows switch (cout)
    (1, 13, 5, 260, 4, 1, 1),        # few-rows form
    (2, 13, 5, 388, 32, 1, 1),       # few-rows form, two ci tiles
]
SINGLE_PRODUCT_MAX_K = 400
SINGLE_PRODUCT_EXEMPT = {(2, 31, 45, 256, 256, 9, 1)}        # the only row above SINGLE_PRODUCT_MAX_K that is let off
# (N, H, W, cin, cout, s) through conv_train.deconv: forward, dx and dw
DECONV_TRAIN = [(2, 5, 6, 8, 4, 2), (1, 3, 5, 24, 20, 4), (2, 7, 9, 40, 12, 1)]


def families():
    """name -> list of Op: every row of every table (the forward tables in their plain form: no ReLU, so that every element
    speaks; the epilogue variants and the ReLU deconvolutions as rows of their own)."""
    N, H, W, ci, co, s = CONV_BACKWARD
    return {
        "fwd3x3": [Fwd(*r, k=3) for r in FWD3x3],
        "fwd1x1": [Fwd(*r, stride=1, k=1) for r in FWD1x1],
        "epilogue": [Fwd(*r[:6], k=r[6], **kw) for r in EPILOGUE_ROWS for kw, _ in EPILOGUES.values()],
        "deconv": [Deconv(*r, relu=relu) for r in DECONV for relu in (False, True)],
        "walk": [Fwd(*r[:6], k=r[6]) for r in WALK],
        "s2dgrad": [S2Dgrad(*r) for r in S2DGRAD],
        "conv_backward": [Fwd(N, H, W, ci, co, s, 3, bias=False, fold=False), S2Dgrad(N, H, W, ci, co), Wgrad(N, H, W, ci, co, 9, s)],
        "wgrad": [Wgrad(*r) for r in WGRAD],
        "deconv_train": [op for r in DECONV_TRAIN for op in (Deconv(*r, fold=False), DeconvGrad(*r, "dx"), DeconvGrad(*r, "dw"))],
    }
