"""Float64 references, the per-element rounding bound and the case tables of the Winograd F(2x2, 3x3) training kernels: the weight
gradient (csrc/conv_wino_wgrad.hip: k_wgrad_wino, k_wgrad_wino_reduce) and the forward kernel of csrc/conv_wino.hip on plain and on
adjoint-packed filters (the data gradient).  Shared by test_conv_wino_host.py (a plain-torch fp32 stand-in with the kernels'
summation structure: the bound proves itself) and test_gpu_conv_wino_bound.py (the kernels against the same bound).  Plain torch, no
GPU.  U, gamma, used_fraction, caught_share and the Op pattern are those of conv_direct_cases.py.

The bound.  Every operation of these kernels is an add, a subtract or a multiply of earlier results, so an element computed with at
most n roundings on any path from an input to it satisfies (running-error form, Higham, Accuracy and Stability of Numerical
Algorithms, §3.1)

    |got - ref| <= gamma(n) * S + (n / 2 - 2) * 2**-126,      gamma(n) = n u / (1 - n u),  u = 2**-24

with S the same straight-line program evaluated in float64 with every input AND every transform matrix replaced by its absolute
value.  conv_direct_cases.bound(K, S) is gamma(2 K + 4) S + K 2**-126, so K = (n - 4) / 2 (a half-integer where n is odd) makes
used_fraction and caught_share apply exactly gamma(n).  The additive term is there for a unit that flushes a subnormal product; the
rows' inputs are of order one or exact zeros, so it never decides (an exact zero is exact on both sides).

n, read off the kernel text.

  Weight gradient   dg = Gt [ sum_blocks (A dY At) . (Bt d B) ] G      (conv_wino_wgrad.hip)
    row wa of A dY At      t = fma(cA, dY1, dY0), then t.x +- t.y                                       2
    row wa of Bt d B       t01, t23 = fma(sB, d[r1], d[r0]), then a difference or a sum of two t         2
    every block term       one K slot of v_mfma_f32_32x32x2_f32: the product and the accumulate          2 per block
    chain length           what ONE workgroup accumulates: 32 blocks per 8 x 16 tile times its
                           tiles_max = ceil(n_pt / n_chunks) tiles (a chunk sums only its own tiles)     2 * 32 * tiles_max
    k_wgrad_wino_reduce    s0 takes n_chunks // 4 adds in the unrolled loop and the n_chunks % 4 of the
                           remainder loop, then (s0 + s1) + (s2 + s3); the sign is exact                 n_chunks // 4 + n_chunks % 4 + 2
                           (for n_chunks % 4 == 3 this is one more than ceil(n_chunks / 4) + 2: the
                           remainder chunks all go to s0)
    Gt . G                 u + 0.5 (u' + u''), 0.5 (u' - u''): two roundings a pass (0.5 x is exact)     4
    n = 64 * tiles_max + n_chunks // 4 + n_chunks % 4 + 10
    S = |Gt| [ sum_blocks (|A| |dY| |At|) . (|Bt| |d| |B|) ] |G|

  Forward / adjoint   Y = At [ sum_cin U . (Bt d B) ] A, + bias, gate * y + resid      (conv_wino.hip)
    U = G g Gt             k_wino_pack forms it in double and rounds once                                1
    V = Bt d B             t = fma(sgn, d[r1], d[r0]), then t +- t                                       2
    every cin term         product and accumulate of one MFMA K slot                                    2 per input channel
    output transform       (m0 + m1) + m2 / (m1 - m2) - m3, then x0 +- x1 +- x2                          4
    bias add, gate fma                                                                                   1 + 1
    n = 2 * Cin + 9       (Cin: the input channels of the kernel's layer; for the data gradient the layer's OUTPUT channels)
    S = |gate| ( |At| [ sum_cin (|G| |g| |Gt|) . (|Bt| |d| |B|) ] |A| + |bias| ) + |resid|
  The float64 side widens the fp32 weights the kernel is handed (the training path folds no scale).

Nothing here is fitted to what a kernel returns."""
import functools
import math

import torch
import torch.nn.functional as F

from conv_direct_cases import Op, U, _nchw, _nhwc, _seed, caught_share, gamma, used_fraction      # noqa: F401 (re-exported)

TH, TW = 8, 16                   # pixel tile of both kernels: 4 x 8 blocks of 2 x 2 outputs
BLOCKS = 32                      # blocks per tile = MFMA K slots a workgroup spends on it

A_ = torch.tensor([[1., 0.], [1., 1.], [1., -1.], [0., -1.]], dtype=torch.float64)                                   # 4 x 2 (At = A_.T)
BT = torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]], dtype=torch.float64)
G_ = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64)                    # 4 x 3


def _m(mat, dt, absval):
    return (mat.abs() if absval else mat).to(dt)


def ww_chunks(N, H, W, cin, cout):
    """The split-K chunk count of hvpr_conv2d_wino_wgrad_nhwc_f32 (csrc/conv_wino_wgrad.hip ww_chunks), restated: the GPU test pins it
    against hvpr_conv2d_wino_wgrad_workspace_bytes."""
    n_pt = N * (-(-H // TH)) * (-(-W // TW))
    n_ot = (-(-cin // 64)) * (-(-cout // 64))
    return max(1, min(-(-256 // n_ot), n_pt))


def wgrad_fits(H, W, cin, cout):
    """The kernel's own 32-bit-offset check (hvpr_conv2d_wino_wgrad_nhwc_f32 refuses where this is False), restated."""
    return H * W * max(cin, cout) * 4 < (1 << 31)


def geometry(row):
    """What a (N, H, W, cin, cout) row makes k_wgrad_wino do."""
    N, H, W, cin, cout = row
    per_image = (-(-H // TH)) * (-(-W // TW))
    n_pt = N * per_image
    n_ot = (-(-cin // 64)) * (-(-cout // 64))
    n_chunks = ww_chunks(*row)
    tiles = [len(range(c, n_pt, n_chunks)) for c in range(n_chunks)]
    crosses = any(p // per_image != (p + n_chunks) // per_image for p in range(n_pt - n_chunks))
    return dict(n_pt=n_pt, n_ot=n_ot, n_chunks=n_chunks, tiles_max=max(tiles), tiles_min=min(tiles), grid_mod8=n_ot * n_chunks % 8,
                crosses_images=crosses, per_image=per_image)


def wgrad_roundings(tiles_max, n_chunks):
    return 2 * BLOCKS * tiles_max + n_chunks // 4 + n_chunks % 4 + 10


def _input(g, shape, sparse):
    """randn, or what a BEV canvas looks like after a ReLU: non-negative, about 70 % of the pixels all zero."""
    t = torch.randn(*shape, generator=g)
    if sparse:
        t = torch.relu(t) * (torch.rand(*shape[:3], 1, generator=g) < 0.3)
    return t


def _patches(x, dt, absval, Hp, Wp):
    """x (N,H,W,C) -> V = Bt d B of every 2 x 2 output block of the zero-padded (Hp, Wp) canvas: (N, Hp/2, Wp/2, C, 4, 4)."""
    N, H, W, C = x.shape
    xp = torch.zeros(N, Hp + 2, Wp + 2, C, dtype=dt)
    xp[:, 1:H + 1, 1:W + 1] = x.to(dt).abs() if absval else x.to(dt)
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                                   # (N, Hp/2, Wp/2, C, 4, 4)
    bt = _m(BT, dt, absval)
    return torch.einsum("ar,nyxcrs,bs->nyxcab", bt, d, bt)


def _by_tile(t):
    """(N, 4 ty, 8 tx, C, 4, 4) -> (n_pt, 32, C, 16), tiles in the kernels' order (image, tile row, tile column)."""
    N, Hb, Wb, C = t.shape[:4]
    t = t.reshape(N, Hb // 4, 4, Wb // 8, 8, C, 16).permute(0, 1, 3, 2, 4, 5, 6)
    return t.reshape(N * (Hb // 4) * (Wb // 8), BLOCKS, C, 16).contiguous()


class WgradWino(Op):
    """hvpr_conv2d_wino_wgrad_nhwc_f32: x (N,H,W,cin), dz (N,H,W,cout) -> dw (cout,cin,3,3), evaluated in the Winograd domain.
    drops (the float64 value with something lost): "tile" every block of one pixel tile, "chunk" every tile of one split-K chunk,
    "co_group" / "ci_group" four channels of one tile, "sign" the signs of A's last row and column not applied by the reducer,
    "single" one block term."""

    def __init__(self, N, H, W, cin, cout, sparse=False):
        g = torch.Generator().manual_seed(_seed(N, H, W, cin, cout, 9, 1, 71))
        self.dims = (N, H, W, cin, cout)
        self.cin, self.cout, self.sparse = cin, cout, sparse
        self.x = _input(g, (N, H, W, cin), sparse)
        self.dz = torch.randn(N, H, W, cout, generator=g)
        self.geo = geometry(self.dims)
        self.n_chunks = self.geo["n_chunks"]
        self.n = wgrad_roundings(self.geo["tiles_max"], self.n_chunks)
        self.K = (self.n - 4) / 2
        self.Hp, self.Wp = -(-H // TH) * TH, -(-W // TW) * TW
        self._cache = {}
        t0 = (N - 1) * self.geo["per_image"]                  # the first tile of the last image: never a ragged one's remainder
        self.drops = {
            "tile": dict(tiles=[t0]),
            "chunk": dict(tiles=list(range(0, self.geo["n_pt"], self.n_chunks))),      # chunk 0: the longest walk, from a whole tile
            "co_group": dict(tiles=[t0], co=slice(cout - 4, cout)),
            "ci_group": dict(tiles=[t0], ci=slice(cin - 4, cin)),
            "sign": "sign",
            "single": dict(tiles=[t0], block=True),
        }

    def _operands(self, dt, absval):
        """-> dM = A dY At (n_pt, 32, cout, 16) and V = Bt d B (n_pt, 32, cin, 16) at dt."""
        key = (dt, absval)
        if key not in self._cache:
            N, H, W = self.dims[:3]
            dzp = torch.zeros(N, self.Hp, self.Wp, self.cout, dtype=dt)
            dzp[:, :H, :W] = self.dz.to(dt).abs() if absval else self.dz.to(dt)
            dy = dzp.reshape(N, self.Hp // 2, 2, self.Wp // 2, 2, self.cout).permute(0, 1, 3, 5, 2, 4)      # (N, Hb, Wb, co, 2, 2)
            a = _m(A_, dt, absval)
            dm = torch.einsum("ap,nyxcpq,bq->nyxcab", a, dy, a)
            self._cache[key] = (_by_tile(dm), _by_tile(_patches(self.x, dt, absval, self.Hp, self.Wp)))
        return self._cache[key]

    def _first_live_block(self):
        """The first block, from the tile's second row and column on, that carries anything (a sparse row has empty ones)."""
        dm, v = self._operands(torch.float64, True)
        t0 = self.drops["tile"]["tiles"][0]
        live = (dm[t0].sum((1, 2)) > 0) & (v[t0].sum((1, 2)) > 0)
        order = list(range(9, BLOCKS)) + list(range(9))
        return next(b for b in order if bool(live[b]))

    @staticmethod
    def _du(dm, v):
        return torch.einsum("tbox,tbix->xoi", dm, v)                          # (16, cout, cin)

    def _dg(self, du, dt, absval):
        g = _m(G_, dt, absval)
        return torch.einsum("ar,aboi,bs->oirs", g, du.reshape(4, 4, self.cout, self.cin), g)

    def _eval(self, dt, absval, drop):
        dm, v = self._operands(dt, absval)
        key = ("du", dt, absval)
        if key not in self._cache:
            self._cache[key] = self._du(dm, v)
        du = self._cache[key]
        if drop == "sign":
            xi = torch.arange(16)
            odd = ((xi // 4) == 3) != ((xi % 4) == 3)
            # the value with the sign left off; on the absolute side the same terms are taken OUT, which is what marks an element as touched
            du = du * torch.where(odd, 0.0 if absval else -1.0, 1.0).to(dt).view(16, 1, 1)
        elif drop is not None:
            dm_s, v_s = dm[drop["tiles"]], v[drop["tiles"]]
            if drop.get("block"):
                b = self._first_live_block()
                dm_s, v_s = dm_s[:, b:b + 1], v_s[:, b:b + 1]
            lost = torch.zeros_like(du)
            co, ci = drop.get("co", slice(None)), drop.get("ci", slice(None))
            lost[:, co, ci] = self._du(dm_s[:, :, co], v_s[:, :, ci])
            du = du - lost
        return self._dg(du, dt, absval)

    def live(self):
        """Index of the taps that meet the image at all.  With H == 1 (W == 1) the outer rows (columns) of the filter only ever see
        padding: there the float64 value is an exact zero whatever is lost — inside a block the 16 products cancel — so a lost term
        does not touch them, although the absolute sum S, which cannot cancel, shrinks there too."""
        H, W = self.dims[1:3]
        rows = torch.tensor([H > 1, True, H > 1])
        cols = torch.tensor([W > 1, True, W > 1])
        return (slice(None), slice(None), rows.view(3, 1) & cols.view(1, 3))

    def direct_reference(self):
        """float64 conv2d autograd, which knows nothing of the Winograd form."""
        w0 = torch.zeros(self.cout, self.cin, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(_nchw(self.x.double()), w0, padding=1)
        (dw,) = torch.autograd.grad(y, w0, _nchw(self.dz.double()))
        return dw

    def standin(self):
        """Honest fp32 arithmetic with the kernels' summation structure: fp32 transforms, one fp32 sum per tile, the tiles of a chunk
        added in order, the chunks in k_wgrad_wino_reduce's four-accumulator order, Gt . G as the reducer writes it."""
        dm, v = self._operands(torch.float32, False)
        n_pt, nc = self.geo["n_pt"], self.n_chunks
        part = torch.zeros(nc, 16, self.cout, self.cin)
        for k in range(self.geo["tiles_max"]):
            lo, hi = k * nc, min((k + 1) * nc, n_pt)                           # tile chunk + k * n_chunks of every chunk that has one
            part[:hi - lo] += torch.einsum("tbox,tbix->txoi", dm[lo:hi], v[lo:hi])
        s = [torch.zeros(16, self.cout, self.cin) for _ in range(4)]
        c = 0
        while c + 3 < nc:
            for j in range(4):
                s[j] = s[j] + part[c + j]
            c += 4
        while c < nc:
            s[0] = s[0] + part[c]
            c += 1
        u = ((s[0] + s[1]) + (s[2] + s[3])).reshape(4, 4, self.cout, self.cin)           # u[a][b]
        h = torch.stack([u[0] + 0.5 * (u[1] + u[2]), 0.5 * (u[1] - u[2]), 0.5 * (u[1] + u[2]) + u[3]])      # (3, b, co, ci)
        o = torch.stack([h[:, 0] + 0.5 * (h[:, 1] + h[:, 2]), 0.5 * (h[:, 1] - h[:, 2]), 0.5 * (h[:, 1] + h[:, 2]) + h[:, 3]], 1)
        return o.permute(2, 3, 0, 1).contiguous()                                           # (r, s, co, ci) -> (co, ci, r, s)


class FwdWino(Op):
    """hvpr_conv2d_wino_nhwc_f32 as the training step calls it (no bias, no ReLU): x (N,H,W,kin) -> (N,H,W,kout) with the filter
    w (kout,kin,3,3) — or, adjoint, with the filter w (kin,kout,3,3) of the layer whose data gradient is wanted: the kernel's filter is
    w'[o][i][u][v] = w[i][o][2-u][2-v].  sfm: _SfmStep.backward's form, gate of ones and a residual.
    drops: "flip" the 2-u, 2-v flip of the adjoint pack omitted, "group" the last four input channels lost, "single" the last one."""

    def __init__(self, N, H, W, kin, kout, adjoint=False, sfm=False, sparse=False):
        g = torch.Generator().manual_seed(_seed(N, H, W, kin, kout, 9, 1, 73 + adjoint))
        self.dims = (N, H, W, kin, kout, adjoint, sfm)
        self.kin, self.kout, self.adjoint = kin, kout, adjoint
        self.x = _input(g, (N, H, W, kin), sparse)
        shape = (kin, kout, 3, 3) if adjoint else (kout, kin, 3, 3)
        self.w = torch.randn(*shape, generator=g) / math.sqrt(9 * kin)
        self.gate = torch.ones(N, H, W) if sfm else None
        self.resid = torch.randn(N, H, W, kout, generator=g) if sfm else None
        self.n = 2 * kin + 9
        self.K = (self.n - 4) / 2
        self.Hp, self.Wp = -(-H // TH) * TH, -(-W // TW) * TW
        self.drops = {"flip": "flip", "group": slice(kin - 4, kin), "single": slice(kin - 1, kin)}

    def filter(self, flip=True):
        """(kout, kin, 3, 3) as the kernel's layer sees it."""
        if not self.adjoint:
            return self.w
        w = self.w.permute(1, 0, 2, 3)
        return w.flip(2, 3) if flip else w

    def _epilogue(self, z, dt, absval):
        if self.gate is None:
            return z
        f = (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))
        return f(self.gate).unsqueeze(-1) * z + f(self.resid)

    def _eval(self, dt, absval, drop):
        N, H, W = self.dims[:3]
        if drop == "flip" and absval:
            return torch.zeros(N, H, W, self.kout, dtype=dt)                  # every element is touched
        w = self.filter(flip=drop != "flip").double()
        if isinstance(drop, slice):
            w = w.clone()
            w[:, drop] = 0
        g = _m(G_, torch.float64, absval)
        u = torch.einsum("ar,oirs,bs->oiab", g, w.abs() if absval else w, g).to(dt)          # formed in double, rounded once
        v = _patches(self.x, dt, absval, self.Hp, self.Wp)
        m = torch.einsum("nyxiab,oiab->nyxoab", v, u)
        a = _m(A_, dt, absval)
        y = torch.einsum("ap,nyxoab,bq->nyxopq", a, m, a)                    # At M A
        y = y.permute(0, 1, 4, 2, 5, 3).reshape(N, self.Hp, self.Wp, self.kout)[:, :H, :W]
        return self._epilogue(y, dt, absval).contiguous()

    def live(self):
        return (Ellipsis,)

    def direct_reference(self):
        z = _nhwc(F.conv2d(_nchw(self.x.double()), self.filter().double(), padding=1))
        return self._epilogue(z, torch.float64, False)


# ------------------------------------------------------------------------------------------------ the tables
# Rows are (N, H, W, cin, cout): the smallest shapes that reach each path.  n_ot = 64 x 64 (co, ci) tiles, n_pt = 8 x 16 pixel tiles,
# n_chunks = min(ceil(256 / n_ot), n_pt); chunk c walks the tiles c, c + n_chunks, ...  Channel pairs with 16 output tiles: 256 x 256
# as in the backbone, and the cheaper 964 x 4 (16 x 1, dead co groups) and 452 x 68 (8 x 2, both last tiles partly live).
WGRAD_PIPE = [
    (1, 16, 128, 964, 4),        # 16 tiles on 16 chunks: one tile each — nothing of the pipeline's steady state
    (1, 8, 272, 256, 256),       # 17 tiles: chunk 0 walks two, the other 15 see "past the end" right after their only tile
    (5, 16, 128, 256, 64),       # 4 output tiles, 64 chunks, 80 tiles: two tiles in 16 workgroups, one in 48
    (3, 8, 176, 964, 4),         # 33 tiles, 11 an image: chunk 0 walks tiles 0, 16, 32 = images 0, 1, 2; the others two
    (3, 16, 128, 452, 68),       # 48 tiles: three each, one per image (sparse)
    (4, 8, 208, 964, 4),         # 52 tiles: four in chunks 0-3, three in the rest
    (5, 16, 128, 256, 256),      # 80 tiles: five each — both LDS stages reused twice
]
WGRAD_EDGE = [
    (1, 1, 1, 4, 4),             # a 1 x 1 image, the smallest legal channel counts, a grid of one
    (2, 7, 15, 24, 68),          # dead ci groups inside the only ci tile, two co tiles with the last partly live; 2 chunks
    (2, 13, 21, 24, 68),         # the ragged row of test_gpu_conv_wino.py: 8 tiles, grid 16
    (3, 9, 17, 68, 132),         # two ci / three co tiles, last ones partly live; 12 tiles = 12 chunks, grid 72 = 9 x 8 (sparse)
    (1, 9, 33, 132, 24),         # three ci tiles, dead co groups; 6 chunks
    (3, 1, 15, 4, 132),          # H = 1, odd width inside one tile; 3 chunks
    (1, 7, 1, 132, 4),           # W = 1
    (5, 1, 1, 68, 68),           # 5 chunks on four output tiles
    (1, 9, 17, 4, 132),          # cin = 4 over three co tiles, one pixel column past the tile edge
    (2, 7, 31, 68, 4),           # odd width whose last pixel pair straddles the image edge; grid 8
]
WGRAD_SPARSE = {(3, 16, 128, 452, 68), (3, 9, 17, 68, 132)}

# (N, H, W, cin_w, cout_w) of the WEIGHT (cout_w, cin_w, 3, 3): the kernel's layer takes cout_w channels in and gives cin_w out
DGRAD_WINO = [
    (2, 12, 20, 12, 40),         # 12 outputs padded to one 64-channel tile; 12 x 20 pairs its right and bottom edge tiles
    (1, 14, 26, 24, 72),         # 5 live block columns, 3 live block rows: ragged, nothing can pair
    (2, 13, 21, 132, 64),        # three output channel tiles, the last with one live group; pairs on the right (sparse dz)
    (2, 12, 20, 24, 24),         # _SfmStep.backward's form: gate of ones, resid = dy
]
DGRAD_SFM = {(2, 12, 20, 24, 24)}
DGRAD_SPARSE = {(2, 13, 21, 132, 64)}
DGRAD_PAIRS = {(2, 12, 20, 12, 40): True, (1, 14, 26, 24, 72): False, (2, 13, 21, 132, 64): True, (2, 12, 20, 24, 24): True}

# (N, H, W, cin, cout) through conv_fwd_raw(x, w, 1) with and without stats=True
FWD_TRAIN = [
    (3, 8, 16, 8, 64),           # whole tiles, one chunk of input channels
    (2, 12, 20, 40, 12),         # the ragged and padded-channel shapes of DGRAD_WINO, as a forward layer
    (1, 14, 26, 72, 24),
    (2, 13, 21, 64, 132),        # (sparse x)
]
FWD_SPARSE = {(2, 13, 21, 64, 132)}

# Rows on which every corruption but the single lost block must put >= DETECT_SHARE of the elements it touches outside the bound: one
# tile per workgroup, >= 3 tiles per workgroup, ragged channels, ragged image (conditions, not measurements).
DETECT = [(1, 16, 128, 964, 4), (3, 16, 128, 452, 68), (2, 13, 21, 24, 68), (3, 9, 17, 68, 132), (1, 9, 17, 4, 132)]
DETECT_SHARE = 0.9
SINGLE_SHARE = 0.5
# One lost block term in a chain of c = 32 * tiles_max: the term is ~1 / (32 n_pt) of S while the bound is ~2 c u S, so it stands out
# by ~1 / (64 c n_pt u); what decides is how often a product of two near-normal numbers falls below that.  Determined on the CPU
# (the host test prints every share): at least half of the touched elements are caught on every row of both tables, the longest chain
# (five tiles, c = 160: 0.58; three tiles of the sparse row, c = 96: 0.52; one tile: 0.80 - 1.0) included.  Every row with a chain up
# to this length is held to SINGLE_SHARE; a longer one added later is too unless it is named in SINGLE_BLOCK_EXEMPT (one a family).
SINGLE_BLOCK_MAX_CHAIN = 160
SINGLE_BLOCK_EXEMPT = {"wgrad_pipe": set(), "wgrad_edge": set()}


@functools.lru_cache(maxsize=None)
def families():
    """name -> list of Op, built once and shared (an Op keeps its transformed operands)."""
    return {
        "wgrad_pipe": [WgradWino(*r, sparse=r in WGRAD_SPARSE) for r in WGRAD_PIPE],
        "wgrad_edge": [WgradWino(*r, sparse=r in WGRAD_SPARSE) for r in WGRAD_EDGE],
        "dgrad": [dgrad_op(r) for r in DGRAD_WINO],
        "fwd_train": [FwdWino(*r, sparse=r in FWD_SPARSE) for r in FWD_TRAIN],
    }


def dgrad_op(row):
    N, H, W, cin_w, cout_w = row
    return FwdWino(N, H, W, cout_w, cin_w, adjoint=True, sfm=row in DGRAD_SFM, sparse=row in DGRAD_SPARSE)
