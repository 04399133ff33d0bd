"""Float64 reference, the per-element rounding bound and the case tables of SpatialAttention in training mode
(csrc/gate_train.hip: k_gt_pool, k_gt_conv, k_gt_sums, k_gt_stats, k_gt_apply, k_gt_bwd_red, k_gt_bwd_fin, k_gt_bwd_da, k_gt_bwd_conv,
k_gt_bwd_fin2), shared by test_gate_train_host.py (the kernels' formulas in fp32 torch stand in for the kernels: the bound proves
itself, and the reference with one mistake made falls outside it) and test_gpu_gate_train.py (the kernels against the same bound).
Plain torch, no GPU.  Q, qsum, gamma, used_fraction, caught_share and the constants come from bn_train_cases.py / conv_direct_cases.py.

The reference takes exactly the fp32 numbers the forward entry point is handed (eps crosses the C interface as a float), widened to
float64: pooled = (max_c y, mean_c y) with the arg-max of the lowest channel on ties (torch's max(dim)); a = conv3x3(pooled, zero
padding) + bias; mean, biased variance, invstd = 1 / sqrt(var + eps) of a over all N H W pixels; gate = sigmoid((a - mean) invstd gamma
+ beta); and backwards ds = dgate gate (1 - gate), dbeta = sum ds, dgamma = sum ds xhat, da = gamma invstd (ds - dbeta / n - xhat
dgamma / n), dW = sum da pooled(shifted), dbias = sum da, d pooled = conv_transpose(da, W), dy = d mean / C + [c == argmax] d max.  The
backward entry point is handed what the forward one returned, so its bound is the bound of the whole chain from y.  The arg-max is
taken on input values: exact in fp32 and float64 alike, no element is undecided.

The bound.  Every value is followed as Q = (float64 value, error bound) operation by operation from the kernels' source, as in
bn_train_cases.py.  The k of each fp32 sum (roundings on the longest path of a partial sum):

  * mean_c y (k_gt_pool): a lane takes T = ceil(C / 4 / 8) float4 groups, 3 roundings each ((x + y) + (z + w), then the accumulator),
    then 3 butterfly steps over its 8 lanes: k = 3 T + 3 (pool_k); then one division by C.
  * conv3x3: a chain of 18 fmaf from 0: k = 18.  d pooled: a chain of 9 fmaf per plane: k = 9; d mean / C one division more; the
    arg-max channel's dy one addition more.
  * per-tile (sum a', sum a'^2) with a' the convolution BEFORE the bias (the kernel's point: the variance does not see the bias):
    a'^2 is rounded once, then 6 butterfly steps of a wave and 2 additions of the 4 waves: k = 8 (block_sums; TILE_K).  The tiles meet in
    double: ceil(tiles / 256) serial additions of a thread and 8 steps of the LDS tree (final_k64), then mean = sum / n + bias,
    var = sum2 / n - (sum / n)^2 clamped at 0 and invstd in double, one fp32 rounding each.
  * sum ds, sum ds xhat (k_gt_bwd_red): red_blocks(P) workgroups of 256 threads stride over the pixels: red_trips(P) serial additions (the
    second by fmaf) + 8: k = red_trips + 8; the workgroups meet in double (final_k64(red_blocks)).
  * dW (18) and dbias: products da pooled rounded once, then block_sums per tile (k = 8) and the tiles in double.
  * expf: no statement of its maximum error was found in the HIP math documentation shipped with ROCm, so it is ASSUMED to be
    at most EXPF_ULP = 2 ulp (<= 4 u relative); the observed used fraction of `gate` shows whether that holds.  The divisions
    are correctly rounded (the library is built without fast-math).

Nothing here is fitted to what a kernel returns.

What each row is for stands next to it in ROWS; the host test asserts from the restated launch arithmetic (tiles, red_blocks,
red_trips, pool_trips; workspace_bytes is pinned against hvpr_spatial_gate_train_workspace_bytes on the GPU) that it gets there.

Observed on the MI355X (max err / bound over all rows, per output): see OBSERVED at the end of this file."""
import numpy as np
import torch
import torch.nn.functional as F

from bn_train_cases import Q, TINY, U64, caught_share, qsum, used_fraction  # noqa: F401  (re-exported to the tests)
from conv_direct_cases import SENTINEL, U, gamma  # noqa: F401

EPS = 1e-3
GT = 16
EXPF_ULP = 2.0
TILE_K = 8


# ------------------------------------------------------------------------------------------------ the kernels' launch arithmetic
def n_tiles(N, H, W):
    return N * -(-H // GT) * -(-W // GT)


def red_blocks(P):
    return min(max(-(-P // 2048), 1), 1024)


def red_trips(P):
    """Trips of k_gt_bwd_red's grid-stride loop taken by thread 0 (the most any thread takes)."""
    return -(-P // (red_blocks(P) * 256))


def final_trips(blocks):
    return -(-blocks // 256)


def final_k64(blocks):
    return final_trips(blocks) + 8


def pool_trips(C):
    return -(-(C // 4) // 8)


def pool_k(C):
    return 3 * pool_trips(C) + 3


def workspace_bytes(N, H, W):
    up = lambda b: -(-b // 256) * 256
    return up((n_tiles(N, H, W) * 19 + 1024 * 2) * 4) + up(N * H * W * 4) + 256


# ------------------------------------------------------------------------------------------------ one case
def _seed(*row):
    return int(sum((int(v) + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


class Case:
    """Inputs of one row: y (N, H, W, C) post-ReLU with about one pixel in eight all zero (every channel ties: channel 0 takes the
    gradient), conv weight (1, 2, 3, 3), bias, gamma, beta, dgate (N, H, W).  content:
      tie_lanes     every third pixel's maximum is shared by channels 1 and C - 3: two lanes of the pixel's group (C >= 12)
      tie_trips     every third pixel's maximum is shared by channels 2 and 34: lane 0 on its first and second trip (C >= 36)
      negative      every second pixel is negative in every channel (not a post-ReLU input: max < 0, mean < 0)
      constant      the same positive vector in every pixel and a weight whose only taps are the two centres: the variance is exactly 0"""

    def __init__(self, N, H, W, C, content=None, bias=0.3, gam=1.3, beta=-0.2, dgate_zero=False, plant_tail=False, seed=0, name=None):
        g = torch.Generator().manual_seed(_seed(N, H, W, C, seed))
        self.N, self.H, self.W, self.C, self.P, self.eps = N, H, W, C, N * H * W, EPS
        self.content, self.name = content, name or f"{N}x{H}x{W}x{C}"
        P = self.P
        y = torch.relu(torch.randn(P, C, generator=g))
        y[torch.rand(P, generator=g) < 0.125] = 0.0
        pix = torch.arange(P)
        if content == "tie_lanes":
            assert C >= 12 and (1 // 4) % 8 != ((C - 3) // 4) % 8
            top = y.max(1)[0] + 0.5
            y[pix % 3 == 0, 1] = top[pix % 3 == 0]
            y[pix % 3 == 0, C - 3] = top[pix % 3 == 0]
        elif content == "tie_trips":
            assert C >= 36
            top = y.max(1)[0] + 0.5
            y[pix % 3 == 0, 2] = top[pix % 3 == 0]
            y[pix % 3 == 0, 34] = top[pix % 3 == 0]
        elif content == "negative":
            y[pix % 2 == 0] = -torch.rand(int((pix % 2 == 0).sum()), C, generator=g) - 0.1
        elif content == "constant":
            y = (torch.rand(C, generator=g) + 0.25).expand(P, C).clone()
        else:
            assert content is None, content
        self.y = y.view(N, H, W, C)
        self.w = torch.randn(1, 2, 3, 3, generator=g) * 0.4
        if content == "constant":
            keep = torch.zeros(1, 2, 3, 3)
            keep[:, :, 1, 1] = 1.0
            self.w = self.w * keep
        self.bias, self.gamma, self.beta = torch.tensor([float(bias)]), torch.tensor([float(gam)]), torch.tensor([float(beta)])
        self.dgate = torch.zeros(N, H, W) if dgate_zero else torch.randn(N, H, W, generator=g)
        if plant_tail:          # the pixels past 2048 * 1024 carry a weight no rounding can hide
            self.dgate.view(-1)[2048 * 1024:] = 40.0

    def to(self, device):
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self


# ------------------------------------------------------------------------------------------------ the reference and its bound
WRONG = ("ties_to_highest", "mean_over_c_minus_1", "edge_clamped_padding", "taps_not_flipped", "dbeta_term_dropped",
         "dgamma_term_dropped", "last_tile_column_lost", "tail_pixels_lost_from_dgamma")
WRONG_STANDIN = ("bias_in_fp32_squares",)


def _chain(p, w, k, transpose=False, flip=True, clamp=False):
    """3x3 convolution (or its transpose) of the Q planes p (N, ch, H, W) by the exact weight w as a sum with k roundings on a path."""
    wa = w.abs()
    if transpose:
        op = (lambda t, ww: F.conv_transpose2d(t, ww, padding=1)) if flip else (lambda t, ww: F.conv2d(t, ww.transpose(0, 1), padding=1))
    elif clamp:
        op = lambda t, ww: F.conv2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), ww)
    else:
        op = lambda t, ww: F.conv2d(t, ww, padding=1)
    S = op(p.hi(), wa)
    return Q(op(p.v, w), op(p.e, wa) + gamma(k) * S + k * TINY * (S > 0))


def _recip(q):
    """1 / q for q.v - q.e > 0, before the rounding of the division."""
    lo = q.v - q.e
    assert bool((lo > 0).all())
    return Q(1.0 / q.v, q.e / (q.v * lo))


def reference(c, wrong=None):
    """-> dict: pooled (N, H, W, 2), a, gate, dy, stats (3: mean, var, invstd), dw18, dbias, dgamma, dbeta as Q and argmax (int64).
    wrong: one of WRONG — the same formulas with that mistake made."""
    assert wrong is None or wrong in WRONG
    N, H, W, C, P = c.N, c.H, c.W, c.C, c.P
    n = float(P)
    y = c.y.double()
    one = torch.ones((), dtype=torch.float64, device=y.device)
    r = {}
    # k_gt_pool
    if wrong == "ties_to_highest":
        mx, am = y.flip(-1).max(-1)
        am = C - 1 - am
    else:
        mx, am = y.max(-1)
    sm = qsum(Q.exact(c.y), -1, pool_k(C))
    mean_c = (sm * Q(one / (C - 1 if wrong == "mean_over_c_minus_1" else C))).rnd()
    pooled = Q(torch.stack([mx, mean_c.v], -1), torch.stack([torch.zeros_like(mx), mean_c.e], -1))
    r["pooled"], r["argmax"] = pooled, am
    # k_gt_conv
    pl = Q(pooled.v.permute(0, 3, 1, 2), pooled.e.permute(0, 3, 1, 2))
    w = c.w.double()
    acc = _chain(pl, w, 18, clamp=wrong == "edge_clamped_padding")              # (N, 1, H, W)
    acc = Q(acc.v[:, 0], acc.e[:, 0])
    a = (acc + Q.exact(c.bias)).rnd()
    r["a"] = a
    # per-tile partial sums, k_gt_sums, k_gt_stats
    keep = torch.ones(W, dtype=torch.float64, device=y.device)
    if wrong == "last_tile_column_lost":
        keep[(-(-W // GT) - 1) * GT:] = 0.0
    k64 = final_k64(n_tiles(N, H, W))
    flat = lambda q: Q((q.v * keep).reshape(-1), (q.e * keep).reshape(-1))
    s1 = qsum(flat(acc), 0, TILE_K, k64)
    s2 = qsum(flat((acc * acc).rnd()), 0, TILE_K, k64)
    inv_n = Q(one / n, U64 / n * one)
    ms = s1 * inv_n
    var = s2 * inv_n - ms * ms
    var = Q(var.v.clamp_min(0.0), var.e + 4.0 * U64 * (s2.hi() / n + ms.hi() ** 2))      # (the clamp moves towards the true var >= 0)
    eps = float(np.float32(c.eps))
    invstd_v = (var.v + eps) ** -0.5
    invstd = Q(invstd_v, 0.5 * var.e * ((var.v - var.e).clamp_min(0.0) + eps) ** -1.5 + 4.0 * U64 * invstd_v).rnd()
    m_all = ms + Q.exact(c.bias)[0]
    mean = Q(m_all.v, m_all.e + 2.0 * U64 * m_all.hi()).rnd()
    var = var.rnd()
    r["stats"] = Q(torch.stack([mean.v, var.v, invstd.v]), torch.stack([mean.e, var.e, invstd.e]))
    # k_gt_apply
    gam, bet = Q.exact(c.gamma)[0], Q.exact(c.beta)[0]
    xh = ((a - mean).rnd() * invstd).rnd()
    z = ((xh * gam).rnd() + bet).rnd()
    ev = torch.exp(-z.v)
    ee = ev * torch.expm1(z.e)
    ex = Q(ev, ee + 2.0 * EXPF_ULP * U * (ev + ee) + TINY)
    gate = _recip((ex + Q(one)).rnd()).rnd()
    r["gate"] = gate
    # k_gt_bwd_red, k_gt_bwd_fin
    ds = ((Q.exact(c.dgate) * gate).rnd() * (Q(one) - gate).rnd()).rnd()
    kr, kr64 = red_trips(P) + TILE_K, final_k64(red_blocks(P))
    dbeta = qsum(Q(ds.v.reshape(-1), ds.e.reshape(-1)), 0, kr, kr64).rnd()
    t = ds * xh
    if wrong == "tail_pixels_lost_from_dgamma":
        live = (torch.arange(P, device=y.device) < 2048 * 1024).view(N, H, W)
        t = Q(t.v * live, t.e * live)
    dgamma = qsum(Q(t.v.reshape(-1), t.e.reshape(-1)), 0, kr, kr64).rnd()
    r["dbeta"], r["dgamma"] = dbeta, dgamma
    # k_gt_bwd_da
    inv_nf = Q(one / n).rnd()
    t1, t2 = (dbeta * inv_nf).rnd(), (dgamma * inv_nf).rnd()
    if wrong == "dbeta_term_dropped":
        t1 = Q(torch.zeros_like(t1.v))
    if wrong == "dgamma_term_dropped":
        t2 = Q(torch.zeros_like(t2.v))
    da = ((gam * invstd).rnd() * ((ds - t1).rnd() - (xh * t2).rnd()).rnd()).rnd()
    # k_gt_bwd_conv, k_gt_bwd_fin2
    pp = Q(F.pad(pl.v, (1, 1, 1, 1)), F.pad(pl.e, (1, 1, 1, 1)))
    dw_v, dw_e = [], []
    for ch in range(2):
        for ky in range(3):
            for kx in range(3):
                sh = Q(pp.v[:, ch, ky:ky + H, kx:kx + W], pp.e[:, ch, ky:ky + H, kx:kx + W])
                s = qsum(flat((da * sh).rnd()), 0, TILE_K, k64).rnd()
                dw_v.append(s.v)
                dw_e.append(s.e)
    r["dw18"] = Q(torch.stack(dw_v), torch.stack(dw_e))
    db = qsum(flat(da), 0, TILE_K, k64).rnd()
    r["dbias"] = Q(db.v.reshape(1), db.e.reshape(1))
    dp = _chain(Q(da.v[:, None], da.e[:, None]), w, 9, transpose=True, flip=wrong != "taps_not_flipped")          # (N, 2, H, W)
    dmax = Q(dp.v[:, 0], dp.e[:, 0])
    dmean = (Q(dp.v[:, 1], dp.e[:, 1]) * Q(one / C)).rnd()
    hit = F.one_hot(am, C).bool()
    with_max = (dmean + dmax).rnd()
    r["dy"] = Q(torch.where(hit, with_max.v[..., None], dmean.v[..., None]), torch.where(hit, with_max.e[..., None], dmean.e[..., None]))
    r["dgamma"], r["dbeta"] = Q(dgamma.v.reshape(1), dgamma.e.reshape(1)), Q(dbeta.v.reshape(1), dbeta.e.reshape(1))
    return r


def autograd64(c):
    """The same outputs from torch autograd of the formula in float64 (what the existing test in test_gpu_train_ops.py compares with):
    the values of reference() must agree with it."""
    y, w, b, gam, bet = (t.double().clone().requires_grad_(True) for t in (c.y, c.w, c.bias, c.gamma, c.beta))
    yc = y.permute(0, 3, 1, 2)
    pooled = torch.cat((yc.max(dim=1, keepdim=True)[0], yc.mean(dim=1, keepdim=True)), dim=1)
    a = F.conv2d(pooled, w, b, padding=1)
    m, v = a.mean(), a.var(unbiased=False)
    gate = torch.sigmoid((a - m) / torch.sqrt(v + float(np.float32(c.eps))) * gam + bet)[:, 0]
    dy, dw, db, dg, dbt = torch.autograd.grad(gate, (y, w, b, gam, bet), c.dgate.double())
    return {"a": a.detach()[:, 0], "gate": gate.detach(), "dy": dy, "dw18": dw.reshape(18), "dbias": db, "dgamma": dg, "dbeta": dbt,
            "stats": torch.stack([m.detach(), v.detach(), (v.detach() + float(np.float32(c.eps))) ** -0.5])}


# ------------------------------------------------------------------------------------------------ the fp32 stand-in
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _tree(x):
    """fp32 pairwise sum over the last dimension (a power of two): log2 roundings on every path, as a butterfly has."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _tile_partials(t, N, H, W):
    """fp32 (N, H, W) -> per-tile sums as block_sums takes them: a tree over each wave's 64 threads, then (w0 + w1) + (w2 + w3)."""
    th, tw = -(-H // GT), -(-W // GT)
    t = F.pad(t, (0, tw * GT - W, 0, th * GT - H)).view(N, th, GT, tw, GT).permute(0, 1, 3, 2, 4).reshape(N * th * tw, 4, 64)
    s = _tree(t)
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def _red_partials(t, P):
    """fp32 (P,) terms -> k_gt_bwd_red's workgroup rows: a thread's strided pixels one after the other, then block_sums."""
    rb, trips = red_blocks(P), red_trips(P)
    t = F.pad(t, (0, trips * rb * 256 - P)).view(trips, rb, 4, 64)
    acc = t[0].clone()
    for i in range(1, trips):
        acc = acc + t[i]
    s = _tree(acc)
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def standin(c, wrong=None):
    """The kernels' formulas in fp32 torch, partial sums in the kernels' structure, the finalising in double.  wrong =
    "bias_in_fp32_squares": the statistics taken of a = conv + bias instead of the value before the bias."""
    assert wrong is None or wrong in WRONG_STANDIN
    N, H, W, C, P = c.N, c.H, c.W, c.C, c.P
    f32 = torch.float32
    o = {}
    y = c.y
    mx, am = y.max(-1)
    T = pool_trips(C)
    g4 = F.pad(y, (0, T * 32 - C)).view(N, H, W, T, 8, 4)
    grp = (g4[..., 0] + g4[..., 1]) + (g4[..., 2] + g4[..., 3])
    sm = grp[..., 0, :].clone()
    for i in range(1, T):
        sm = sm + grp[..., i, :]
    mean_c = _tree(sm) / torch.tensor(float(C), dtype=f32)
    o["pooled"], o["argmax"] = torch.stack([mx, mean_c], -1), am
    pp = F.pad(torch.stack([mx, mean_c], 1), (1, 1, 1, 1))
    acc = torch.zeros(N, H, W, dtype=f32)
    for ky in range(3):
        for kx in range(3):
            for ch in range(2):
                acc = _fma(c.w[0, ch, ky, kx], pp[:, ch, ky:ky + H, kx:kx + W], acc)
    a = acc + c.bias
    o["a"] = a
    src = a if wrong == "bias_in_fp32_squares" else acc
    s1, s2 = _tile_partials(src, N, H, W).double().sum(), _tile_partials(src * src, N, H, W).double().sum()
    ms = s1 / P
    var = (s2 / P - ms * ms).clamp_min(0.0)
    m = ms if wrong == "bias_in_fp32_squares" else ms + c.bias.double()[0]
    stats = torch.stack([m.float(), var.float(), (1.0 / torch.sqrt(var + float(np.float32(c.eps)))).float()])
    o["stats"] = stats
    xh = (a - stats[0]) * stats[2]
    z = xh * c.gamma + c.beta
    gate = 1.0 / (1.0 + torch.exp(-z))
    o["gate"] = gate
    ds = c.dgate * gate * (1.0 - gate)
    dbeta_d, dgamma_d = _red_partials(ds.reshape(-1), P).double().sum(), _red_partials((ds * xh).reshape(-1), P).double().sum()
    dbeta, dgamma = dbeta_d.float(), dgamma_d.float()
    o["dbeta"], o["dgamma"] = dbeta.reshape(1), dgamma.reshape(1)
    inv_n = torch.tensor(1.0 / P, dtype=torch.float64).float()
    da = c.gamma * stats[2] * (ds - dbeta * inv_n - xh * (dgamma * inv_n))
    dw = [_tile_partials(da * pp[:, ch, ky:ky + H, kx:kx + W], N, H, W).double().sum().float()
          for ch in range(2) for ky in range(3) for kx in range(3)]
    o["dw18"] = torch.stack(dw)
    o["dbias"] = _tile_partials(da, N, H, W).double().sum().float().reshape(1)
    dap = F.pad(da, (1, 1, 1, 1))
    dmax, dmean = torch.zeros(N, H, W, dtype=f32), torch.zeros(N, H, W, dtype=f32)
    for ky in range(3):
        for kx in range(3):
            d = dap[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
            dmax, dmean = _fma(c.w[0, 0, ky, kx], d, dmax), _fma(c.w[0, 1, ky, kx], d, dmean)
    dmean = dmean / torch.tensor(float(C), dtype=f32)
    o["dy"] = torch.where(F.one_hot(am, C).bool(), (dmean + dmax)[..., None], dmean[..., None])
    return o


OUTPUTS = ("pooled", "a", "stats", "gate", "dy", "dw18", "dbias", "dgamma", "dbeta")


def fractions(got, r):
    """name -> max err / bound for every Q output (argmax is compared exactly by the caller); stats as mean / var / invstd."""
    fr = {k: used_fraction(got[k].reshape(r[k].v.shape), r[k]) for k in OUTPUTS if k != "stats"}
    for i, k in enumerate(("mean", "var", "invstd")):
        fr[k] = used_fraction(got["stats"][i], r["stats"][i])
    return fr


# ------------------------------------------------------------------------------------------------ the table
# name -> Case keywords.  (N, H, W, C), then what the row is there for.
ROWS = {
    "one_pixel": dict(N=1, H=1, W=1, C=4),                                  # variance 0, every neighbour is padding; lanes 1 to 7 empty
    "one_row": dict(N=1, H=1, W=37, C=8),
    "one_column": dict(N=1, H=37, W=1, C=8),
    "one_tile": dict(N=1, H=16, W=16, C=12, content="tie_lanes"),           # lanes 3 to 7 empty; a maximum shared across lanes
    "one_past_a_tile": dict(N=1, H=17, W=17, C=12),                         # four tiles, three of them one pixel wide or high
    "ragged_tiles_two_trips": dict(N=2, H=15, W=33, C=36, content="tie_trips"),      # C / 4 = 9: lane 0 takes a second trip, and shares a maximum with it
    "pixels_not_by_32": dict(N=3, H=5, W=7, C=8),                           # 105 pixels: the last pool workgroup is ragged
    "wide": dict(N=2, H=9, W=7, C=128, content="negative"),                 # four trips of every lane; all-negative pixels
    "widest": dict(N=1, H=3, W=3, C=512),                                   # 16 trips; 128 float4 groups per dy row
    "one_red_block": dict(N=1, H=32, W=64, C=4),                            # 2048 pixels: red_blocks = 1
    "two_red_blocks": dict(N=1, H=1, W=2049, C=4),                          # one pixel more: red_blocks = 2 (and 129 tiles in a row)
    "tiles_256": dict(N=1, H=256, W=256, C=4),                              # final_sums: exactly one trip of its 256 threads
    "tiles_257": dict(N=1, H=16, W=4112, C=4),                              # ... and thread 0 takes a second
    "tiles_300_three_images": dict(N=3, H=160, W=160, C=4),
    "constant_field": dict(N=1, H=9, W=20, C=8, content="constant"),        # variance exactly 0: invstd = 1 / sqrt(eps)
    "bias_300": dict(N=1, H=17, W=17, C=12, bias=300.0),                    # |mean| / sigma in the hundreds: the statistics must not see the bias
    "gamma_zero": dict(N=1, H=17, W=17, C=12, gam=0.0),                     # da, dy, dW exactly zero
    "gamma_negative": dict(N=1, H=17, W=17, C=12, gam=-0.8),
    "dgate_zero": dict(N=1, H=17, W=17, C=12, dgate_zero=True),             # every gradient exactly zero
}
# the smallest input that gives k_gt_bwd_red a ninth trip: one pixel row more than 2048 * 1024 pixels (34 MB of y)
LARGE = {"past_the_reduction_grid": dict(N=1, H=1449, W=1448, C=4)}
ALL = {**ROWS, **LARGE}

# wrong variant -> (Case keywords of the inputs built for it, the outputs on which every touched element must be outside the bound)
WRONG_CASES = {
    "ties_to_highest": (dict(N=2, H=15, W=33, C=36, content="tie_trips"), ("dy",)),
    "mean_over_c_minus_1": (dict(N=1, H=17, W=17, C=12), ("pooled",)),
    "edge_clamped_padding": (dict(N=1, H=17, W=17, C=12), ("a",)),
    "taps_not_flipped": (dict(N=1, H=17, W=17, C=12), ("dy",)),
    "dbeta_term_dropped": (dict(N=1, H=17, W=17, C=12), ("dy", "dw18", "dbias")),
    "dgamma_term_dropped": (dict(N=1, H=17, W=17, C=12), ("dy", "dw18")),
    "last_tile_column_lost": (dict(N=1, H=17, W=17, C=12), ("stats", "dw18", "dbias")),
    "tail_pixels_lost_from_dgamma": (dict(N=1, H=1449, W=1448, C=4, plant_tail=True), ("dgamma",)),
}


def case(name, **over):
    return Case(**{**ALL[name], **over}, name=name)


OBSERVED = """max err / bound on the MI355X over the twenty rows, per output (the row that sets it):
pooled 0.3236 (C = 12), a 0.7328 (bias_300; 0.4973 otherwise), gate 0.4452 (bias_300; at most 0.1286 otherwise: the 2 ulp assumed
for expf hold with room), dy 0.0605, dw18 0.0021, dbias 0.0007, dgamma 0.0021, dbeta 0.0068, mean 0.2166 (bias_300), var 0.0199,
invstd 0.0959 (one_pixel).  The arg-max is equal everywhere; nothing is masked."""
