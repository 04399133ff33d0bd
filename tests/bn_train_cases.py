"""Float64 reference, the per-element rounding bound and the case tables of the training BatchNorm + ReLU kernels
(csrc/conv_train.hip: k_bn_reduce<false|true>, k_bn_finalize, k_bn_finalize4, k_bn_affine, k_bn_apply, k_bn_bwd_apply), shared by
test_bn_train_host.py (the kernel's formula in fp32 torch stands in for the kernel: the bound proves itself, and the reference with
one term lost falls outside it) and test_gpu_bn_train.py (the kernels against the same bound).  Plain torch / numpy, no GPU.

The reference takes exactly the fp32 numbers the kernels are handed (eps and momentum included: they cross the C interface as
floats), widened to float64, and evaluates train-mode BatchNorm: mean, biased variance, invstd = 1 / sqrt(var + eps); the running
statistics with the unbiased factor n / max(n - 1, 1); y = [gate *] relu(scale * z + shift) [+ resid] with scale = gamma * invstd,
shift = beta - mean * scale; d beta = sum dy_m, d gamma = sum dy_m * xhat, dz = scale * (dy_m - s1 / n - xhat * s2 / n) with
dy_m = [gate *] dy where the ReLU passed; d gate = sum_c relu(a) * dy.

The bound.  Every value the kernels compute is followed as a pair Q = (float64 value v, error bound e): |computed - v| <= e.

  * One fp32 operation on computed operands: the exact operation's error propagates (|a| e_b + |b| e_a + e_a e_b for a product,
    e_a + e_b for a sum), then the rounding adds u (|v| + e) + 2**-126, u = 2**-24 (Q.rnd; the additive term is the flush of a
    subnormal result, as in conv_direct_cases.bound, and is left out only where value and error are exactly zero: 0 is computed
    exactly).  A fused multiply-add is a product and a sum with ONE rounding; where the compiler may contract a * b + c the
    uncontracted form is bounded, whose bound holds for the contracted one (it has one rounding fewer).
  * A sum of n terms with at most k fp32 roundings on the path of any partial sum, in ANY order within that structure (Higham,
    Accuracy and Stability of Numerical Algorithms, §4.2): |computed - sum v_i| <= sum e_i + gamma(k) * sum (|v_i| + e_i) + k * 2**-126,
    gamma(n) = n u / (1 - n u)  (qsum).  For k_bn_reduce a partial sum's path is: a thread's <= ceil(slab / lanes) pixels over four
    accumulators, their 3 meetings, then <= lanes additions in LDS: k = ceil(slab / lanes) + lanes + 3 (reduce_k; slab and lanes
    capped by P where the pass is smaller than one slab: adding an exact zero does not round), with
    slab = bn_slab(P), lanes = max(256 / (C / 4), 1) restated here from the kernel and pinned by the GPU test against
    hvpr_bn_workspace_bytes.  sum x^2 and sum dy_m * xhat accumulate by fmaf: the product is not rounded, the same k holds.  The rows
    of the workspace meet in double (k_bn_finalize / k_bn_finalize4): gamma64(rows + 8) with u64 = 2**-53, then one fp32 rounding.
  * Statistics, in this order:  d_mean = gamma(k) E|x|;  d_var = gamma(k) E[x^2] + 2 |m| d_mean + d_mean^2 (the clamp at 0 moves
    towards the true var >= 0);  d_invstd = 1/2 d_var (max(var - d_var, 0) + eps)^(-3/2) (mean value theorem; the computed variance
    is >= 0);  each then rounded to fp32 once.  scale, shift, the running statistics, y, the backward sums (their own k) and dz
    follow operation by operation from the kernels' source; the pre-activation alone is bounded through the identity
    z scale + (beta - mean scale) = (z - mean) scale + beta, which keeps the one error of scale from being counted twice.
  * d gate: 4 roundings in the thread (product + 3 additions), log2(min(C/4, 64)) butterfly steps and ceil(C/4 / 64) atomic additions
    when C/4 is a power of two, else C/4 atomic additions (dgate_k).

Nothing here is fitted to what a kernel returns.

Conditioning.  The kernel's formula var = E[x^2] - m^2 on fp32 partial sums loses |mean|^2 / var of its relative accuracy: at
|mean| / sigma = 16 and k = 37 the bound on var is ~2e-3 * var (3 gamma(k) E[x^2] / var; the row "cond16", whose channels spread
around that ratio, reaches 2.6e-3 and shows the bound scale with it; at |mean| / sigma <= 1, the activations of this network, it is
4e-6 at k = 23 and 1.3e-5 at k = 132).  That is a limit of the formula, not of the bound; a shifted or
Welford form would remove it and is a different kernel.

The ReLU mask.  The kernels mask on fmaf(z, scale, shift) > 0 in fp32.  Where the float64 pre-activation a64 has |a64| <= delta_a
(delta_a: the bound on the computed pre-activation, > 0) the kernel's decision is not determined by the reference: the element is
*undecided*.  It is left out of the element-wise dz check only; its |dy_m| (and through the products |dy_m * xhat|) is added to the
error of its term in d beta / d gamma, and so through s1 / n, s2 / n to every dz bound.  y and d gate need no exclusion: ReLU is
1-Lipschitz.  The undecided share of a case is computed from the reference alone and must stay <= UNDECIDED_CAP."""
import math

import numpy as np
import torch

from conv_direct_cases import SENTINEL, SLICE_EXTRA, SLICE_OFF, U, gamma

TINY = 2.0 ** -126
U64 = 2.0 ** -53
EPS = 1e-3
UNDECIDED_CAP = 1e-3


# ------------------------------------------------------------------------------------------------ the kernels' launch arithmetic
def bn_slab(P):
    slab = 2048
    while slab > 64 and P // slab < 2048:
        slab >>= 1
    return slab


def bn_lanes(C):
    return max(256 // (C // 4), 1)


def bn_blocks(P):
    return -(-P // bn_slab(P))


def workspace_bytes(P, C):
    return bn_blocks(P) * 2 * C * 4


def reduce_k(P, C):
    """Roundings on the longest path of a partial sum of k_bn_reduce.  A workgroup holds at most min(slab, P) pixels: its threads
    take at most ceil(that / lanes) each, and only min(lanes, that) of the LDS additions add anything but an exact zero."""
    pix, lanes = min(bn_slab(P), P), bn_lanes(C)
    return -(-pix // lanes) + min(lanes, pix) + 3


def reduce_trips(P, C):
    """{(trips of the 4-way unrolled loop, trips of the remainder loop)} over every live thread of every workgroup of k_bn_reduce."""
    slab, lanes = bn_slab(P), bn_lanes(C)
    out = set()
    for blk in {0, bn_blocks(P) - 1}:                      # (all full blocks are alike)
        p0, p1 = blk * slab, min(blk * slab + slab, P)
        for pl in range(lanes):
            n = len(range(p0 + pl, p1, lanes))
            out.add((n // 4, n % 4))
    return out


def apply_grid(P, C):
    n4 = P * (C // 4)
    return min(-(-n4 // 256), 16384)


def apply_trips(P, C):
    """(trips of the grid-stride loop of k_bn_apply / k_bn_bwd_apply, float4 elements of the last trip, threads of the grid)."""
    n4, threads = P * (C // 4), apply_grid(P, C) * 256
    trips = -(-n4 // threads)
    return trips, n4 - (trips - 1) * threads, threads


def dgate_atomics_meet(C):
    """More than one atomicAdd lands on a pixel's d gate: its fp32 sum depends on their order."""
    g = C // 4
    return g & (g - 1) != 0 or g > 64


def dgate_k(C):
    g = C // 4
    if g & (g - 1) == 0:
        return 4 + int(math.log2(min(g, 64))) + -(-g // 64)
    return 4 + g


# ------------------------------------------------------------------------------------------------ value and error bound
class Q:
    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def exact(t):
        return Q(t.double())

    @staticmethod
    def num(x, like):
        return Q(torch.full((), float(x), dtype=torch.float64, device=like.v.device))

    def hi(self):
        return self.v.abs() + self.e

    def rnd(self):
        h = self.hi()
        return Q(self.v, self.e + U * h + TINY * (h > 0))

    def __mul__(self, o):
        return Q(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __add__(self, o):
        return Q(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return Q(self.v - o.v, self.e + o.e)

    def relu(self):
        return Q(torch.relu(self.v), self.e)

    def __getitem__(self, i):
        return Q(self.v[i], self.e[i])


def qsum(q, dim, k, k64=0):
    S = q.hi().sum(dim)
    return Q(q.v.sum(dim), q.e.sum(dim) + (gamma(k) + (k64 + 0.0) * U64) * S + k * TINY * (S > 0))


def used_fraction(got, q, skip=None):
    """max over the elements (all but `skip`) of |got - q.v| / q.e: <= 1 means inside the bound everywhere.  Only an exact match
    counts as 0 (0 / 0 included); an element that is not a number, infinite, or off where the bound is zero counts as inf."""
    err = (got.double() - q.v).abs()
    assert err.shape == q.e.shape, (err.shape, q.e.shape)
    frac = torch.where(err == 0, torch.zeros_like(err), err / q.e)
    frac = torch.where(torch.isnan(frac), torch.full_like(frac, float("inf")), frac)
    if skip is not None:
        frac = torch.where(skip, torch.zeros_like(frac), frac)
    return float(frac.max()) if frac.numel() else 0.0


def caught_share(q, bad, touched):
    """Share of the `touched` elements on which the wrong value `bad` is outside the bound around the reference."""
    assert bool(touched.any()), "the wrong variant touches no element"
    out = ~((bad - q.v).abs() <= q.e)            # "not inside": a NaN is outside
    return float(out[touched].double().mean())


# ------------------------------------------------------------------------------------------------ one case
def _seed(*row):
    return int(sum((int(v) + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


class Case:
    """Inputs of one row.  z (P, C); dy (P, C) — inside dy_wide (P, C + SLICE_EXTRA) at SLICE_OFF when `sliced`, the other columns
    random; gate (P,), resid (P, C) when `gated`; gamma with every third channel negative; running buffers unless running=False.
    edge: channels 0, 1, 2 get gamma = 0 with beta = 0, < 0, > 0.  plant: pixel index whose z is mean + 3 sigma towards the side the
    ReLU passes, with dy = 3, in every channel."""

    def __init__(self, P, C, relu=True, gated=False, sliced=False, momentum=0.1, running=True, mean=0.5, sigma=2.0, edge=False,
                 plant=None, parts=None, backward=True, seed=0, name=None):
        g = torch.Generator().manual_seed(_seed(P, C, seed))
        self.P, self.C, self.relu, self.gated, self.sliced, self.momentum, self.eps = P, C, relu, gated, sliced, momentum, EPS
        self.parts, self.plant, self.edge, self.backward = parts, plant, edge, backward
        self.name = name or f"P{P}_C{C}"
        mu_c = mean * (1.0 + 0.1 * torch.randn(C, generator=g))
        sg_c = sigma * (0.75 + 0.5 * torch.rand(C, generator=g))
        unit = torch.randn(P, C, generator=g)
        self.gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0)
        self.beta = torch.randn(C, generator=g) * 0.3
        dy = torch.randn(P, C, generator=g) + 1.0 + 0.5 * unit
        if plant is not None:
            unit[plant] = 3.0 * torch.sign(self.gamma)
            dy[plant] = 3.0
        self.z = unit * sg_c + mu_c
        if edge:
            self.gamma[:3] = 0.0
            self.beta[:3] = torch.tensor([0.0, -0.5, 0.5])
        self.dy_wide = None
        if sliced:
            self.dy_wide = torch.randn(P, C + SLICE_EXTRA, generator=g)
            self.dy_wide[:, SLICE_OFF:SLICE_OFF + C] = dy
        self.dy = dy
        self.gate = torch.rand(P, generator=g) * 1.5 - 0.25 if gated else None
        self.resid = torch.randn(P, C, generator=g) if gated else None
        self.running_mean = torch.randn(C, generator=g) * 0.1 if running else None
        self.running_var = torch.rand(C, generator=g) + 0.5 if running else None

    def to(self, device):
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self


def stats_q(m, var, e_abs, e_sq, eps, k, k64):
    """(mean, var, invstd) as Q from the float64 moments m, var, E|x|, E[x^2]: fp32 partial sums with k roundings on a path, k64
    double additions of the finalising kernel, one rounding to fp32 each."""
    g = gamma(k) + k64 * U64
    d_m = g * e_abs + k * TINY
    d_var = g * e_sq + k * TINY + 2.0 * m.abs() * d_m + d_m * d_m + 4.0 * U64 * (e_sq + m * m)
    eps = float(np.float32(eps))
    invstd = (var + eps) ** -0.5
    d_is = 0.5 * d_var * ((var - d_var).clamp_min(0.0) + eps) ** -1.5 + 4.0 * U64 * invstd
    return Q(m, d_m).rnd(), Q(var, d_var).rnd(), Q(invstd, d_is).rnd()


WRONG = ("lost_slab_pixel", "lost_partial_row", "unbiased_normalising", "biased_running", "s1_dropped", "s2_dropped", "mask_ge",
         "gate_not_in_sums", "dgate_without_relu", "slice_offset_ignored")


def reference(c, wrong=None):
    """-> dict of Q: mean, var, invstd, scale, shift, running_mean, running_var (when the case has them), y, dbeta, dgamma, dz,
    dgate (gated), and `undecided` (bool, (P, C)).  parts = (Pa, Pb): the backward sums are taken per part (dbeta_0, dgamma_0,
    dbeta_1, dgamma_1), added in double and divided by the count before the fp32 rounding, as sync_backward_sums does.
    wrong: one of WRONG — the same formulas with that mistake made."""
    assert wrong is None or wrong in WRONG
    z = c.z.double()
    P, C = z.shape
    n = float(P)
    k, k64 = reduce_k(P, C), bn_blocks(P) + 8
    if wrong in ("lost_slab_pixel", "lost_partial_row"):
        keep = torch.ones(P, 1, dtype=torch.float64, device=z.device)
        if wrong == "lost_slab_pixel":
            keep[c.plant] = 0.0
        else:
            keep[(bn_blocks(P) - 1) * bn_slab(P):] = 0.0
        m = (z * keep).sum(0) / n
        var = (z * z * keep).sum(0) / n - m * m
    else:
        keep = None
        m = z.mean(0)
        var = ((z - m) ** 2).mean(0)
    r = {}
    var_n = var * (n / (n - 1.0)) if wrong == "unbiased_normalising" else var
    mean, r["var"], invstd = stats_q(m, var_n, z.abs().mean(0), (z * z).mean(0), c.eps, k, k64)
    if wrong == "unbiased_normalising":
        r["var"] = stats_q(m, var, z.abs().mean(0), (z * z).mean(0), c.eps, k, k64)[1]
    r["mean"], r["invstd"] = mean, invstd
    # k_bn_affine
    scale = (Q.exact(c.gamma) * invstd).rnd()
    mprod = (mean * scale).rnd()
    shift = (Q.exact(c.beta) - mprod).rnd()
    r["scale"], r["shift"] = scale, shift
    if c.running_mean is not None:
        m_f = float(np.float32(c.momentum))
        keep_f = Q.num(1.0 - m_f, mean).rnd()
        mu = Q.num(c.momentum * (1.0 if wrong == "biased_running" else n / max(n - 1.0, 1.0)), mean).rnd()
        r["running_mean"] = (Q.num(m_f, mean) * mean + (Q.exact(c.running_mean) * keep_f).rnd()).rnd()
        r["running_var"] = (mu * r["var"] + (Q.exact(c.running_var) * keep_f).rnd()).rnd()
    # k_bn_apply
    zq = Q.exact(c.z)
    # a = fmaf(z, scale^, shift^) with shift^ = fl(beta - fl(mean^ scale^)): z scale^ + shift^ = (z - mean^) scale^ + beta + E exactly,
    # |E| <= the two roundings inside shift^.  The errors of z scale^ and mean^ scale^ are one error, not two: bounded together
    # (bounded apart, |mean| d_scale would enter a twice, and all of it at P = 1 where z = mean)
    E = (mean * scale).rnd().e - (mean * scale).e + (Q.exact(c.beta) - mprod).rnd().e - (Q.exact(c.beta) - mprod).e
    core = Q(zq.v - mean.v, mean.e.expand_as(zq.v)) * scale + Q.exact(c.beta)
    a = Q(core.v, core.e + E).rnd()
    act = a.relu() if c.relu else a
    gq = Q.exact(c.gate[:, None]) if c.gated else None
    r["y"] = (gq * act + Q.exact(c.resid)).rnd() if c.gated else act
    if not c.backward:
        return r
    # k_bn_reduce<true>, k_bn_bwd_apply
    if c.sliced:
        off = 0 if wrong == "slice_offset_ignored" else SLICE_OFF
        dy = Q.exact(c.dy_wide[:, off:off + C])
    else:
        dy = Q.exact(c.dy)
    und = (a.v.abs() <= a.e) & (a.e > 0) if c.relu else torch.zeros_like(a.v, dtype=torch.bool)
    r["undecided"] = und
    passed = (a.v >= 0) if wrong == "mask_ge" else (a.v > 0)

    def masked(d):
        if not c.relu:
            return d
        zero = torch.zeros_like(d.v)
        return Q(torch.where(passed, d.v, zero), torch.where(passed, d.e, zero) + torch.where(und, d.hi(), zero))
    dm = masked((dy * gq).rnd() if c.gated else dy)
    dm_sums = masked(dy) if (c.gated and wrong == "gate_not_in_sums") else dm
    if keep is not None:            # the lost pixels are lost to the backward sums as well (the same loops)
        dm_sums = Q(dm_sums.v * keep, dm_sums.e * keep)
    xhat = ((zq - mean).rnd() * invstd).rnd()
    inv_n = Q.num(1.0 / n, mean).rnd()
    if c.parts is None:
        s1, s2 = qsum(dm_sums, 0, k, k64).rnd(), qsum(dm_sums * xhat, 0, k, k64).rnd()
        t1, t2 = (s1 * inv_n).rnd(), (s2 * inv_n).rnd()
        r["dbeta"], r["dgamma"] = s1, s2
    else:
        assert sum(c.parts) == P
        tot1 = tot2 = None
        lo = 0
        for j, Pj in enumerate(c.parts):
            kj, k64j = reduce_k(Pj, C), bn_blocks(Pj) + 8
            s1 = qsum(dm_sums[lo:lo + Pj], 0, kj, k64j).rnd()
            s2 = qsum((dm_sums * xhat)[lo:lo + Pj], 0, kj, k64j).rnd()
            r[f"dbeta_{j}"], r[f"dgamma_{j}"] = s1, s2
            tot1, tot2 = (s1 if tot1 is None else tot1 + s1), (s2 if tot2 is None else tot2 + s2)
            lo += Pj
        exact_inv = Q.num(1.0 / n, mean)
        t1, t2 = (tot1 * exact_inv).rnd(), (tot2 * exact_inv).rnd()        # double until the cast; inv_count = 1 multiplies exactly
        r["dbeta"], r["dgamma"] = tot1, tot2
    if wrong == "s1_dropped":
        t1 = Q(torch.zeros_like(t1.v))
    if wrong == "s2_dropped":
        t2 = Q(torch.zeros_like(t2.v))
    r["dz"] = (scale * ((dm - t1).rnd() - (xhat * t2).rnd()).rnd()).rnd()
    if c.gated:
        r["dgate"] = qsum((a if wrong == "dgate_without_relu" else act) * dy, 1, dgate_k(C))
    return r


# ------------------------------------------------------------------------------------------------ the fp32 stand-in
def _fma(a, b, c):
    """fmaf in torch: the product of two fp32 numbers is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _slab_partials(t, P, C):
    """fp32 (P, C) terms -> the workspace rows (blocks, C) of k_bn_reduce: per thread over its pixels, then over the lanes, in fp32."""
    slab, lanes, blocks = bn_slab(P), bn_lanes(C), bn_blocks(P)
    J = -(-slab // lanes)
    t = torch.nn.functional.pad(t, (0, 0, 0, blocks * slab - P)).view(blocks, slab, C)
    t = torch.nn.functional.pad(t, (0, 0, 0, J * lanes - slab)).view(blocks, J, lanes, C)
    return t.sum(1, dtype=torch.float32).sum(1, dtype=torch.float32)


def standin(c):
    """The kernels' formulas in fp32 torch: fp32 partial sums in the slab / lane structure, the finalise in double.  (The stand-in
    rounds the products of sum x^2 and sum dy_m xhat once more than the kernels' fmaf; the first addition to a zero accumulator is
    exact, which k counts, so the bound still covers it.)"""
    f32 = torch.float32
    z, P, C = c.z, c.P, c.C
    n = float(P)
    eps = float(np.float32(c.eps))
    a_sum, b_sum = _slab_partials(z, P, C).double().sum(0), _slab_partials(z * z, P, C).double().sum(0)
    m = a_sum / n
    var = (b_sum / n - m * m).clamp_min(0.0)
    o = {"mean": m.float(), "var": var.float(), "invstd": (1.0 / torch.sqrt(var + eps)).float()}
    mean, invstd = o["mean"], o["invstd"]
    scale = c.gamma * invstd
    shift = c.beta - mean * scale
    o["scale"], o["shift"] = scale, shift
    if c.running_mean is not None:
        m_f = torch.tensor(c.momentum, dtype=f32)
        mu_f = torch.tensor(c.momentum * n / max(n - 1.0, 1.0), dtype=f32)
        o["running_mean"] = _fma(m_f, mean, c.running_mean * (1.0 - m_f))
        o["running_var"] = _fma(mu_f, o["var"], c.running_var * (1.0 - m_f))
    a = _fma(z, scale, shift)
    act = torch.relu(a) if c.relu else a
    o["y"] = _fma(c.gate[:, None], act, c.resid) if c.gated else act
    if not c.backward:
        return o
    dy = c.dy_wide[:, SLICE_OFF:SLICE_OFF + C] if c.sliced else c.dy
    d = dy * c.gate[:, None] if c.gated else dy
    if c.relu:
        d = torch.where(a > 0, d, torch.zeros_like(d))
    xhat = (z - mean) * invstd
    inv_n = torch.tensor(1.0 / n, dtype=f32)
    if c.parts is None:
        s1 = _slab_partials(d, P, C).double().sum(0).float()
        s2 = _slab_partials(d * xhat, P, C).double().sum(0).float()
        t1, t2 = s1 * inv_n, s2 * inv_n
    else:
        t1 = t2 = 0.0
        lo = 0
        for j, Pj in enumerate(c.parts):
            s1 = _slab_partials(d[lo:lo + Pj], Pj, C).double().sum(0).float()
            s2 = _slab_partials((d * xhat)[lo:lo + Pj], Pj, C).double().sum(0).float()
            o[f"dbeta_{j}"], o[f"dgamma_{j}"] = s1, s2
            t1, t2 = t1 + s1.double(), t2 + s2.double()
            lo += Pj
        s1, s2 = t1, t2
        t1, t2 = (t1 / n).float(), (t2 / n).float()
    o["dbeta"], o["dgamma"] = s1, s2
    o["dz"] = scale * (d - t1 - xhat * t2)
    if c.gated:
        o["dgate"] = (act * dy).sum(1, dtype=f32)
    return o


OUTPUTS = ("mean", "var", "invstd", "scale", "shift", "running_mean", "running_var", "y", "dbeta", "dgamma", "dz", "dgate")


def fractions(got, r):
    """name -> max err / bound for every output both sides have (dz without the undecided elements)."""
    return {k: used_fraction(got[k], r[k], r["undecided"] if k == "dz" else None) for k in r if k != "undecided" and k in got}


def undecided_share(r):
    return float(r["undecided"].double().mean()) if "undecided" in r else 0.0


# ------------------------------------------------------------------------------------------------ finalising synthetic partial rows
class Partials:
    """hvpr_bn_finalize_partials_f32 on `rows` synthetic workspace rows [sum x | sum x^2] of three values each: count = 3 * rows."""

    def __init__(self, rows, C):
        rng = np.random.default_rng(_seed(rows, C, 5))
        x = rng.standard_normal((rows, 3, C)) * 2.0 + 0.5
        self.rows, self.C, self.count, self.eps = rows, C, 3 * rows, EPS
        self.partials = torch.from_numpy(np.stack([x.sum(1), (x * x).sum(1)], 1).astype(np.float32))        # (rows, 2, C)

    def reference(self, wrong=None):
        p = self.partials.numpy().astype(np.longdouble)
        if wrong == "lost_partial_row":
            p = p[:-1]
        s = p.sum(0)
        m = s[0] / self.count
        var = s[1] / self.count - m * m
        t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
        e_abs, e_sq = np.abs(p).sum(0)[0] / self.count, np.abs(p).sum(0)[1] / self.count
        mean, var, invstd = stats_q(t(m), t(var), t(e_abs), t(e_sq), self.eps, 0, self.rows + 8)
        return {"mean": mean, "var": var, "invstd": invstd}

    def standin(self):
        s = self.partials.double().sum(0)
        m = s[0] / self.count
        var = (s[1] / self.count - m * m).clamp_min(0.0)
        return {"mean": m.float(), "var": var.float(), "invstd": (1.0 / torch.sqrt(var + float(np.float32(self.eps)))).float()}


# ------------------------------------------------------------------------------------------------ the tables
# name -> Case keywords.  Every row runs statistics, affine, forward and backward.
SHAPES = {
    "one_pixel": dict(P=1, C=8),                              # count 1: factor max(n - 1, 1), variance 0
    "fewer_pixels_than_lanes": dict(P=5, C=8),                # 128 lanes
    "one_ragged_block": dict(P=60, C=64),                     # slab 64, 16 lanes: 12 threads take 4 pixels (unrolled), 4 take 3 (remainder)
    "one_lane": dict(P=70, C=1024),                           # 256 groups: 16 unrolled trips; last block 1 unrolled + 2 remainder
    "twelve_groups": dict(P=200, C=48),                       # 21 lanes, 252 live threads; d gate by atomics
    "slab_128": dict(P=262144 + 5, C=8),                      # 128 lanes: one pixel per thread, remainder loop only; 2049 rows
    "slab_256": dict(P=524288 + 3, C=32),                     # 32 lanes: two unrolled trips, no remainder in a full block; 2049 rows
    "whole_slabs": dict(P=128, C=16),
    "one_past_a_slab": dict(P=129, C=16),
    # |mean| / sigma = 16: the cancellation of E[x^2] - m^2.  Statistics and forward only: the bound on the pre-activation grows
    # with it (~0.03), and with it the undecided share of a backward (~2e-2, far above the cap)
    "cond16": dict(P=4185, C=32, mean=32.0, sigma=2.0, backward=False),
}
AFFINE = {
    "momentum_0.01": dict(P=60, C=64, momentum=0.01),
    "momentum_1": dict(P=60, C=64, momentum=1.0),
    "no_running_buffers": dict(P=60, C=64, running=False),
    "two_affine_blocks": dict(P=9, C=260),                    # C > 256: num_batches_tracked must still grow by exactly 1
}
FORWARD = {
    "sliced": dict(P=37, C=32, sliced=True),                  # y into, dy out of, a channel slice of a wider tensor
    "gated": dict(P=37, C=32, gated=True),
    "gated_sliced_dy": dict(P=37, C=32, gated=True, sliced=True),
    "no_relu": dict(P=37, C=32, relu=False),
    "no_relu_gated": dict(P=37, C=32, relu=False, gated=True),
}
DGATE = {f"dgate_groups_{c // 4}": dict(P=37, C=c, gated=True) for c in (8, 32, 256, 1024, 48)}
MULTI_TRIP = {
    "two_trips_butterfly": dict(P=16400, C=1024, gated=True),
    "two_trips_atomics": dict(P=350000, C=48, gated=True),
}
EDGE = {"gamma_zero": dict(P=60, C=8, edge=True, gated=True)}
TWO_PART = {"two_parts": dict(P=200, C=48, parts=(137, 63)), "two_parts_gated": dict(P=200, C=32, parts=(1, 199), gated=True)}

SMALL = {**{k: v for k, v in SHAPES.items() if v["P"] < 100000}, **AFFINE, **FORWARD, **DGATE, **EDGE, **TWO_PART}
LARGE = {**{k: v for k, v in SHAPES.items() if v["P"] >= 100000}, **MULTI_TRIP}
ROWS = {**SMALL, **LARGE}

FINALIZE_ROWS = (1, 63, 257, 1030)
FINALIZE_C = (4, 6, 7, 68)

# wrong variant -> (Case keywords of the inputs built for it, the outputs on which every touched element must be outside the bound)
# P = 189: three blocks of slab 64, the last holds 61 pixels
WRONG_CASES = {
    "lost_slab_pixel": (dict(P=189, C=16, plant=127), ("mean", "var", "dbeta", "dgamma")),      # the last pixel of the second slab
    "lost_partial_row": (dict(P=189, C=16, plant=188), ("mean", "var", "dbeta", "dgamma")),
    "unbiased_normalising": (dict(P=189, C=16), ("invstd", "scale")),
    "biased_running": (dict(P=189, C=16), ("running_var",)),
    "s1_dropped": (dict(P=189, C=16), ("dz",)),
    "s2_dropped": (dict(P=189, C=16), ("dz",)),
    "mask_ge": (dict(P=60, C=8, edge=True, gated=True), ("dbeta", "dgamma")),
    "gate_not_in_sums": (dict(P=189, C=16, gated=True), ("dbeta", "dgamma")),
    "dgate_without_relu": (dict(P=189, C=16, gated=True), ("dgate",)),
    "slice_offset_ignored": (dict(P=189, C=16, sliced=True), ("dbeta", "dgamma", "dz")),
}


def case(name, **over):
    return Case(**{**ROWS[name], **over}, name=name)
