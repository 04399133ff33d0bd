"""Float64 reference, the per-element rounding bound and the case tables of the fused PFN training kernels (csrc/vfe_train.hip:
k_vfe_train_fwd<0|1|2>, k_vfe_reduce_rows, k_vfe_fin_stats, k_vfe_train_bwd1, k_vfe_fin_bwd1, k_vfe_train_bwd0, k_vfe_fin_bwd0), shared
by test_pfn_train_host.py (the file header's closed form in fp32 torch stands in for the kernels: the bound proves itself, the algebra
is checked against float64 autograd, and the reference with one mistake made falls outside the bound) and test_gpu_pfn_train.py (the
kernels against the same bound).  Plain torch, no GPU.  Q, qsum, gamma, used_fraction, caught_share and the constants come from
bn_train_cases.py / conv_direct_cases.py.

The reference takes exactly the fp32 numbers the entry points are handed (eps, voxel size and offsets cross the C interface as
floats), widened to float64, and restates the PFN part of torch_forms.vfe_train: x0 = [voxel, xyz - xyz.sum(1) / n, xyz - centre]
masked to the live slots; twice linear -> BatchNorm1d with batch statistics over all M * P slots (padded ones included) -> ReLU ->
max over the slots -> concat.  autograd64() differentiates exactly that; reference() follows the kernels' closed form of the same
gradients (dense BatchNorm term carried by the moments s = sum x, S = sum x x^T) in float64 and must agree with it.

The bound.  Every value is followed as Q = (float64 value, error bound) operation by operation from the kernels' source, as in
bn_train_cases.py.  T = sweeps(M) = ceil(ceil(M / 2) / 1024) is the number of pillars a half-wave takes (one sweep of the grid covers
256 workgroups x 4 waves x 2 = 2048 pillars).  The k of each fp32 sum (roundings on the longest path of a partial sum):

  * xyz.sum over the slots: a 5-step butterfly: k = 5; y0: a chain of 10 fmaf: k = 10; y1: of 32: k = 32.
  * statistics of y0 / y1, d beta0 / d gamma0: a lane's T pillars, the 5-step butterfly, the 8 half-waves one after the other in LDS:
    k = T + 13; the 256 workgroup rows meet in double (k64 = 256 + 8), mean / variance / invstd in double, one fp32 rounding each.
  * d beta1, d gamma1, sum g x1^T: lane-owned entries, no butterfly: k = T + 8.
  * s1, S1: a lane adds up to P + 1 rows per pillar (the padded row once, times its multiplicity: one rounding more): k = T (P + 1) + 9.
  * g_x1 of a slot: w + 32 fmaf of Q x1, then up to 64 fmaf of the channels whose arg-max the slot is: k = 96; the m0 half summed over
    the slots by a butterfly: k = 5, and added to the arg-max slot of z0.
  * sum g x0^T, s0, S0: a lane adds up to P rounded products per pillar: k = T P + 9.
  * the finishing kernels (dW1, Q, w, dW0) work in double on the double sums: their roundings are charged as U64 terms, then one
    fp32 rounding.

  * the gradients: the errors of the 160 batch statistics (mean and invstd of both layers) are the same numbers in every slot, so
    they are carried as common-mode quantities through the backward sums and cancel there as the values do (reference(): the
    interval chain with the statistics exact, plus |Jacobian of the closed form in the statistics| times their bounds, plus a
    second-order term); the rounding of everything else stays a worst case over the slots.

Nothing here is fitted to what a kernel returns.

Decisions the reference cannot make.  The ReLU of a0 / a1 and the arg-max of z0 / z1 are taken on computed values.  A decision whose
float64 margin is within the sum of the bounds of the two compared values is *undecided*: |a| against the bound of a for a ReLU; for
an arg-max the gap to any slot of a different value against the two slots' bounds on y, the linear output — the errors of the
statistics are common to the slots of a channel and cannot reorder them — plus the fp32 spacing at a (_decide).  Layer 1:
d_out[m, c] is set to 0 for every undecided (pillar, channel) before the kernel and the reference see it (reference()["d_out"];
share <= MASKED_CAP).  Layer 0: the count of
undecided decisions must be ZERO on every row (asserted from the reference alone by both tests), so no error is charged for them.
Slots whose float64 values agree to TIE64 (padded slots, duplicated points: identical inputs, identical fp32 results) are exact ties:
the lowest takes the gradient in the kernel and in torch, and the sums do not depend on which does.

Rows with M > 2048 are drawn from a pool of template pillars in a seeded random order (fresh random pillars always leave a few
layer-0 decisions undecided at that size); d_out stays random per pillar.  What this cannot see: a mix-up among pillars of the same
template (their forward values are identical, only d_out tells them apart).  On these rows d_out is drawn from 0.5 to 1.5: sums
over thousands of pillars of a signed d_out cancel to 1 / 60 of their terms, and a worst-case rounding bound, which cannot cancel,
would stand that much higher beside them.  The M = 2049 row gives its first and its last pillar 400 times the weight, so that
counting the one twice (the inactive half-wave) or losing the other (the second sweep) moves every sum.

Observed on the MI355X: see OBSERVED at the end of this file."""
import numpy as np
import torch

from bn_train_cases import Q, TINY, U64, caught_share, qsum, used_fraction  # noqa: F401  (re-exported to the tests)
from conv_direct_cases import SENTINEL, U, gamma  # noqa: F401

EPS = 1e-3
MASKED_CAP = 1e-3
TIE64 = 2.0 ** -40
LANES, C0, CIN, C1, K1 = 32, 16, 10, 64, 32
K_BLOCKS, K_WAVES = 256, 4
SWEEP = K_BLOCKS * K_WAVES * 2
VOXEL_SIZE = (0.16, 0.16, 3.0)
OFFSETS = (0.08, -19.76, -1.0)
GRID = (296, 248)                                   # x, y cells


# ------------------------------------------------------------------------------------------------ the kernels' launch arithmetic
def sweeps(M):
    """Trips of the grid-stride loop of k_vfe_train_* taken by the first wave of the first workgroup (the most any wave takes)."""
    return -(-((M + 1) // 2) // (K_BLOCKS * K_WAVES))


def last_sweep(M):
    """(pairs in the last sweep, whether its last pair has an inactive second half)."""
    pairs = (M + 1) // 2
    return pairs - (sweeps(M) - 1) * K_BLOCKS * K_WAVES, M % 2 == 1


def workspace_bytes():
    row = 2 * C1 + C1 * K1 + K1 + K1 * K1
    scratch = (4 * C0 + 4 * C1 + K1 * K1 + K1 + 2 * C1) * 4
    return K_BLOCKS * row * 4 + (2 + row + 2 * C1) * 8 + scratch + 256


# ------------------------------------------------------------------------------------------------ one case
def _seed(*row):
    return int(sum((int(v) + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


class Case:
    """Inputs of one row: voxels (M, P, 4), num (M,), coords (M, 4) [b, z, y, x], the two Linear weights and BatchNorm affines (every
    fifth gamma negative), d_out (M, 64).  counts: full | one | alt (1, P, 1, P, ...) | pm1 (P - 1) | mixed.  pool: the pillars are
    drawn from that many templates.  content: dirty_pad (the padded slots hold random points) | dup (slot 1 repeats slot 0) |
    corners (cells (0, 0) and (295, 247) in turn) | constant (every pillar is the same single point) | cluster (all points within
    a few cells of the far corner: |mean| / sigma of y0 is large).  affine: gamma0[3] = 0, gamma1[5] = 0, beta1[7] = -50."""

    def __init__(self, M, P, counts="mixed", pool=None, content=None, affine=False, dout_zero=False, dout_positive=False, plant=False, backward=True, seed=0, name=None):
        g = torch.Generator().manual_seed(_seed(M, P, seed))
        self.M, self.P, self.eps, self.backward, self.content = M, P, EPS, backward, content
        self.name = name or f"M{M}_P{P}_{counts}"
        T = pool or M
        if counts == "full":
            num = torch.full((T,), P)
        elif counts == "one":
            num = torch.ones(T, dtype=torch.long)
        elif counts == "alt":
            num = torch.where(torch.arange(T) % 2 == 0, 1, P)
        elif counts == "pm1":
            num = torch.full((T,), max(P - 1, 1))
        else:
            assert counts == "mixed", counts
            num = torch.randint(1, P + 1, (T,), generator=g)
        cx, cy = torch.randint(0, GRID[0], (T,), generator=g), torch.randint(0, GRID[1], (T,), generator=g)
        if content == "corners":
            cx, cy = torch.where(torch.arange(T) % 2 == 0, 0, GRID[0] - 1), torch.where(torch.arange(T) % 2 == 0, 0, GRID[1] - 1)
        elif content == "cluster":
            cx, cy = GRID[0] - 1 - torch.randint(0, 3, (T,), generator=g), GRID[1] - 1 - torch.randint(0, 3, (T,), generator=g)
        coords = torch.stack([torch.zeros(T, dtype=torch.long), torch.zeros(T, dtype=torch.long), cy, cx], 1)
        vs, off = torch.tensor(VOXEL_SIZE), torch.tensor(OFFSETS)
        centre = coords[:, [3, 2, 1]].float() * vs + off
        # points anywhere in the range, as test_gpu_train_ops.py draws them (points of one cell would differ by 1e-2 sigma between the
        # slots: one arg-max in a hundred would be undecided); the far cluster alone keeps its points inside their cells
        vox = torch.rand(T, P, 4, generator=g) * torch.tensor([47.0, 39.0, 3.0, 1.0]) + torch.tensor([0.0, -19.5, -2.5, 0.0])
        if content == "cluster":
            vox[:, :, :3] = centre[:, None, :] + (torch.rand(T, P, 3, generator=g) - 0.5) * vs
        if content == "constant":
            vox, coords, num = vox[:1, :1].expand(T, P, 4).clone(), coords[:1].expand(T, 4).clone(), torch.ones(T, dtype=torch.long)
        if content == "dup" and P > 1:
            vox[:, 1] = vox[:, 0]
        if content != "dirty_pad":
            vox = vox * (torch.arange(P).view(1, -1, 1) < num.view(-1, 1, 1))
        if pool:
            pick = torch.randint(0, pool, (M,), generator=g)
            vox, coords, num = vox[pick], coords[pick], num[pick]
            self.template = pick
        self.voxels, self.num, self.coords = vox.contiguous(), num.int(), coords.int().contiguous()
        sign = lambda n: torch.where(torch.arange(n) % 5 == 4, -1.0, 1.0)
        self.w0, self.w1 = torch.randn(C0, CIN, generator=g) * 0.3, torch.randn(C1, K1, generator=g) * 0.2
        self.gamma0, self.beta0 = (torch.rand(C0, generator=g) + 0.5) * sign(C0), torch.randn(C0, generator=g) * 0.3
        self.gamma1, self.beta1 = (torch.rand(C1, generator=g) + 0.5) * sign(C1), torch.randn(C1, generator=g) * 0.3
        if affine:
            self.gamma0[3], self.gamma1[5], self.beta1[7] = 0.0, 0.0, -50.0
        self.d_out = torch.zeros(M, C1) if dout_zero else torch.randn(M, C1, generator=g)
        if dout_positive:           # 0.5 to 1.5: the sums over thousands of pillars do not cancel, so their rounding bound is small beside them
            self.d_out = torch.rand(M, C1, generator=g) + 0.5
        if plant:                   # the first and the last pillar weigh 400 times the others: counting one twice or losing one moves every sum
            self.d_out[0] *= 400.0
            self.d_out[M - 1] *= 400.0

    def to(self, device):
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self


# ------------------------------------------------------------------------------------------------ Q helpers
def _lin(x, w, k):
    """x (.., n) Q times the exact weight rows w (c, n) as a sum of n products with k roundings on a path -> (.., c)."""
    wa = w.abs().t()
    S = x.hi() @ wa
    return Q(x.v @ w.t(), x.e @ wa + gamma(k) * S + k * TINY * (S > 0))


def _mm(a, b):
    """The exact product of two Q matrices (no rounding)."""
    return Q(a.v @ b.v, a.v.abs() @ b.e + a.e @ b.v.abs() + a.e @ b.e)


def _d64(q, ops=8):
    return Q(q.v, q.e + ops * U64 * q.hi())


def _sum_rows(q, k, k64):
    return qsum(Q(q.v.reshape(-1, q.v.shape[-1]), q.e.reshape(-1, q.e.shape[-1])), 0, k, k64)


def _gram(a, b, k, k64):
    """sum over the rows of a_i b_i^T (products rounded once: one more than k) -> (ca, cb)."""
    A, B = Q(a.v.reshape(-1, a.v.shape[-1]).t(), a.e.reshape(-1, a.e.shape[-1]).t()), Q(b.v.reshape(-1, b.v.shape[-1]), b.e.reshape(-1, b.e.shape[-1]))
    p = _mm(A, B)
    S = A.hi() @ B.hi()
    return Q(p.v, p.e + (gamma(k + 1) + k64 * U64) * S + (k + 1) * TINY * (S > 0))


def _batch_stats(y, wt, n, eps, k, k64, unbiased=False):
    """(mean, var, invstd rounded to fp32) of the slots of y (M, P, C) Q with multiplicities wt (M, P, 1) over the count n: fp32 partial
    sums of y and y^2 (fmaf) with k roundings on a path, met by k64 double additions; mu = s1 / n, var = s2 / n - mu^2 clamped at 0,
    invstd in double.  With y^ = y + d (|d| <= e) and r1, r2 the rounding of the two sums, exactly
        var^ - var = 2 / n sum (y - mu) d + 1 / n sum d^2 - 2 mu r1 / n - (mu^ - mu)^2 + r2 / n:
    the part of d that moves the mean does not move the variance."""
    yv, ye = (y.v * wt).reshape(-1, y.v.shape[-1]), (y.e * wt).reshape(-1, y.e.shape[-1])
    w = wt.reshape(-1, 1)
    hi = yv.abs() + ye
    g = gamma(k) + k64 * U64
    mu_v = yv.sum(0) / n
    r1 = g * hi.sum(0) / n + k * TINY
    d_mu = ye.sum(0) / n + r1
    yc, e1 = (y.v.reshape(-1, y.v.shape[-1]) - mu_v).abs() * w, y.e.reshape(-1, y.e.shape[-1])
    var_v = ((y.v.reshape(-1, y.v.shape[-1]) - mu_v) ** 2 * w).sum(0) / n - ((yv.sum(0) / n - mu_v) ** 2)
    if float(w.sum()) != n:                 # (a wrong count: the moments are no longer central)
        var_v = (y.v.reshape(-1, y.v.shape[-1]) ** 2 * w).sum(0) / n - mu_v ** 2
    r2 = g * ((y.v.reshape(-1, y.v.shape[-1]).abs() + e1) ** 2 * w).sum(0) / n + k * TINY
    d_var = 2.0 * (yc * e1).sum(0) / n + (e1 * e1 * w).sum(0) / n + 2.0 * mu_v.abs() * r1 + d_mu ** 2 + r2 + 8.0 * U64 * (var_v.abs() + mu_v ** 2)
    var_v = var_v.clamp_min(0.0)
    eps = float(np.float32(eps))
    vn = var_v * (n / (n - 1.0)) if unbiased else var_v
    inv_v = (vn + eps) ** -0.5
    invstd = Q(inv_v, 0.5 * d_var * ((var_v - d_var).clamp_min(0.0) + eps) ** -1.5 + 4.0 * U64 * inv_v).rnd()
    return Q(mu_v, d_mu + 2.0 * U64 * mu_v.abs()).rnd(), Q(var_v, d_var).rnd(), invstd


def _bn_relu(y, mean, invstd, gam, bet):
    """a = fmaf(y, scale, shift) with scale = fl(gamma invstd), shift = fl(beta - fl(mean scale)), through the identity
    y scale + shift = (y - mean) scale + beta + E (|E|: the two roundings inside shift), as bn_train_cases.reference does."""
    scale = (Q.exact(gam) * invstd).rnd()
    prod = mean * scale
    mprod = prod.rnd()
    diff = Q.exact(bet) - mprod
    E = mprod.e - prod.e + diff.rnd().e - diff.e
    core = Q(y.v - mean.v, y.e + mean.e) * scale + Q.exact(bet)
    return Q(core.v, core.e + E).rnd(), scale


def _decide(a, y, scale):
    """a, y (M, P, C) Q, scale (C,) Q -> (arg-max slot (M, C), lowest among exact ties; the maximum passes the ReLU (M, C); the ReLU of
    the maximum or the choice of the slot is undecided (M, C)).  The kernel's a^ = fl(fmaf(y^, scale^, shift^)) is monotone in y^ with one
    scale^ and shift^ for all slots of a channel, so two slots are ordered as their y^ are — the errors of the statistics are common to
    both — unless the two a^ round to one fp32 number: a rival is within the margin when its gap in y is within the two bounds on y
    plus 4 u |a| / |scale|, the spacing of fp32 numbers at a.  The ReLU of the maximum is decided on |a| against the whole bound of a."""
    best, _ = a.v.max(1)
    tol = TIE64 * (1.0 + best.abs())
    tied = a.v >= (best - tol)[:, None]
    am = tied.int().argmax(1)
    pick = lambda t: t.gather(1, am[:, None])[:, 0]
    e_am = pick(a.e)
    passed = best > 0
    relu_und = (best.abs() <= e_am) & (e_am > 0)
    s_lo = (scale.v.abs() - scale.e).clamp_min(TINY)
    spacing = 4.0 * U * (best.abs() + e_am + TINY) / s_lo
    gap = (pick(y.v)[:, None] - y.v).abs()
    arg_und = (~tied & (a.v + a.e > 0) & (gap <= pick(y.e)[:, None] + y.e + spacing[:, None])).any(1)          # (a slot the ReLU zeroes for sure is no rival)
    return am, passed, relu_und | (passed & arg_und)


WRONG = ("count_M32", "pad_not_in_stats", "pad_multiplicity_minus_1", "lanes_past_P_in_max", "dense_dropped_dW1", "dense_dropped_dW0",
         "m0_grad_not_routed", "inactive_half_as_pillar_0", "pillars_past_2048_lost", "mean_over_P", "centre_xz_swapped",
         "unbiased_normalising")


def _chain(c, wrong=None, local=False, d_out=None):
    """The interval chain.  local: the batch statistics (mean, invstd of both layers) are taken as exact numbers, so what is bounded
    is the rounding of everything else; d_out: the masked d_out of the full chain.
    -> dict of Q: out (M, 64), mean0, var0, mean1, var1, and with a backward dw0, dgamma0, dbeta0, dw1, dgamma1, dbeta1; plus
    d_out (fp32: the case's with the undecided layer-1 entries set to 0 — what the kernel must be handed), masked_share,
    undecided0 (count).  wrong: one of WRONG — the same formulas with that mistake made."""
    assert wrong is None or wrong in WRONG
    M, PS = c.M, c.P
    dev = c.voxels.device
    f64 = torch.float64
    T = sweeps(M)
    k64 = K_BLOCKS + 8
    one = torch.ones((), dtype=f64, device=dev)
    n = c.num.double()
    live = (torch.arange(PS, device=dev)[None, :] < c.num[:, None]).double()[..., None]          # (M, P, 1)
    # per-pillar multiplicity in every sum over the pillars
    wm = torch.ones(M, dtype=f64, device=dev)
    if wrong == "inactive_half_as_pillar_0":
        assert M % 2 == 1
        wm[0] = 2.0
    if wrong == "pillars_past_2048_lost":
        wm[SWEEP:] = 0.0
    count = float(M * (LANES if wrong == "count_M32" else PS))
    if wrong == "pad_not_in_stats":
        count = float(c.num.sum())
    in_stats = (live if wrong == "pad_not_in_stats" else torch.ones_like(live)) * wm[:, None, None]
    # load_rows
    xyz = Q.exact(c.voxels[:, :, :3])
    inv_n = Q(one / (n if wrong != "mean_over_P" else torch.full_like(n, PS))).rnd()
    mean = (qsum(xyz, 1, 5) * inv_n[:, None]).rnd()
    order = [1, 2, 3] if wrong == "centre_xz_swapped" else [3, 2, 1]
    vs, off = (torch.tensor(t, dtype=torch.float32, device=dev).double() for t in (VOXEL_SIZE, OFFSETS))
    centre = Q(c.coords[:, order].double() * vs + off).rnd()
    dm, dc = (xyz - mean[:, None]).rnd(), (xyz - centre[:, None]).rnd()
    x0 = Q(torch.cat([c.voxels.double(), dm.v, dc.v], -1) * live, torch.cat([torch.zeros_like(c.voxels, dtype=f64), dm.e, dc.e], -1) * live)
    w0, w1 = c.w0.double(), c.w1.double()
    r = {}

    def layer(x, w, k, gam, bet, tag):
        y = _lin(x, w, k)
        mu, var, inv = _batch_stats(y, in_stats, count, c.eps, T + 13, k64, wrong == "unbiased_normalising")
        r["mean" + tag], r["var" + tag] = mu, var
        if local:
            mu, inv = Q(mu.v), Q(inv.v)
        return (y, mu, inv) + _bn_relu(y, mu, inv, gam, bet)

    y0, mu0, inv0, a0, sc0 = layer(x0, w0, 10, c.gamma0, c.beta0, "0")
    z0 = a0.relu()
    am0, passed0, und0 = _decide(a0, y0, sc0)
    m0 = Q(z0.v.max(1)[0], z0.e.max(1)[0])
    if wrong == "lanes_past_P_in_max" and PS < LANES:                 # a lane past P computes a padded slot's value: y0 = 0
        pad = _bn_relu(Q(torch.zeros(C0, dtype=f64, device=dev)), mu0, inv0, c.gamma0, c.beta0)[0].relu()
        m0 = Q(torch.maximum(m0.v, pad.v), torch.maximum(m0.e, pad.e))
    x1 = Q(torch.cat([z0.v, m0.v[:, None].expand(-1, PS, -1)], -1), torch.cat([z0.e, m0.e[:, None].expand(-1, PS, -1)], -1))
    y1, mu1, inv1, a1, sc1 = layer(x1, w1, 32, c.gamma1, c.beta1, "1")
    z1 = a1.relu()
    r["out"] = Q(z1.v.max(1)[0], z1.e.max(1)[0])
    am1, passed1, und1 = _decide(a1, y1, sc1)
    relu0_und = ((a0.v.abs() <= a0.e) & (a0.e > 0))
    r["undecided0"] = int(relu0_und.sum()) + int(und0.sum())
    r["masked_share"] = float(und1.double().mean())
    r["d_out"] = torch.where(und1, torch.zeros_like(c.d_out), c.d_out) if d_out is None else d_out
    r["_theta"] = (mu0, inv0, mu1, inv1)
    r["_fixed"] = dict(x0=x0.v, am0=am0, am1=am1, passed1=passed1.double(), on0=(a0.v > 0).double(), count=count)
    if not c.backward or wrong == "lanes_past_P_in_max":
        return r
    # k_vfe_train_bwd1
    g1 = Q(r["d_out"].double() * passed1)                                                   # (M, 64), exact
    g1w = Q(g1.v * wm[:, None])
    hot1 = torch.arange(PS, device=dev)[None, :, None] == am1[:, None, :]                   # (M, P, 64)
    y_at = Q(y1.v.gather(1, am1[:, None])[:, 0], y1.e.gather(1, am1[:, None])[:, 0])
    xh1 = ((y_at - mu1).rnd() * inv1).rnd()
    db1, dg1 = qsum(g1w, 0, T + 8, k64), qsum(g1w * xh1, 0, T + 8, k64)
    idx = am1[:, :, None].expand(-1, -1, K1)                                                # x1 of the arg-max slot: (M, 64, 32)
    x1_at = Q(x1.v.gather(1, idx), x1.e.gather(1, idx))
    gw1 = qsum(Q(g1w.v[..., None]) * x1_at, 0, T + 8, k64)
    slot_w = torch.ones(M, PS, 1, dtype=f64, device=dev)
    if wrong == "pad_multiplicity_minus_1":
        slot_w[torch.arange(PS, device=dev)[None, :] == c.num[:, None]] = 0.0
    ks = T * (PS + 1) + 9
    xs = Q(x1.v * slot_w * wm[:, None, None], x1.e * slot_w * wm[:, None, None])
    s1, S1 = _sum_rows(xs, ks, k64), _gram(xs, x1, ks, k64)
    r["dbeta1"], r["dgamma1"] = db1.rnd(), dg1.rnd()

    def finish(gam, inv, mu, db, dg, gw, s, S, w, dense=True):
        """k_vfe_fin_bwd1 / k_vfe_fin_bwd0: c gw - (c / N) (db s^T + dg inv (W S - mu s^T)) in double, one fp32 rounding."""
        cc = Q.exact(gam) * inv
        ws = _mm(Q(w), S)
        inner = db[:, None] * s[None, :] + (dg * inv)[:, None] * (ws - mu[:, None] * s[None, :])
        d = (cc * Q(one / count))[:, None] * inner
        if not dense:
            d = Q(torch.zeros_like(d.v))
        return _d64(cc[:, None] * gw - d, 48).rnd(), cc

    r["dw1"], c1 = finish(c.gamma1, inv1, mu1, db1, dg1, gw1, s1, S1, w1, wrong != "dense_dropped_dW1")
    coef_q = c1 * inv1 * dg1 * Q(one / count)
    coef_w = c1 * (db1 - mu1 * inv1 * dg1) * Q(one / count)
    W1 = Q(w1)
    Qm = _d64(_mm(Q(w1.t()) * coef_q[None, :], W1), 72).rnd()                               # (32, 32)
    wv = _d64(_mm(coef_w[None, :], W1)[0], 72).rnd()                                        # (32,)
    # k_vfe_train_bwd0
    gc = ((Q.exact(r["d_out"]) * Q.exact(c.gamma1)).rnd() * inv1).rnd()
    G = Q(torch.where(hot1 & passed1[:, None], gc.v[:, None], torch.zeros_like(gc.v[:, None])),
          torch.where(hot1 & passed1[:, None], gc.e[:, None], torch.zeros_like(gc.e[:, None])))
    dense = _mm(x1, Q(Qm.v.t(), Qm.e.t()))
    sparse = _mm(G, W1)
    S = wv.hi() + x1.hi() @ Qm.hi().t() + G.hi() @ w1.abs()
    gx = Q(sparse.v - dense.v - wv.v, sparse.e + dense.e + wv.e + gamma(96) * S + 96 * TINY * (S > 0))          # (M, P, 32)
    gm = qsum(gx[:, :, C0:], 1, 5)
    if wrong == "m0_grad_not_routed":
        gm = Q(torch.zeros_like(gm.v))
    hot0 = torch.arange(PS, device=dev)[None, :, None] == am0[:, None, :]                   # (M, P, 16)
    routed = (gx[:, :, :C0] + gm[:, None]).rnd()
    gz = Q(torch.where(hot0, routed.v, gx.v[:, :, :C0]), torch.where(hot0, routed.e, gx.e[:, :, :C0]))
    on = (a0.v > 0).double() * wm[:, None, None]
    ga = Q(gz.v * on, gz.e * on)
    xh0 = ((y0 - mu0).rnd() * inv0).rnd()
    db0, dg0 = _sum_rows(ga, T + 13, k64), _sum_rows(ga * xh0, T + 13, k64)
    r["dbeta0"], r["dgamma0"] = db0.rnd(), dg0.rnd()
    k0 = T * PS + 9
    x0w = Q(x0.v * wm[:, None, None], x0.e * wm[:, None, None])
    gw0, s0, S0 = _gram(ga, x0, k0, k64), _sum_rows(x0w, k0, k64), _gram(x0w, x0, k0, k64)
    r["dw0"], _ = finish(c.gamma0, inv0, mu0, db0, dg0, gw0, s0, S0, w0, wrong != "dense_dropped_dW0")
    return r


# the factors of statistics in one term of a gradient, counted generously: dW0 has invstd0 four times (c0, the dense term's inv0,
# xhat0 in d gamma0, x1 in y1), invstd1 three times (c1, Q's inv1, xhat1 in d gamma1), and each mean at most twice
STAT_DEGREE = 12


def _closed64(c, d_out, fx, t):
    """The header's closed form in float64 with the decisions fixed (fx) and the 160 batch statistics t = [mu0 | inv0 | mu1 | inv1] as
    free numbers, as the backward kernels use them: the six gradients as one differentiable function of t."""
    mu0, inv0, mu1, inv1 = t[:C0], t[C0:2 * C0], t[2 * C0:2 * C0 + C1], t[2 * C0 + C1:]
    M, PS, N = c.M, c.P, fx["count"]
    dev = c.voxels.device
    w0, w1, g0, b0, g1_, b1 = (v.double() for v in (c.w0, c.w1, c.gamma0, c.beta0, c.gamma1, c.beta1))
    x0 = fx["x0"]
    y0 = x0 @ w0.t()
    z0 = ((y0 - mu0) * (g0 * inv0) + b0) * fx["on0"]
    slots = torch.arange(PS, device=dev)
    hot0 = (slots[None, :, None] == fx["am0"][:, None, :]).double()
    hot1 = (slots[None, :, None] == fx["am1"][:, None, :]).double()
    m0 = (z0 * hot0).sum(1)
    x1 = torch.cat([z0, m0[:, None].expand(-1, PS, -1)], -1)
    y1 = x1 @ w1.t()
    g = d_out.double() * fx["passed1"]
    y_at = (y1 * hot1).sum(1)
    db1, dg1 = g.sum(0), (g * (y_at - mu1) * inv1).sum(0)
    G = hot1 * g[:, None, :]                                                                # (M, P, 64)
    gw1 = G.reshape(-1, C1).t() @ x1.reshape(-1, K1)
    xf = x1.reshape(-1, K1)
    s1, S1 = xf.sum(0), xf.t() @ xf

    def finish(gam, inv, mu, db, dg, gw, s, S, w):
        cc = gam * inv
        return cc[:, None] * gw - (cc / N)[:, None] * (db[:, None] * s[None, :] + (dg * inv)[:, None] * (w @ S - mu[:, None] * s[None, :])), cc

    o = {}
    o["dw1"], c1 = finish(g1_, inv1, mu1, db1, dg1, gw1, s1, S1, w1)
    o["dbeta1"], o["dgamma1"] = db1, dg1
    Qm = (w1.t() * (c1 * inv1 * dg1 / N)) @ w1
    wv = (c1 * (db1 - mu1 * inv1 * dg1) / N) @ w1
    gx = (G * c1) @ w1 - (x1 @ Qm.t() + wv)
    gm = gx[:, :, C0:].sum(1)
    ga = (gx[:, :, :C0] + hot0 * gm[:, None]) * fx["on0"]
    gf, x0f = ga.reshape(-1, C0), x0.reshape(-1, CIN)
    db0, dg0 = gf.sum(0), (gf * ((y0 - mu0) * inv0).reshape(-1, C0)).sum(0)
    o["dw0"], _ = finish(g0, inv0, mu0, db0, dg0, gf.t() @ x0f, x0f.sum(0), x0f.t() @ x0f, w0)
    o["dbeta0"], o["dgamma0"] = db0, dg0
    return o


def reference(c, wrong=None):
    """The float64 values and their bounds (see _chain for the keys).  Forward outputs and statistics: the interval chain as it is.
    Gradients: the errors of the 160 batch statistics are COMMON to all slots, so they are carried as common-mode quantities:
        |computed - value| <= local + sum_j |d value / d t_j| dt_j + STAT_DEGREE rho / 2 * worst
    local: the interval chain with the statistics taken as exact (the rounding of everything else, times 1 + 1e-3 for being taken
    at t instead of the computed t^);  d value / d t_j: the Jacobian of the closed form with the decisions fixed (_closed64), so the
    statistics' errors cancel across the slots as the values do;  dt_j: the bounds of the interval chain on mean and invstd;  the
    last term is the second order: every term of a gradient is a product of at most STAT_DEGREE statistics, so its second-order
    change is at most STAT_DEGREE rho / 2 times its first-order change taken without cancellation, which `worst` — the interval
    chain's own bound, statistics included — covers (rho: the largest relative dt_j, the means measured in units of 1 / invstd)."""
    full = _chain(c, wrong)
    if wrong is not None or "dw0" not in full:
        return full
    loc = _chain(c, None, local=True, d_out=full["d_out"])
    theta = full["_theta"]
    t = torch.cat([q.v for q in theta])
    dt = torch.cat([q.e for q in theta])
    mu0, inv0, mu1, inv1 = theta
    rho = float(torch.cat([inv0.e / inv0.v, mu0.e * inv0.v, inv1.e / inv1.v, mu1.e * inv1.v]).max())
    fn = lambda tt: _closed64(c, full["d_out"], full["_fixed"], tt)
    val = fn(t)
    step = 160 if c.M * c.P <= 4096 else 16            # (forward mode, a block of statistics at a time: the tangents of (M, P, 64) tensors)
    parts = [torch.func.jacfwd(lambda tc, a=a: fn(torch.cat([t[:a], tc, t[a + step:]])))(t[a:a + step]) for a in range(0, t.numel(), step)]
    jac = {k: torch.cat([p_[k] for p_ in parts], -1) for k in GRADS}
    for k in GRADS:
        assert float((val[k] - full[k].v).abs().max()) <= 1e-9 * max(float(full[k].v.abs().max()), 1e-3), k
        first = (jac[k].abs() * dt).sum(-1)
        full["worst_" + k] = full[k]
        full[k] = Q(full[k].v, loc[k].e * (1.0 + 1e-3) + first + 0.5 * STAT_DEGREE * rho * full[k].e)
    return full


def autograd64(c, d_out):
    """The PFN part of torch_forms.vfe_train in float64, differentiated by autograd: out, the batch statistics and the six gradients."""
    p = [t.double().clone().requires_grad_(True) for t in (c.w0, c.gamma0, c.beta0, c.w1, c.gamma1, c.beta1)]
    vox, n = c.voxels.double(), c.num.double()
    dev = vox.device
    xyz = vox[:, :, :3]
    mean = xyz.sum(dim=1, keepdim=True) / n.view(-1, 1, 1)
    vs, off = (torch.tensor(t, dtype=torch.float32, device=dev).double() for t in (VOXEL_SIZE, OFFSETS))
    centre = c.coords[:, [3, 2, 1]].double() * vs + off
    mask = (torch.arange(c.P, device=dev).view(1, -1) < c.num.view(-1, 1)).unsqueeze(-1).double()
    x = torch.cat([vox, xyz - mean, xyz - centre.unsqueeze(1)], dim=-1) * mask
    o = {}
    eps = float(np.float32(c.eps))
    for i, (w, g, b) in enumerate((p[:3], p[3:])):
        y = x @ w.t()
        flat = y.reshape(-1, y.shape[-1])
        m, v = flat.mean(0), flat.var(0, unbiased=False)
        o[f"mean{i}"], o[f"var{i}"] = m.detach(), v.detach()
        y = torch.relu((y - m) / torch.sqrt(v + eps) * g + b)
        ymax = y.max(dim=1, keepdim=True)[0]
        x = ymax if i == 1 else torch.cat([y, ymax.expand(-1, c.P, -1)], dim=2)
    out = x.reshape(c.M, -1)
    o["out"] = out.detach()
    if c.backward:
        grads = torch.autograd.grad(out, p, d_out.double())
        o.update(dict(zip(("dw0", "dgamma0", "dbeta0", "dw1", "dgamma1", "dbeta1"), grads)))
    return o


# ------------------------------------------------------------------------------------------------ the fp32 stand-in
def _psum(t):
    """fp32 rows (R, ..) -> their sum: fp32 partial sums of 64 rows each, met in double."""
    R = t.shape[0]
    pad = -R % 64
    t = torch.cat([t, t.new_zeros((pad,) + t.shape[1:])]) if pad else t
    return t.view(-1, 64, *t.shape[1:]).sum(1, dtype=torch.float32).double().sum(0)


def _pgram(a, b):
    """fp32 rows a (R, ca), b (R, cb) -> sum of a_i b_i^T, in the same partial sums."""
    R = a.shape[0]
    pad = -R % 64
    if pad:
        a, b = torch.cat([a, a.new_zeros(pad, a.shape[1])]), torch.cat([b, b.new_zeros(pad, b.shape[1])])
    return (a.view(-1, 64, a.shape[1]).transpose(1, 2) @ b.view(-1, 64, b.shape[1])).double().sum(0)


def standin(c, d_out):
    """The kernels' formulas in fp32 torch: the forward, and the CLOSED FORM of the file header for the gradients (no autograd):
    dW = c sum g x^T - (c / N)(dbeta s^T + dgamma inv (W S - mu s^T)), g_x1 = sum_c c1 g W1[c] - (Q x1 + w), the same one level down."""
    f32 = torch.float32
    M, PS = c.M, c.P
    N = float(M * PS)
    eps = float(np.float32(c.eps))
    num = c.num
    live = (torch.arange(PS)[None, :] < num[:, None]).float()[..., None]
    xyz = c.voxels[:, :, :3]
    mean = xyz.sum(1, dtype=f32) * (1.0 / num.float())[:, None]
    centre = c.coords[:, [3, 2, 1]].float() * torch.tensor(VOXEL_SIZE) + torch.tensor(OFFSETS)
    x0 = torch.cat([c.voxels, xyz - mean[:, None], xyz - centre[:, None]], -1) * live
    o = {}

    def layer(x, w, gam, bet, tag):
        y = x @ w.t()
        flat = y.reshape(-1, y.shape[-1])
        mu = _psum(flat) / N
        var = (_psum(flat * flat) / N - mu * mu).clamp_min(0.0)
        inv = (1.0 / torch.sqrt(var + eps)).float()
        o["mean" + tag], o["var" + tag] = mu.float(), var.float()
        scale = gam * inv
        shift = bet - mu.float() * scale
        return y, mu.float(), inv, y * scale + shift

    y0, mu0, inv0, a0 = layer(x0, c.w0, c.gamma0, c.beta0, "0")
    z0 = torch.relu(a0)
    m0, am0 = z0.max(1)
    x1 = torch.cat([z0, m0[:, None].expand(-1, PS, -1)], -1)
    y1, mu1, inv1, a1 = layer(x1, c.w1, c.gamma1, c.beta1, "1")
    z1 = torch.relu(a1)
    out, am1 = z1.max(1)
    o["out"] = out
    if not c.backward:
        return o
    g1 = torch.where(out > 0, d_out, torch.zeros_like(d_out))
    y_at = y1.gather(1, am1[:, None])[:, 0]
    db1, dg1 = _psum(g1), _psum(g1 * ((y_at - mu1) * inv1))
    x1_at = x1.gather(1, am1[:, :, None].expand(-1, -1, K1))
    gw1 = _psum(g1[..., None] * x1_at)
    xf = x1.reshape(-1, K1)
    s1, S1 = _psum(xf), _pgram(xf, xf)

    def finish(gam, inv, mu, db, dg, gw, s, S, w):
        cc = gam.double() * inv.double()
        ws = w.double() @ S
        dense = (cc / N)[:, None] * (db[:, None] * s[None, :] + (dg * inv.double())[:, None] * (ws - mu.double()[:, None] * s[None, :]))
        return (cc[:, None] * gw - dense).float(), cc

    o["dw1"], c1 = finish(c.gamma1, inv1, mu1, db1, dg1, gw1, s1, S1, c.w1)
    o["dbeta1"], o["dgamma1"] = db1.float(), dg1.float()
    coef_q = c1 * inv1.double() * dg1 / N
    coef_w = c1 * (db1 - mu1.double() * inv1.double() * dg1) / N
    Qm = ((c.w1.double().t() * coef_q) @ c.w1.double()).float()
    wv = (coef_w @ c.w1.double()).float()
    gc = g1 * c.gamma1 * inv1
    G = torch.zeros(M, PS, C1).scatter_(1, am1[:, None], gc[:, None])
    gx = G @ c.w1 - (x1 @ Qm.t() + wv)
    gm = gx[:, :, C0:].sum(1, dtype=f32)
    gz = gx[:, :, :C0] + torch.zeros(M, PS, C0).scatter_(1, am0[:, None], gm[:, None])
    ga = torch.where(z0 > 0, gz, torch.zeros_like(gz))
    gf, x0f = ga.reshape(-1, C0), x0.reshape(-1, CIN)
    db0, dg0 = _psum(gf), _psum(gf * ((y0 - mu0) * inv0).reshape(-1, C0))
    gw0, s0, S0 = _pgram(gf, x0f), _psum(x0f), _pgram(x0f, x0f)
    o["dw0"], _ = finish(c.gamma0, inv0, mu0, db0, dg0, gw0, s0, S0, c.w0)
    o["dbeta0"], o["dgamma0"] = db0.float(), dg0.float()
    return o


FORWARD = ("out", "mean0", "var0", "mean1", "var1")
GRADS = ("dw0", "dgamma0", "dbeta0", "dw1", "dgamma1", "dbeta1")


def fractions(got, r):
    return {k: used_fraction(got[k], r[k]) for k in FORWARD + GRADS if k in r}


# ------------------------------------------------------------------------------------------------ the table
# name -> Case keywords, with the seed under which the row has no undecided layer-0 decision, and what the row is there for
ROWS = {
    "one_pillar": dict(M=1, P=32, counts="mixed"),                           # half-wave 1 inactive from the start
    "one_pair_one_slot": dict(M=2, P=1, counts="full"),                      # no padded slot, no choice of maximum
    "three_pillars_two_slots": dict(M=3, P=2, counts="alt"),
    "eight_pillars": dict(M=8, P=5, counts="mixed"),
    "nine_pillars_31": dict(M=9, P=31, counts="mixed"),                      # one lane past the slots
    "all_full_32": dict(M=9, P=32, counts="full"),                           # wpad == 0: the padded row is written by lane 0
    "all_full_20": dict(M=8, P=20, counts="full"),
    "all_one_point": dict(M=9, P=20, counts="one"),
    "one_next_to_full": dict(M=9, P=32, counts="alt"),                       # n_loop is the larger of the pair
    "all_but_one_slot": dict(M=8, P=20, counts="pm1"),
    "dirty_padding": dict(M=9, P=20, counts="mixed", content="dirty_pad"),   # the mean sums the padded slots, the features mask them
    "duplicated_points": dict(M=9, P=5, counts="full", content="dup"),       # exact ties between live slots: the lowest takes the gradient
    "grid_corners": dict(M=8, P=5, counts="mixed", content="corners"),
    # variance of y0 and y1 exactly 0: inv = 1 / sqrt(eps).  Statistics and forward only, and of the forward only the four statistics
    # are really pinned: the bound on y - mu is a worst-case sum times 1 / sqrt(eps), twice over, so every a1 is beta1 within its
    # bound, `out` is bounded no tighter than |a1| on most entries (layer-1 undecided share 0.83), and a backward would be masked whole
    "constant_batch": dict(M=9, P=1, counts="full", content="constant", backward=False),
    "affine_edges": dict(M=9, P=20, counts="mixed", affine=True),            # gamma0 == 0, gamma1 == 0, a channel whose maximum is 0
    "d_out_zero": dict(M=9, P=20, counts="mixed", dout_zero=True),           # every gradient exactly zero
    # |mean| / sigma of y0 in the hundreds: the cancellation of E[y^2] - mu^2.  Statistics and forward only: the bound on a0 grows with it
    "far_cluster": dict(M=50, P=5, counts="full", content="cluster", backward=False),          # (full: a padded slot's y0 = 0 would be the spread)
    # the sweep edges, from templates: the last pillar of the first sweep alone in its pair, the full sweep, one pillar of a second
    # sweep beside an inactive half, and a third sweep
    "sweep_minus_1": dict(dout_positive=True, M=2047, P=4, counts="mixed", pool=64),
    "sweep_exact": dict(dout_positive=True, M=2048, P=5, counts="mixed", pool=64),
    "sweep_plus_1": dict(dout_positive=True, plant=True, M=2049, P=20, counts="mixed", pool=48),
    "three_sweeps": dict(dout_positive=True, M=4100, P=8, counts="mixed", pool=96),
}
SEEDS = {"all_full_32": 1, "all_but_one_slot": 2, "affine_edges": 1}

# wrong variant -> [(row name, the outputs on which the touched elements must be outside the bound)]
WRONG_CASES = {
    "count_M32": [("all_but_one_slot", ("mean0", "mean1"))],
    "pad_not_in_stats": [("all_one_point", ("mean0", "mean1", "var1"))],
    "pad_multiplicity_minus_1": [("all_one_point", ("dw1",))],
    "lanes_past_P_in_max": [("all_full_20", ("mean1", "var1", "out"))],
    "dense_dropped_dW1": [("eight_pillars", ("dw1",)), ("three_sweeps", ("dw1",))],
    "dense_dropped_dW0": [("eight_pillars", ("dw0",)), ("three_sweeps", ("dw0",))],
    "m0_grad_not_routed": [("eight_pillars", ("dbeta0", "dgamma0", "dw0")), ("three_sweeps", ("dbeta0", "dgamma0", "dw0"))],
    "inactive_half_as_pillar_0": [("nine_pillars_31", ("mean0", "var0", "mean1", "var1", "dbeta1", "dbeta0", "dgamma0", "dw0")),
                                  ("sweep_plus_1", ("dbeta1", "dbeta0", "dgamma0", "dw0"))],
    "pillars_past_2048_lost": [("three_sweeps", ("mean0", "mean1", "dbeta1", "dbeta0", "dgamma0", "dw0")),
                               ("sweep_plus_1", ("dbeta1", "dbeta0", "dgamma0", "dw0"))],
    "mean_over_P": [("eight_pillars", ("mean0", "var0"))],
    "centre_xz_swapped": [("eight_pillars", ("mean0", "var0"))],
    "unbiased_normalising": [("eight_pillars", ("out",))],
}


def case(name, **over):
    kw = {**ROWS[name], **over}
    kw.setdefault("seed", SEEDS.get(name, 0))
    return Case(**kw, name=name)


OBSERVED = """max err / bound on the MI355X over the twenty-one rows, per output: out 0.0383, mean0 0.0639, var0 0.0941, mean1 0.0121,
var1 0.0643, dw1 0.0400, dgamma1 0.0197, dbeta1 0.1872, dw0 0.0011, dgamma0 0.0004, dbeta0 0.0008.  Masked layer-1 share: 0 on the
rows with M <= 9 and at M = 2049, 7.71e-04 / 2.29e-04 / 4.80e-04 at M = 2047 / 2048 / 4100; no undecided layer-0 decision anywhere.

How sharp the bound is (bound / largest element).  Forward outputs and statistics: 1e-6 to 3e-4.  Gradients on the rows with
M from 3 to 9: dW1 2e-4 to 2e-3, d gamma1 1e-4 to 7e-4, d beta1 1e-6, dW0 3e-3 to 4e-2, d gamma0, d beta0 2e-3 to 2e-2; the rows
of one pillar and of two slots in all are there for their edges, not their sharpness (a BatchNorm over two slots has xhat = +-1:
dW0 stands at 0.3 and 3e2 of the largest element there).  On the sweep rows: dW1 5e-4 to 1e-3, d gamma1 1e-4 to 2e-4, d beta1 7e-7,
dW0 8e-3 to 1e-2, d gamma0 3e-3 to 1e-2, d beta0 4e-3 to 9e-3.  With the statistics' errors common-mode
what is left is the rounding of everything else, taken as a worst case in which the roundings of every slot push the same way;
the layer-0 gradients are sums over all M P slots of terms that cancel, and no deterministic bound cancels with them: the fp32
closed form uses 1e-4 to 4e-3 of the bound there.  test_pfn_train_host.py states, per wrong variant and row, the share of the
touched elements the bound catches and which elements escape."""
