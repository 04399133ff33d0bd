"""Float64 reference, the per-element rounding bound and the case tables of the memory addressing training kernels
(csrc/memory_train.hip: k_bank_pack_f32, k_memtrain_fwd, k_memtrain_bwd_rows, k_memtrain_bwd_items, k_memtrain_items_reduce), shared by
test_memory_train_host.py (the kernels' formulas in fp32 torch stand in for the kernels: the bound proves itself, and the reference
with one mistake made falls outside it) and test_gpu_memory_train.py (the kernels against the same bound).  Plain torch, no GPU.
Q, qsum, gamma, used_fraction, caught_share and the constants come from bn_train_cases.py / conv_direct_cases.py; added here are only
the reciprocal and the division whose bound comes from the interval [v - e, v + e] (_recip, _div), a sum whose k differs from row
to row (_ksum), and the two shrink functions bounded over the interval of a.

The reference takes exactly the fp32 x, bank, dy and shrink threshold the entry points are handed (the threshold crosses the C
interface as a float), widened to float64, and evaluates in closed form
    l = x W^T,  a = softmax(l),  s = (a - lam) a / ((a - lam) + eps) on a > lam, else 0,  n = sum s,  t = s / max(n, eps),  y = t W
    dt = dy W^T,  q = sum_S t dt,  ds = (dt - q) / n,  da = ds hs'(a),  c = sum_S a da,  dl = a (da - c),
    dx = sum_S a da w - c (a W),  dW_j = sum_r [ dl_rj x_r + t_rj dy_r ]
with hs'(a) = (u^2 + eps (a + u)) / (u + eps)^2, u = a - lam, and eps the fp32 number nearest 1e-12 (the kernel's 1e-12f, and what the
fp32 module adds).  Outputs: y, stats (mx, Z, n, 0), crow (c, q), dx, dW.  The host test checks the values against torch autograd of
torch_forms.hard_shrink_relu in float64.

The bound.  Every value is followed as Q = (float64 value, error bound) operation by operation from the source, as in
bn_train_cases.py.  Per value:

  * logits        K = 64 terms on chained fp32 MFMAs: 16 v_mfma_f32_16x16x4_f32 in the forward and in bwd_rows, 32 v_mfma_f32_32x32x2_f32
                  in bwd_items.  ASSUMED, as in conv_wino_cases.py: a K slot of an fp32 MFMA costs at most a rounded product and a rounded
                  accumulate, in whatever order the unit takes the slots: gamma(2 K) sum |x| |w| (LOGIT_K = 128) holds for both
                  shapes.  bwd_items works from its own logits but the forward's mx and Z: the same expression bounds its a.
  * mx            the exact maximum of computed logits: its error is the largest logit error of the row.  a = v / Z does not depend
                  on which number near the maximum is subtracted, so mx's error is charged to mx and to the Z that is reported, and
                  to a only through the rounding of the subtraction (_softmax).
  * exp_nonpos    v_exp_f32 on a rounded product, corrected to first order by two fmaf.  No statement of its accuracy ships with ROCm,
                  so it is ASSUMED to return exp of its fp32 argument within EXP_ULP = 2 ulp (<= 4 u relative) plus 2^-126 (the flush of a
                  subnormal); the argument's own error (the subtraction of mx rounds once) propagates by expm1.  An argument below the
                  -150 clamp has a float64 value below 2^-126 as well.  Items past n_items add exact zeros.
  * Z             32 serial additions of a lane, of which only the ceil(n_items / 64) slices that hold items add anything but an exact
                  zero, and 6 butterfly steps: z_k = ceil(n_items / 64) + 6 (38 at n_items > 1984).   a = v (1 / Z): a correctly rounded
                  reciprocal and a product.
  * hard_shrink, hard_shrink_grad   as functions F(a, u), H(a, u) of the computed a and u = fl(a - lam), bounded by the mean value
                  theorem over the interval of a: |dF/da| <= 1, |dF/du| <= a eps / (u_lo + eps)^2, |dH/da| <= eps / d_lo^2,
                  |dH/du| <= eps (2 a + u + eps) / d_lo^3 with u_lo = u - du, d_lo = u_lo + eps; then 3 and 8 roundings of the
                  expressions themselves (every term is positive).  Plain Q arithmetic would charge da / u for a ratio u / (u + eps)
                  that does not move with u.
  * over the support S   n, y (fmaf chain), q (fmaf chain), c and dxs (fmaf chain) are chains of |S| roundings, row by row (_ksum).
                  Each dt of bwd_rows is a once-rounded product and a 64-lane butterfly: DT_K = 7; bwd_items takes dt on the MFMAs (128).
  * a W           a wave's share of n4 = ceil(n_items / 4) k-steps (4 items each, 2 roundings an item) and 16 partial sums added
                  serially: abar_k = 8 ceil(n4 / 16) + 16.   dx = dxs - c (a W), bounded uncontracted.
  * dW            a split's row tiles on the MFMAs, the x and the dy products into the same accumulator: 4 roundings a row, 64 rows a
                  tile, ceil(row tiles / 32) tiles; then 32 serial additions: dw_k = 256 ceil(row_tiles / 32) + 32.
  The bound follows no correlation: a row whose support is one item has y = w_j whatever s_j is, yet is charged twice the error of s_j.

The support decision is the one discontinuity: a_j > lam is taken in fp32, by the forward and bwd_rows on one a and by bwd_items on
another.  Where |a64_j - lam| <= delta a_j the reference cannot take it.  A row with such an item is *undecided*; the case generator
draws every row from its own seed and draws it again with the next seed while any item lies within NEAR * delta a_j of lam, so the
undecided share of every row of the table is exactly 0, from the reference alone.  NEAR = 4 keeps u_lo >= 3 delta a > 0: the interval
bound of hard_shrink_grad stays finite (and small: eps lam / (3 delta a)^3 delta a).  The row near_threshold keeps N_FREE rows
within 3 fp32 ulps of lam on both sides with dy = 0: there y and dx need only be finite, crow is exactly 0, and such a row adds
exactly 0 to dW whichever way it is decided (dt = 0, so q = c = 0 and cx = 0; cy multiplies dy = 0).

Nothing here is fitted to what a kernel returns.  What each row is for stands next to it in ROWS.

Observed on the MI355X: see OBSERVED at the end of this file."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from bn_train_cases import Q, TINY, U64, caught_share, qsum, used_fraction  # noqa: F401  (re-exported to the tests)
from conv_direct_cases import SENTINEL, U, gamma  # noqa: F401

KC, ROWS_WG, WAVES, ITEMS_MAX, IB, RT, SPLITS = 64, 16, 16, 2048, 128, 64, 32
LAMBDA = 0.0025
EPS32 = float(np.float32(1e-12))
EXP_ULP = 2.0
NEAR = 4.0
N_FREE = 8
LOGIT_K, DT_K = 2 * KC, 7


# ------------------------------------------------------------------------------------------------ the kernels' launch arithmetic
def n_tiles(n_items):
    return -(-n_items // 16)


def first(wid, block):
    """The first 16-item tile wave `wid` of workgroup `block` takes; it goes on in steps of 16."""
    return (wid + block) % WAVES


def row_groups(R):
    return -(-R // ROWS_WG)


def row_tiles(R):
    return -(-R // RT)


def tiles_per_split(R):
    return -(-row_tiles(R) // SPLITS)


def split_tiles(R, split):
    per = tiles_per_split(R)
    return range(split * per, min(row_tiles(R), split * per + per))


def n4(n_items):
    return -(-n_items // 4)


def n4_per_wave(n_items):
    return -(-n4(n_items) // WAVES)


def ipad(n_items):
    return -(-n_items // IB) * IB


def workspace_bytes(n_items):
    return n_tiles(n_items) * 16 * KC * 4 + SPLITS * ipad(n_items) * KC * 4 + 256


def z_k(n_items):
    return -(-n_items // 64) + 6


def abar_k(n_items):
    return 8 * n4_per_wave(n_items) + WAVES


def dw_k(R):
    return 4 * RT * tiles_per_split(R) + SPLITS


# ------------------------------------------------------------------------------------------------ what Q lacks
def _recip(q):
    """1 / q over [v - e, v + e], v - e > 0, before the rounding of the division."""
    lo = q.v - q.e
    assert bool((lo > 0).all())
    return Q(1.0 / q.v, q.e / (q.v * lo))


def _div(p, q):
    """p / q over the interval of q, q.v - q.e > 0, before the rounding of the division."""
    lo = q.v - q.e
    assert bool((lo > 0).all())
    return Q(p.v / q.v, (p.e * q.v + p.v.abs() * q.e) / (q.v * lo))


def _ksum(q, dim, k):
    """qsum with a tensor k (the chain length differs from row to row)."""
    S = q.hi().sum(dim)
    return Q(q.v.sum(dim), q.e.sum(dim) + gamma(k) * S + k * TINY * (S > 0))


def _kmm(q, w, k):
    """q (Q) @ w (exact) as sums with k roundings on a path; k a number or a column."""
    S = q.hi() @ w.abs()
    return Q(q.v @ w, q.e @ w.abs() + gamma(k) * S + k * TINY * (S > 0))


def _mask(q, m):
    z = torch.zeros_like(q.v)
    return Q(torch.where(m, q.v, z), torch.where(m, q.e, z))


def _exp(d):
    ev = torch.exp(d.v)
    ee = ev * torch.expm1(d.e)
    return Q(ev, ee + 2.0 * EXP_ULP * U * (ev + ee) + TINY)


def _u_interval(a, lam, hit, strict):
    u = a.v - lam
    du = a.e + U * (u.abs() + a.e) + TINY
    lo = u - du
    if strict:
        assert bool((lo[hit] > 0).all()), "an item of the support within the error of a of the threshold"
    return u, du, torch.where(hit, lo, torch.ones_like(lo)).clamp_min(TINY)


def _shrink(a, lam, hit, eps, strict):
    u, du, lo = _u_interval(a, lam, hit, strict)
    val = a.v * u / (u + eps)
    err = a.e + du * a.hi() * eps / (lo + eps) ** 2
    return _mask(Q(val, err + gamma(3) * (val.abs() + err) + TINY), hit)


def _shrink_grad(a, lam, hit, eps, strict):
    u, du, lo = _u_interval(a, lam, hit, strict)
    d_lo = lo + eps
    val = (u * u + eps * (a.v + u)) / (u + eps) ** 2
    err = a.e * eps / d_lo ** 2 + du * eps * (2.0 * a.hi() + u.abs() + du + eps) / d_lo ** 3
    return _mask(Q(val, err + gamma(8) * (val.abs() + err) + TINY), hit)


def _softmax(x, bank):
    """-> a, mx, Z as Q from fp32 x (rows, 64) and bank: the part of the chain the support decision rests on."""
    xd, wd = x.double(), bank.double()
    S = xd.abs() @ wd.abs().t()
    l = Q(xd @ wd.t(), gamma(LOGIT_K) * S + KC * TINY * (S > 0))
    mx = Q(l.v.max(1)[0], l.e.max(1)[0])
    # a = v / Z does not depend on WHICH number near the maximum is subtracted: with m the computed maximum, v_j = exp(l_j - m) is
    # followed for that m; only the rounding of the subtraction sees m's error.  v and Z then carry the common factor
    # exp(mx64 - m) within exp(+-mx.e): it cancels in a (a.e is widened by it for the additive 2^-126 terms) and is charged to the Z
    # that is reported
    d = l - Q(mx.v[:, None])
    v = _exp(Q(d.v, d.e + U * (d.v.abs() + d.e + mx.e[:, None]) + TINY))
    Z = qsum(v, 1, z_k(bank.shape[0]))
    a = (v * _recip(Z).rnd()[:, None]).rnd()
    grow = torch.exp(mx.e)
    return Q(a.v, a.e * grow[:, None]), mx, Q(Z.v, Z.e * grow + Z.hi() * grow * torch.expm1(mx.e))


# ------------------------------------------------------------------------------------------------ one case
def _seed(*row):
    return int(sum((int(v) + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


MAX_DRAWS = 64


def _borders(n_items):
    """Items on each side of every border an item walk of the kernels has: the ends, a 16-item tile, a 64-item slice, a 128-item block
    (which is also the border between two waves' shares of n4 where n4_per_wave = 32), the last full tile, slice and block."""
    b = [0, n_items - 1, 15, 16, 63, 64, 127, 128, 4 * n4_per_wave(n_items) - 1, 4 * n4_per_wave(n_items),
         16 * (n_items // 16) - 1, 16 * (n_items // 16), 64 * (n_items // 64) - 1, 64 * (n_items // 64),
         IB * (n_items // IB) - 1, IB * (n_items // IB), 4 * n4_per_wave(n_items) * (WAVES - 1) - 1, 4 * n4_per_wave(n_items) * (WAVES - 1)]
    return [j for j in b if 0 <= j < n_items]


class Case:
    """Inputs of one row of the table: x (R, 64), bank (n_items, 64) uniform in +-1/8 scaled x4, dy (R, 64), lam.  A row of x is
    relu(randn(64)) * scale / 4 drawn from the row's own seed.  content:
      planted       row r adds 6 relu(w_j) with j = _borders(n_items)[r % len]: item j dominates the row's support
      empty_all     scale 0.5: no softmax value reaches lam
      mixed_groups  scale 0.5 (empty) and `scale` (live) rows by MIXED_LIVE
      one_item      x_r = 60 w_j, j = (37 r) % n_items: a_j ~ 1, most other exponentials underflow
      ties          every fourth row is x = 0: all a are equal
    near_by (>= NEAR): the row is drawn again while an item lies within near_by * delta a of lam.
      near          the first N_FREE rows are moved until their item nearest lam lies within 3 fp32 ulps of it, above for even rows and
                    below for odd ones, with dy = 0"""

    def __init__(self, R, n_items=2000, lam=LAMBDA, scale=8.0, content=None, relu=True, dy_zero=False, seed=0, name=None,
                 allow_undecided=False, near_by=NEAR):
        assert near_by >= NEAR
        self.R, self.n_items, self.scale, self.content, self.seed = R, n_items, scale, content, seed
        self.lam = float(np.float32(lam))
        self.name = name or f"R{R}_n{n_items}"
        base = _seed(R, n_items, seed)
        g = torch.Generator().manual_seed(base)
        self.bank = (torch.rand(n_items, KC, generator=g) * 2 - 1) / 8 * 4
        self.dy = torch.zeros(R, KC) if dy_zero else torch.randn(R, KC, generator=g)
        self.free = torch.zeros(R, dtype=torch.bool)
        self._relu = relu
        draws = torch.zeros(R, dtype=torch.long)
        self.x = torch.stack([self._row(base, r, 0) for r in range(R)]) if R else torch.zeros(0, KC)
        fixed = torch.zeros(R, dtype=torch.bool)
        if content == "ties":
            fixed[0::4] = True
            self.x[fixed] = 0.0
        todo = torch.arange(R)[~fixed]
        while todo.numel():
            a, _, _ = _softmax(self.x[todo], self.bank)
            near = ((a.v - self.lam).abs() <= near_by * a.e).any(1)
            todo = todo[near]
            draws[todo] += 1
            assert not todo.numel() or int(draws.max()) < MAX_DRAWS
            for r in todo.tolist():
                self.x[r] = self._row(base, r, int(draws[r]))
        self.draws = draws
        if content == "near":
            for r in range(N_FREE):
                self.x[r] = _move_to_threshold(self.x[r], self.bank, self.lam, above=r % 2 == 0)
            self.free[:N_FREE] = True
            self.dy[:N_FREE] = 0.0
        if not allow_undecided and R:
            a, _, _ = _softmax(self.x, self.bank)
            und = ((a.v - self.lam).abs() <= near_by * a.e).any(1)
            assert torch.equal(und, self.free), (self.name, "rows near the threshold that no redraw can move")

    def _row(self, base, r, draw):
        g = torch.Generator().manual_seed((base % (2 ** 31 // (MAX_DRAWS * 4096)) * 4096 + r) * MAX_DRAWS + draw)
        t = torch.randn(KC, generator=g)
        t = torch.relu(t) if self._relu else t
        sc = self.scale
        if self.content == "empty_all" or (self.content == "mixed_groups" and not MIXED_LIVE(r)):
            sc = 0.5
        row = t * sc / 4
        if self.content == "planted":
            b = _borders(self.n_items)
            row = row + 6.0 * torch.relu(self.bank[b[r % len(b)]])
        elif self.content == "one_item":
            row = 60.0 * self.bank[(37 * r) % self.n_items] + 0.01 * row
        return row

    def to(self, device):
        c = copy.copy(self)
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(c, k, v.to(device))
        return c


def MIXED_LIVE(r):
    """mixed_groups, R = 200: rows 0-63 alternate; the 64-row tile 64-127 is empty (four whole groups); group 128-143 is live, group
    144-159 empty; from 160 two rows in three are live."""
    if r < 64:
        return r % 2 == 0
    if r < 128:
        return False
    if r < 144:
        return True
    if r < 160:
        return False
    return r % 3 != 0


def _move_to_threshold(x, bank, lam, above):
    """Scale the fp32 row x, then move one component ulp by ulp, until the float64 softmax value of the item nearest lam lies within
    3 fp32 ulps of lam on the asked side.  From the reference alone."""
    wd = bank.double()
    ulp = float(np.spacing(np.float32(lam)))
    soft = lambda row: torch.softmax(row.double() @ wd.t(), 0)
    a = soft(x)
    j = int((a - lam).abs().argmin())
    ok = lambda v: (0.0 < v - lam <= 3 * ulp) if above else (0.0 < lam - v <= 3 * ulp)
    lo, hi = 0.8, 1.25                   # a_j of the scaled row crosses lam between them, or the item is no use
    f = lambda s: float(soft((x.double() * s).float())[j]) - lam
    assert f(lo) * f(hi) < 0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(lo) * f(mid) > 0 else (lo, mid)
    row = (x.double() * lo).float()
    grad = (wd[j] - soft(row) @ wd) * (row != 0)                          # d log a_j / d x_c
    comp = int(grad.abs().argmax())
    step = np.float32(np.inf) if grad[comp] > 0 else np.float32(-np.inf)
    for _ in range(4096):
        v = float(soft(row)[j])
        if ok(v):
            return row
        up = (v - lam <= 0) if above else (lam - v > 3 * ulp)          # a_j has to grow
        row = row.clone()
        row[comp] = float(np.nextafter(np.float32(row[comp]), step if up else -step))
    raise AssertionError("no fp32 row within 3 ulps of the threshold")


# ------------------------------------------------------------------------------------------------ the reference and its bound
WRONG = ("hit_ge", "shrink_eps_dropped", "norm_unclamped", "last_item_lost", "tile_tail_lost", "block_tail_lost",
         "last_row_of_group_lost", "rows_clamped_counted", "split_tail_lost", "c_term_dropped", "q_dropped", "cy_dropped",
         "dense_dl_dropped", "stale_stats")


def reference(c, wrong=None):
    """-> dict of Q: y (R, 64), stats (R, 4), crow (R, 2), dx (R, 64), dW (n_items, 64); a (R, n_items) as Q, hit, count (|S| per
    row), undecided (bool per row).  wrong: one of WRONG — the same formulas with that mistake made."""
    assert wrong is None or wrong in WRONG
    R, N, lam = c.R, c.n_items, c.lam
    x, W, dy = c.x.double(), c.bank.double(), c.dy.double()
    dev = x.device
    strict = wrong is None and not bool(c.free.any())
    eps = 0.0 if wrong == "shrink_eps_dropped" else EPS32
    r = {}
    a, mx, Z = _softmax(c.x, c.bank)
    r["a"] = a
    r["undecided"] = ((a.v - lam).abs() <= a.e).any(1)
    hit = (a.v >= lam) if wrong == "hit_ge" else (a.v > lam)
    items = torch.arange(N, device=dev)
    rows = torch.arange(R, device=dev)
    if wrong == "last_item_lost":
        hit = hit & (items != N - 1)
    if wrong == "tile_tail_lost":
        hit = hit & (items < 16 * (N // 16))
    if wrong == "last_row_of_group_lost":
        hit = hit & (rows % ROWS_WG != ROWS_WG - 1)[:, None]
    cnt = hit.sum(1).double()
    live = cnt > 0
    r["hit"], r["count"] = hit, cnt
    # k_memtrain_fwd
    s = _shrink(a, lam, hit, eps, strict)
    n = _ksum(s, 1, cnt)
    kc = cnt[:, None]
    den = Q(torch.where(live, n.v, torch.full_like(n.v, EPS32)), n.e)
    if not strict:          # (an undecided or a wrong row may have n within its error of 0: its bound is not used)
        den = Q(den.v.clamp_min(EPS32), torch.minimum(den.e, 0.5 * den.v.clamp_min(EPS32)))
    y = _div(_kmm(s, W, kc), den[:, None]).rnd()
    if wrong == "norm_unclamped":
        y = Q(torch.where(live[:, None], y.v, torch.full_like(y.v, float("nan"))), y.e)
    zero = torch.zeros_like(n.v)
    r["y"] = y
    r["stats"] = Q(torch.stack([mx.v, Z.v, n.v, zero], 1), torch.stack([mx.e, Z.e, n.e, zero], 1))
    # k_memtrain_bwd_rows
    ab = a
    if wrong == "stale_stats":
        ab = Q(a.v * (Z.v / Z.v.roll(-1))[:, None], a.e)
    inv_n = _recip(den).rnd()[:, None]
    t = _mask((s * inv_n).rnd(), hit)
    Sdt = dy.abs() @ W.abs().t()
    dtv = dy @ W.t()
    dt_rows = Q(dtv, gamma(DT_K) * Sdt + DT_K * TINY * (Sdt > 0))
    dt_items = Q(dtv, gamma(LOGIT_K) * Sdt + KC * TINY * (Sdt > 0))
    q = _ksum(_mask(t * dt_rows, hit), 1, cnt)
    if wrong == "q_dropped":
        q = Q(torch.zeros_like(q.v))
    hg = _shrink_grad(ab, lam, hit, eps, strict)
    da = lambda dt: _mask((((dt - q[:, None]).rnd() * inv_n).rnd() * hg).rnd(), hit)
    ada = (ab * da(dt_rows)).rnd()
    cr = _ksum(ada, 1, cnt)
    r["crow"] = Q(torch.stack([cr.v, q.v], 1), torch.stack([cr.e, q.e], 1))
    dxs = _kmm(ada, W, kc)
    abar = _kmm(ab, W, abar_k(N))
    dx = dxs if wrong == "c_term_dropped" else (dxs - (cr[:, None] * abar).rnd()).rnd()
    r["dx"] = _mask(dx, live[:, None].expand_as(dx.v))
    # k_memtrain_bwd_items, k_memtrain_items_reduce
    on = (ab * (da(dt_items) - cr[:, None]).rnd()).rnd()
    off = (ab * cr[:, None]).rnd()
    off = Q(-off.v, off.e)
    if wrong == "dense_dl_dropped":
        off = Q(torch.zeros_like(off.v))
    cx = Q(torch.where(hit, on.v, off.v), torch.where(hit, on.e, off.e))
    cy = Q(torch.zeros_like(t.v)) if wrong == "cy_dropped" else t
    keep = ~c.free.to(dev)                     # a dy = 0 row adds exactly 0 whichever way it is decided
    if wrong == "split_tail_lost":
        for sp in range(SPLITS):
            tl = split_tiles(R, sp)
            if len(tl) >= 2:
                keep = keep & (rows // RT != tl[-1])
    cx, cy = _mask(cx, keep[:, None].expand_as(hit)), _mask(cy, keep[:, None].expand_as(hit))
    k = dw_k(R)
    Sw = cx.hi().t() @ x.abs() + cy.hi().t() @ dy.abs()
    dW = Q(cx.v.t() @ x + cy.v.t() @ dy, cx.e.t() @ x.abs() + cy.e.t() @ dy.abs() + gamma(k) * Sw + k * TINY * (Sw > 0))
    if wrong == "rows_clamped_counted":
        pad = row_tiles(R) * RT - R
        dW = Q(dW.v + pad * (cx.v[-1][:, None] * x[-1] + cy.v[-1][:, None] * dy[-1]), dW.e)
    if wrong == "block_tail_lost":
        dW = Q(dW.v * (items < IB * (N // IB))[:, None], dW.e)
    r["dW"] = dW
    return r


def autograd64(c):
    """y, dx, dW from torch autograd of memory_module.py:36-48 (torch_forms.hard_shrink_relu) in float64."""
    from torch_forms import hard_shrink_relu
    x, w = c.x.double().clone().requires_grad_(True), c.bank.double().clone().requires_grad_(True)
    att = torch.softmax(x @ w.t(), dim=1)
    y = F.normalize(hard_shrink_relu(att, c.lam, EPS32), p=1, dim=1) @ w
    dx, dw = torch.autograd.grad(y, (x, w), c.dy.double())
    return {"y": y.detach(), "dx": dx, "dW": dw}


# ------------------------------------------------------------------------------------------------ the fp32 stand-in
def _tree(x):
    """fp32 pairwise sum over the last dimension (a power of two): log2 roundings on every path, as a butterfly has."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def standin(c):
    """The kernels' formulas in fp32 torch.  In the kernels' structure: Z (32 serial additions a lane, then a tree), dt of bwd_rows (a
    tree over once-rounded products), a W by the waves' shares, dW by the splits' row tiles.  The sums over the support are dense fp32
    sums whose other terms are exact zeros: at most |S| of their additions round."""
    f32 = torch.float32
    R, N = c.R, c.n_items
    x, W, dy = c.x, c.bank, c.dy
    lam, eps = torch.tensor(c.lam, dtype=f32), torch.tensor(EPS32, dtype=f32)
    l = x @ W.t()
    mx = l.max(1)[0]
    v = torch.exp((l - mx[:, None]).clamp_min(-150.0))
    vp = F.pad(v, (0, ITEMS_MAX - N)).view(R, ITEMS_MAX // 64, 64)
    z = vp[:, 0].clone()
    for i in range(1, ITEMS_MAX // 64):
        z = z + vp[:, i]
    z = _tree(z)
    a = v * (1.0 / z)[:, None]
    hit = a > lam
    u = a - lam
    zero = torch.zeros((), dtype=f32)
    s = torch.where(hit, (u * a) / (u + eps), zero)
    n = s.sum(1)
    o = {"y": (s @ W) / n.clamp_min(eps)[:, None], "stats": torch.stack([mx, z, n, torch.zeros_like(n)], 1)}
    live = n > 0
    inv_n = (1.0 / n.clamp_min(eps))[:, None]
    t = s * inv_n
    idx = hit.nonzero()
    dt_rows = torch.zeros_like(a)
    dt_rows[idx[:, 0], idx[:, 1]] = _tree(dy[idx[:, 0]] * W[idx[:, 1]])
    q = (t * dt_rows).sum(1)
    d = u + eps
    hg = torch.where(hit, (u * u + eps * (a + u)) / (d * d), zero)
    ada = a * torch.where(hit, (dt_rows - q[:, None]) * inv_n * hg, zero)
    cr = ada.sum(1)
    o["crow"] = torch.stack([cr, q], 1)
    per = 4 * n4_per_wave(N)
    abar = torch.zeros(R, KC, dtype=f32)
    for w in range(WAVES):
        abar = abar + a[:, w * per:(w + 1) * per] @ W[w * per:(w + 1) * per]
    o["dx"] = torch.where(live[:, None], ada @ W - cr[:, None] * abar, zero)
    da_items = torch.where(hit, (dy @ W.t() - q[:, None]) * inv_n * hg, zero)
    cx = torch.where(hit, a * (da_items - cr[:, None]), -a * cr[:, None])
    dW = torch.zeros(N, KC, dtype=f32)
    for sp in range(SPLITS):
        tl = split_tiles(R, sp)
        lo, hi = tl.start * RT, min(tl.stop * RT, R)
        if hi > lo:
            dW = dW + (cx[lo:hi].t() @ x[lo:hi] + t[lo:hi].t() @ dy[lo:hi])
    o["dW"] = dW
    return o


OUTPUTS = ("y", "stats", "crow", "dx", "dW")


def fractions(got, r, free=None):
    """name -> max err / bound per output.  On the `free` rows (near_threshold) y, dx and n are left out; the caller requires them
    finite."""
    fr = {}
    for k in OUTPUTS:
        skip = None
        if free is not None and bool(free.any()) and k != "dW":
            skip = free[:, None].expand_as(r[k].v).clone()
            if k == "stats":
                skip[:, :2] = False
            if k == "crow":
                skip[:] = False
        fr[k] = used_fraction(got[k].reshape(r[k].v.shape), r[k], skip)
    return fr


def undecided_share(c, r):
    """Share of the rows, the stated free ones apart, with an item whose decision the reference cannot take."""
    und = r["undecided"] & ~c.free.to(r["undecided"].device)
    return float(und.double().mean()) if c.R else 0.0


# ------------------------------------------------------------------------------------------------ the table
# name -> Case keywords; what the row is there for.  n_items = 2000, lam = 0.0025 unless given.
ROWS = {
    # row edges: one row; a ragged, a full, a full + 1 group of 16; the same around a 64-row tile of the bank gradient
    **{f"R{R}": dict(R=R) for R in (1, 15, 16, 17, 63, 64, 65)},
    "R2048": dict(R=2048),                                                  # 32 row tiles: one to each of the 32 splits
    "R2049": dict(R=2049),                                                  # 33 tiles: two a split, the 17th split takes one, the rest none
    # bank edges: ragged 16-item tiles, 64-item slices, 128-item blocks, n4 shares; 1 / n_items > lam: every item in the support
    **{f"n{n}": dict(R=40, n_items=n, scale=0.25 if n < 400 else 8.0) for n in
       (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048)},
    "planted_borders": dict(R=40, n_items=1999, content="planted", scale=1.0),      # a dominant item on each side of every border
    "empty_all": dict(R=40, content="empty_all"),                           # no support anywhere: the early return of bwd_rows
    "mixed_groups": dict(R=200, content="mixed_groups"),                    # empty and live rows inside a group; whole groups, a whole tile empty
    "one_item": dict(R=40, content="one_item"),                             # a ~ 1, the -150 clamp, underflowing exponentials
    "full_support_ties": dict(R=40, n_items=37, content="ties", scale=2.0),         # x = 0 rows: all a exactly equal
    "wide_support": dict(R=33, n_items=2048, lam=1e-4, scale=6.0),          # supports of hundreds of items
    "lambda_high": dict(R=40, lam=0.3, scale=16.0),                         # supports of at most 3
    "negative_x": dict(R=40, relu=False, scale=6.0),                        # features that are not post-ReLU
    "dy_zero": dict(R=40, dy_zero=True),                                    # every gradient exactly 0
    "near_threshold": dict(R=40, content="near"),                           # N_FREE rows within 3 ulps of lam, dy = 0 there
    # Not in the issue's list.  c = sum_S a da cancels to a^2 eps / (u + eps)^2 terms (sum_S t (dt - q) = 0 and s ~ a, hs' ~ 1 away
    # from lam): in every row above it is rounding noise, and the dense half of the backward (c (a W) in dx, -a c in dW) carries no
    # signal.  Here the features are tiny, a = (1 + 4e-4 N(0, 1)) / 8 straddles lam = 1 / 8 and delta a ~ 1e-7; the items are kept 40 delta a
    # from lam (the bound of hs' is (2 delta a / u) (hs' - 1): nearer items would bury c in it), so the support's items lie 5e-6 .. 1e-4
    # above lam, hs' - 1 = lam eps / (u + eps)^2 is 1e-5 .. 5e-3 and c is a number the bound can see
    "live_c": dict(R=40, n_items=8, lam=1.0 / 8, scale=1e-3, near_by=40.0),
}
EXACT = {"empty_all": ("y", "crow", "dx", "dW"), "dy_zero": ("crow", "dx", "dW")}

# wrong variant -> (Case keywords of the inputs built for it, the outputs on which the touched elements must be outside the bound)
_P = dict(R=40, n_items=1999, content="planted", scale=1.0)
_C = dict(R=40, n_items=8, lam=1.0 / 8, scale=1e-3, near_by=40.0)
_F = dict(R=40, n_items=130, scale=2.0)                                   # 1 / 130 > lam: every item in every support
                   # the row live_c
WRONG_CASES = {
    # x = 0 rows with a = lam exactly: s = 0 either way and y stays 0, but hs'(lam) = lam / eps sends da, c and dx to 1e20
    "hit_ge": (dict(R=40, n_items=32, lam=1.0 / 32, content="ties", scale=2.0, allow_undecided=True), ("crow", "dx")),
    "shrink_eps_dropped": (_C, ("crow", "dx", "dW")),
    "norm_unclamped": (dict(R=200, content="mixed_groups"), ("y",)),
    "last_item_lost": (_P, ("y", "dx")),
    "tile_tail_lost": (_P, ("y", "dx")),
    "block_tail_lost": (_F, ("dW",)),
    "last_row_of_group_lost": (dict(R=40), ("y", "dx")),
    "rows_clamped_counted": (_F, ("dW",)),
    "split_tail_lost": (dict(R=2049, n_items=130, scale=4.0), ("dW",)),
    "c_term_dropped": (_C, ("dx",)),
    "q_dropped": (dict(R=40), ("crow", "dx")),
    "cy_dropped": (dict(R=40), ("dW",)),
    "dense_dl_dropped": (_C, ("dW",)),
    "stale_stats": (_F, ("dx", "dW")),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The row's inputs (shared: nobody writes to them; .to() copies)."""
    return Case(**ROWS[name], name=name)


@functools.lru_cache(maxsize=None)
def wrong_case(wrong):
    return Case(**WRONG_CASES[wrong][0], name=f"wrong_{wrong}")


OBSERVED = """max err / bound on the MI355X over the thirty-nine rows, per output (the row that sets it; the largest of the other rows):
y 0.0658 (live_c; 0.0258 full_support_ties), stats 0.1149 (live_c; 0.0526 full_support_ties), crow 0.0480 (n1), dx 0.0631 (live_c;
0.0144 full_support_ties), dW 0.0133 (live_c; 0.0069 R64).  The rows at n_items = 2000 use 0.002 to 0.009 of the bound of y and
0.01 to 0.03 of that of stats: the bound is gamma(128) sum |x| |w| on every logit, the worst case of 128 roundings of one sign, and
the fp32 stand-in of the host test uses the same share (R1: stats 0.0092 on the CPU and on the MI355X).  Both assumptions are consistent
with this: in live_c (n_items = 8, z_k = 7, tiny logits) the 2 ulp assumed of the exponential are a third of the bound of Z (11 u of Z)
and a sixth of that of n (24 u of n), and stats uses 0.115 there, under 3 u in all: an exponential several ulp off would show
there first.  Nothing suggests that the fp32 MFMA sums round worse than a product and an accumulate per K slot.
The exact rows are exactly 0; the eight near_threshold rows are finite with crow exactly 0; nothing else is left out.
Rows drawn again (rows / R, the most draws of one row): R16 1/16 (1), R17 2/17 (1), R63 1/63 (1), R64 3/64 (1), R65 3/65 (1),
R2048 126/2048 (2), R2049 132/2049 (2), n2047 4/40 (1), n2048 2/40 (1), mixed_groups 4/200 (1), wide_support 9/33 (2),
negative_x 1/40 (1), dy_zero 3/40 (1), near_threshold 3/40 (1), live_c 16/40 (7); no other row needed one."""
