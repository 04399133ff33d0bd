"""Float64 reference, the per-element rounding bound and the case tables of the eval-mode two-stream pillar encoder (csrc/vfe.hip:
vfe_pass, run by k_vfe_rows behind hvpr_pillar_vfe_fwd_f32 and by k_vfe_gather behind hvpr_encode_fwd_f32), shared by
test_vfe_eval_host.py (the kernel's formulas in fp32 torch stand in for the kernel: the bound proves itself, the algebra is checked
against the oracle and fixture G1, and the reference with one mistake made falls outside the bound) and test_gpu_vfe_eval.py (both
kernels against the same bound).  Plain torch / numpy, no GPU.  Q, qsum, gamma, used_fraction, caught_share and the constants come
from bn_train_cases.py / conv_direct_cases.py.

The reference takes exactly the fp32 words the entry point is handed (voxels, the FOLDED weights — folded in fp32 first, widened
afterwards —, voxel size and offsets as fp32 words), widened to float64:
    mean = (sum of xyz over the n live slots) / n;  f = [x y z r | xyz - mean | xyz - (cell * vs + off)] times (slot < n);
    y0 = relu(W0 f + b0) per slot;  x_max = max over ALL P slots — a padded slot (n < P) has f = 0 and gives relu(b0);
    out = max over ALL P slots of relu(W1 [y0 | x_max] + b1) — the padded slot's column is W1 [relu(b0) | x_max] + b1;
    scale = relu(Ws1 relu(Ws0 [n, |mean|, mean] + bs0) + bs1);  mask = (slot < n), exact.

The bound.  Every value is followed as Q = (float64 value, error bound) operation by operation from vfe.hip, as in
bn_train_cases.py.  vfe.hip is built WITHOUT -ffp-contract=off: wherever a * b + c could be fused the unfused form is bounded, whose
bound holds for the fused one (one rounding fewer).  The divisions and sqrtf are correctly rounded (the library is built with
-fno-fast-math, as gate_train_cases.py states for its divisions).  The k of every sum (roundings on the path of a partial sum):

  * pillar sums: NO fp32 rounding of the additions.  to_grid takes every coordinate to an integer multiple of 2^-k metres by
    truncation (error below 2^-k per term), k = sum_scale(|centre| + vs) = 47 - e with 2^(e-1) <= |centre| + vs < 2^e (grid_k below:
    k = 41 for 32 m <= bound < 64 m, 42 for 16 .. 32 m: the far corner of the 102.4 m grid and the KITTI grid differ), and the up to 32
    integer-valued doubles add exactly in any order (asserted: P * max |v| * 2^k <= 2^53).  So |S^ - S| <= n 2^-k, then ONE rounding
    to float and ONE for the division by float(n).  The kernel's own centre may differ from the float64 one in the last bit, so the
    bound takes the k of the bound inflated by 4 u (never larger than the kernel's).
  * centre: fl(fl(cell * vs) + off); cluster and centre features: one subtraction each.
  * every v_mfma_f32_32x32x2_f32 step is charged a rounding for each of its two products and one for its accumulate, as
    conv_direct_cases.py does: a sum of K products on the matrix core has k = 2 K.  Layer 0: K = 10, k = 20, then the bias add.
    Layer 1 is TWO sums of 16 products, accumulated separately — W1a y0 per point and W1b x_max per pillar, k = 32 each —, added
    afterwards (one rounding), then the bias (one rounding).  The padded slot's column W1a relu(b0) runs on the matrix core too
    (k = 32 on an exact input).  Scale stream: K = 6 (the sixth input is a zero), k = 12, bias; K = 16, k = 32, bias.
  * |mean| = sqrtf(fl(fl(fl(mx mx) + fl(my my)) + fl(mz mz))): five roundings and the interval of the square root, one rounding.
  * ReLU and max are 1-Lipschitz: |max a_i - max b_i| <= max |a_i - b_i|.  No decision is undecided; NO element is excluded or masked.

Nothing here is fitted to what a kernel returns.

What the wrong variants are: see WRONG.  mask_on_output_not_input moves the mask from the input of layer 0 to its output: a
padded slot then has y0 = 0 instead of relu(b0) — it no longer raises x_max, and its layer-1 column is W1 [0 | x_max] + b1.

The packed form.  k_vfe_gather walks the voxelizer's arena: the points grouped by voxel, the voxels in rank order (the order of
their first points), every point of a voxel present (those past max_points too), so a frame's arena is the sequence of its voxels'
point counts.  pass_plan restates which pillars a pass of 32 columns takes; SEQUENCES names the edge each sequence hits and
clouds() builds the points.

Observed on the MI355X: see OBSERVED at the end of this file."""
import numpy as np
import torch

from bn_train_cases import Q, TINY, caught_share, qsum, used_fraction  # noqa: F401  (re-exported to the tests)
from conv_direct_cases import SENTINEL, U, gamma  # noqa: F401

C0, CIN, C1, CS0, CS1 = 16, 10, 64, 16, 32
K_WIN, K_PASS = 28, 32                              # arena positions a wave owns / columns of a pass (vfe.hip kWin)
ROWS_WAVES = 2048 * 4                               # waves of the largest k_vfe_rows grid
K_MFMA = lambda K: 2 * K
GRIDS = {"kitti": dict(vs=(0.16, 0.16, 3.0), lo=(0.0, -19.84, -2.5), nx=296, ny=248),
         "dense": dict(vs=(0.2, 0.2, 8.0), lo=(-51.2, -51.2, -5.0), nx=512, ny=512)}
WEIGHTS = ("w0", "b0", "w1", "b1", "ws0", "bs0", "ws1", "bs1")


def f32_words(values):
    """The float32 words a list of Python floats becomes at the C boundary."""
    return torch.tensor([float(v) for v in values], dtype=torch.float32)


def offsets_of(grid):
    g = GRIDS[grid] if isinstance(grid, str) else grid
    return [float(g["vs"][i]) / 2 + float(g["lo"][i]) for i in range(3)]


def grid_k(bound):
    """sum_scale of vfe.hip restated: 2^k grid units per metre for a pillar whose coordinates are below `bound` (float64 tensor of
    fp32 values): bound = m 2^e with 1/2 <= m < 1, k = 47 - e."""
    return 47 - torch.frexp(bound.float())[1].to(torch.int64)


# ------------------------------------------------------------------------------------------------ one case
def _seed(*row):
    return int(sum((int(v) + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


def weights(seed, floor=False):
    """Folded layers by seed.  floor: b0 = 2 in channels 0 .. 5, whose weights are -0.5 on x and a tenth of the others' elsewhere: every
    live point a few metres out has y0 = 0 there, below relu(b0)."""
    g = torch.Generator().manual_seed(_seed(seed, 77))
    w = {"w0": torch.randn(C0, CIN, generator=g) * 0.3, "b0": torch.randn(C0, generator=g) * 0.3,
         "w1": torch.randn(C1, 2 * C0, generator=g) * 0.2, "b1": torch.randn(C1, generator=g) * 0.3,
         "ws0": torch.randn(CS0, 5, generator=g) * 0.3, "bs0": torch.randn(CS0, generator=g) * 0.3,
         "ws1": torch.randn(CS1, CS0, generator=g) * 0.2, "bs1": torch.randn(CS1, generator=g) * 0.3}
    if floor:
        w["w0"][:6, 1:] *= 0.1
        w["w0"][:6, 0] = -0.5
        w["b0"][:6] = 2.0
    return {k: v.contiguous() for k, v in w.items()}


class Case:
    """Inputs of one row: voxels (M, P, 4) zero padded, num (M,), coords (M, 4) [b, z, y, x], the folded weights, voxel size and
    offsets as fp32 words.  counts: a list (repeated to M) | mixed | full | one.  content:
      corners     cells (0, 0) and (nx - 1, ny - 1) in turn          far        every pillar in the cell (nx - 1, ny - 1)
      zero        cell (0, 124): the first point has x = 0, y = 0, z = 0 exactly
      tiny_z      |z| below 2^-20 in every point                     negative   cells of the dense grid's x < 0, y < 0, z < 0
      identical   every slot of a pillar holds the same point        borders    points at the cell's own lower / last-below-upper borders
      near        cells with x >= 100: points 16 m out and more (the floor rows)
    pool: the pillars are drawn from that many templates in a seeded random order.  m_device: the live row count handed over."""

    def __init__(self, M, P, counts="mixed", grid="kitti", content=None, pool=None, floor=False, m_device=None, seed=0, name=None):
        g = torch.Generator().manual_seed(_seed(M, P, seed))
        G = GRIDS[grid]
        self.M, self.P, self.grid, self.content, self.m_device = M, P, grid, content, m_device
        self.name = name or f"M{M}_P{P}"
        T = pool or M
        mixed, short = torch.randint(1, P + 1, (T,), generator=g), torch.randint(1, max(P // 4, 2), (T,), generator=g)
        if counts == "full":
            num = torch.full((T,), P)
        elif counts == "one":
            num = torch.ones(T, dtype=torch.long)
        elif counts == "mixed":
            num = mixed
        elif counts == "short":                          # every pillar has padded slots
            num = short
        else:
            num = torch.tensor([counts[i % len(counts)] for i in range(T)])
        nx, ny = G["nx"], G["ny"]
        cx, cy = torch.randint(0, nx, (T,), generator=g), torch.randint(0, ny, (T,), generator=g)
        odd = torch.arange(T) % 2 == 1
        if content == "corners":
            cx, cy = torch.where(odd, nx - 1, 0), torch.where(odd, ny - 1, 0)
        elif content == "far":
            cx, cy = torch.full((T,), nx - 1), torch.full((T,), ny - 1)
        elif content == "zero":
            cx, cy = torch.zeros(T, dtype=torch.long), torch.full((T,), 124)
        elif content == "negative":
            cx, cy = cx % (nx // 2), cy % (ny // 2)
        elif content == "near":
            cx = 100 + cx % (nx - 100)
        vs, lo = torch.tensor(G["vs"], dtype=torch.float64), torch.tensor(G["lo"], dtype=torch.float64)
        cell = torch.stack([cx, cy, torch.zeros_like(cx)], 1).double()
        u = torch.rand(T, P, 4, generator=g).double()
        u[..., :3] = 0.1 + 0.8 * u[..., :3]              # well inside the cell
        xyz = lo + (cell[:, None] + u[..., :3]) * vs
        if content == "negative":
            xyz[..., 2] = lo[2] + u[..., 2] * (0.0 - lo[2]) * 0.99
        if content == "tiny_z":
            xyz[..., 2] = (u[..., 2] - 0.5) * 2.0 ** -21
        vox = torch.cat([xyz, u[..., 3:]], -1).float()
        if content == "borders":
            lo_b = (lo + cell * vs).float()                                            # the fp32 lower border of the cell
            hi_b = torch.nextafter((lo + (cell + 1.0) * vs).float(), torch.tensor(-1e30))
            pick = (torch.arange(P)[None, :, None] + torch.arange(3)[None, None, :]) % 2 == 0
            vox[..., :3] = torch.where(pick, lo_b[:, None], hi_b[:, None])
        if content == "zero":
            vox[:, 0, :3] = 0.0
        if content == "identical":
            vox = vox[:, :1].expand(T, P, 4).clone()
        vox = vox * (torch.arange(P).view(1, -1, 1) < num.view(-1, 1, 1))
        coords = torch.stack([torch.zeros_like(cx), torch.zeros_like(cx), cy, cx], 1)
        if pool:
            pick = torch.randint(0, pool, (M,), generator=g)
            vox, coords, num = vox[pick], coords[pick], num[pick]
            self.template = pick
        self.voxels, self.num, self.coords = vox.contiguous(), num.int().contiguous(), coords.int().contiguous()
        self.vs, self.off = f32_words(G["vs"]), f32_words(offsets_of(grid))
        for k, v in weights(seed, floor).items():
            setattr(self, k, v)

    def folded(self):
        return {k: getattr(self, k) for k in WEIGHTS}

    def to(self, device):
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self


class Raw:
    """The same fields from arrays a test already has (a fixture, a kernel's returned voxels)."""

    def __init__(self, voxels, num, coords, folded, vs, off, name="raw"):
        self.voxels, self.num, self.coords = voxels.float(), num.int(), coords.int()
        self.M, self.P, self.name = voxels.shape[0], voxels.shape[1], name
        dev = voxels.device
        self.vs, self.off = f32_words(vs).to(dev), f32_words(off).to(dev)
        for k in WEIGHTS:
            setattr(self, k, folded[k].float().to(dev))


# ------------------------------------------------------------------------------------------------ the reference and its bound
WRONG = ("floor_dropped", "floor_on_full_pillars", "mean_over_P", "centre_xz_swapped", "xmax_of_previous_pillar",
         "mask_on_output_not_input", "scale_norm_squared", "scale_n_is_P", "layer1_halves_swapped")


def _lin(x, w, k):
    """x (.., n) Q times the exact weight rows w (c, n) as a sum of n products with k roundings on a path -> (.., c)."""
    wa = w.abs().t()
    S = x.hi() @ wa
    return Q(x.v @ w.t(), x.e @ wa + gamma(k) * S + k * TINY * (S > 0))


def _cat(qs, dim=-1):
    return Q(torch.cat([q.v for q in qs], dim), torch.cat([q.e for q in qs], dim))


def _qmax(q, dim, take):
    """max over `dim` of the entries where take (at least one each): 1-Lipschitz, so the error is the largest of theirs."""
    ninf = torch.full_like(q.v, float("-inf"))
    return Q(torch.where(take, q.v, ninf).max(dim)[0], torch.where(take, q.e, torch.zeros_like(q.e)).max(dim)[0])


def _join(a, b, where):
    """max(a, b) where `where`, else a."""
    return Q(torch.where(where, torch.maximum(a.v, b.v), a.v), torch.where(where, torch.maximum(a.e, b.e), a.e))


def _sqrt(q):
    hi, lo = (q.v + q.e).sqrt(), (q.v - q.e).clamp_min(0.0).sqrt()
    v = q.v.clamp_min(0.0).sqrt()
    return Q(v, torch.maximum(hi - v, v - lo))


def reference(c, wrong=None, rows=1024):
    """-> dict: pillar (M, 64), scale (M, 32) as Q; mask (M, P) float64; x_max (M, 16) Q; pad_wins_xmax (M, 16), pad_wins_out (M, 64):
    the padded slot's value exceeds every live slot's by more than both bounds (and, for out, passes the ReLU by more than its bound).
    wrong: one of WRONG — the same formulas with that mistake made.  More than `rows` pillars are taken in pieces."""
    assert wrong is None or wrong in WRONG
    if c.M > rows:
        assert wrong != "xmax_of_previous_pillar"
        parts = []
        for i in range(0, c.M, rows):
            parts.append(reference(Raw(c.voxels[i:i + rows], c.num[i:i + rows], c.coords[i:i + rows], {k: getattr(c, k) for k in WEIGHTS},
                                       c.vs.tolist(), c.off.tolist()), wrong, rows))
        out = {}
        for k, v in parts[0].items():
            out[k] = _cat([p[k] for p in parts], 0) if isinstance(v, Q) else torch.cat([p[k] for p in parts], 0)
        return out
    M, P = c.M, c.P
    dev = c.voxels.device
    f64 = torch.float64
    n = c.num.to(f64)
    assert bool((c.num >= 1).all()) and bool((c.num <= P).all()), "a row of no points divides by zero in the reference"
    live = torch.arange(P, device=dev)[None, :] < c.num[:, None]                            # (M, P)
    lv = live.to(f64)[..., None]
    vs, off = c.vs.to(f64), c.off.to(f64)
    centre = (Q(c.coords[:, [3, 2, 1]].to(f64) * vs).rnd() + Q(off.expand(M, 3))).rnd()
    # pillar sums on the fixed-point grid
    xyz = c.voxels[:, :, :3].to(f64) * lv
    bnd = centre.v.abs() + vs
    if wrong == "centre_xz_swapped":                                                        # (the features' centre only)
        centre = (Q(c.coords[:, [1, 2, 3]].to(f64) * vs).rnd() + Q(off.expand(M, 3))).rnd()
    k_lo, k_hi = grid_k(bnd * (1.0 + 4.0 * U)), grid_k(bnd * (1.0 - 4.0 * U))
    assert bool((P * xyz.abs().amax(1) * torch.exp2(k_hi.to(f64)) <= 2.0 ** 53).all()), "the grid sums would not be exact"
    s = Q(xyz.sum(1), n[:, None] * torch.exp2(-k_lo.to(f64))).rnd()
    div = torch.full_like(n, float(P)) if wrong == "mean_over_P" else n
    mean = Q(s.v / div[:, None], s.e / div[:, None]).rnd()
    raw = Q(c.voxels.to(f64) * lv)
    X = Q(xyz)
    dm, dc = (X - mean[:, None]).rnd(), (X - centre[:, None]).rnd()
    x0 = _cat([raw, Q(dm.v * lv, dm.e * lv), Q(dc.v * lv, dc.e * lv)])                      # (M, P, 10)
    w0, b0, w1, b1 = c.w0.to(f64), c.b0.to(f64), c.w1.to(f64), c.b1.to(f64)
    w1a, w1b = w1[:, :C0], w1[:, C0:]
    if wrong == "layer1_halves_swapped":
        w1a, w1b = w1b, w1a
    # layer 0, x_max with the padded slot's floor
    y0 = (_lin(x0, w0, K_MFMA(CIN)) + Q(b0)).rnd().relu()                                   # (M, P, 16); padded slots are replaced below
    z0 = Q(torch.relu(b0))                                                                  # fmaxf(0.f + b0, 0.f): exact
    z0_l1 = Q(torch.zeros_like(b0)) if wrong == "mask_on_output_not_input" else z0
    pad = c.num < P
    if wrong == "floor_on_full_pillars":
        pad = torch.ones_like(pad)
    pad_x = torch.zeros_like(pad) if wrong in ("floor_dropped", "mask_on_output_not_input") else pad
    pad_1 = torch.zeros_like(pad) if wrong == "floor_dropped" else pad
    xm_live = _qmax(y0, 1, live[..., None].expand_as(y0.v))
    zq = Q(z0.v.expand(M, C0), torch.zeros(M, C0, dtype=f64, device=dev))
    xm = _join(xm_live, zq, pad_x[:, None].expand(M, C0))
    # layer 1: two separately accumulated halves, their sum, the max over the slots, the bias
    d1 = _lin(y0, w1a, K_MFMA(C0))                                                          # (M, P, 64)
    cc = _lin(xm, w1b, K_MFMA(C0))                                                          # (M, 64)
    if wrong == "xmax_of_previous_pillar" and M > 1:
        cc = Q(torch.cat([cc.v[:1], cc.v[:-1]]), torch.cat([cc.e[:1], cc.e[:-1]]))
    t = (d1 + cc[:, None]).rnd()
    z1 = _lin(z0_l1, w1a, K_MFMA(C0))                                                       # (64,)
    tp = (Q(z1.v.expand(M, C1), z1.e.expand(M, C1)) + cc).rnd()
    m_live = _qmax(t, 1, live[..., None].expand_as(t.v))
    m = _join(m_live, tp, pad_1[:, None].expand(M, C1))
    pre = (m + Q(b1)).rnd()
    r = {"pillar": pre.relu(), "mask": live.to(f64), "x_max": xm}
    r["pad_wins_xmax"] = pad_x[:, None] & (z0.v > xm_live.v + xm_live.e)
    r["pad_wins_out"] = pad_1[:, None] & (tp.v - tp.e > m_live.v + m_live.e) & (pre.v > pre.e)
    # scale stream
    mx, my, mz = mean[:, 0], mean[:, 1], mean[:, 2]
    sq = (((mx * mx).rnd() + (my * my).rnd()).rnd() + (mz * mz).rnd()).rnd()
    nrm = sq if wrong == "scale_norm_squared" else _sqrt(sq).rnd()
    fn = Q(torch.full_like(n, float(P)) if wrong == "scale_n_is_P" else n)
    s_in = Q(torch.stack([fn.v, nrm.v, mx.v, my.v, mz.v], 1), torch.stack([fn.e, nrm.e, mx.e, my.e, mz.e], 1))
    hid = (_lin(s_in, c.ws0.to(f64), K_MFMA(6)) + Q(c.bs0.to(f64))).rnd().relu()
    r["scale"] = (_lin(hid, c.ws1.to(f64), K_MFMA(CS0)) + Q(c.bs1.to(f64))).rnd().relu()
    return r


def standin(c):
    """The kernel's formulas in fp32 torch, one rounding per operation (the pillar sums exact, as the kernel's are) -> pillar, scale,
    mask (fp32)."""
    M, P = c.M, c.P
    live = torch.arange(P)[None, :] < c.num[:, None]
    lv = live.float()[..., None]
    n = c.num.float()
    xyz = c.voxels[:, :, :3] * lv
    mean = xyz.double().sum(1).float() / n[:, None]
    centre = c.coords[:, [3, 2, 1]].float() * c.vs + c.off
    x0 = torch.cat([c.voxels * lv, (xyz - mean[:, None]) * lv, (xyz - centre[:, None]) * lv], -1)
    y0 = torch.relu(x0 @ c.w0.t() + c.b0)
    z0 = torch.relu(c.b0)
    pad = (c.num < P)[:, None]
    xm = torch.where(live[..., None], y0, torch.zeros_like(y0)).max(1)[0]
    xm = torch.where(pad, torch.maximum(xm, z0), xm)
    w1a, w1b = c.w1[:, :C0].contiguous(), c.w1[:, C0:].contiguous()
    cc = xm @ w1b.t()
    t = y0 @ w1a.t() + cc[:, None]
    m = torch.where(live[..., None], t, torch.full_like(t, float("-inf"))).max(1)[0]
    m = torch.where(pad, torch.maximum(m, (z0 @ w1a.t())[None] + cc), m)
    pillar = torch.relu(m + c.b1)
    nrm = torch.sqrt(mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1] + mean[:, 2] * mean[:, 2])
    s_in = torch.stack([n, nrm, mean[:, 0], mean[:, 1], mean[:, 2]], 1)
    scale = torch.relu(torch.relu(s_in @ c.ws0.t() + c.bs0) @ c.ws1.t() + c.bs1)
    assert pillar.dtype == torch.float32 and scale.dtype == torch.float32
    return pillar, scale, live.float()


OUTPUTS = ("pillar", "scale")


def fractions(pillar, scale, r, rows=None):
    """max err / bound per output over every element (of the first `rows` pillars)."""
    sl = slice(None) if rows is None else slice(0, rows)
    return {"pillar": used_fraction(pillar[sl], r["pillar"][sl]), "scale": used_fraction(scale[sl], r["scale"][sl])}


def sharpness(r):
    """bound / largest element per output."""
    return {k: float(r[k].e.max() / r[k].v.abs().max().clamp_min(TINY)) for k in OUTPUTS}


# ------------------------------------------------------------------------------------------------ the table of the rows form
# name -> Case keywords, and what the row is there for
ROWS = {
    "one_point_P32": dict(M=1, P=32, counts="one"),                              # one live column, 31 padded slots
    "full_P32": dict(M=1, P=32, counts="full"),                                  # no padded slot: the scan crosses the 16-lane row border
    "one_beside_full": dict(M=2, P=32, counts=[1, 32]),
    "single_slot": dict(M=3, P=1, counts="full"),                                # n = P = 1: no padded slot at all
    "P5": dict(M=9, P=5, counts="mixed"),
    "P20": dict(M=9, P=20, counts="mixed"),                                      # the pillar ends inside the second 16-lane row
    "P31": dict(M=9, P=31, counts="mixed"),
    "second_workgroup": dict(M=5, P=32, counts="mixed"),                         # a second workgroup with one live wave
    "grid_stride": dict(M=8195, P=32, counts="mixed", pool=64),                  # three waves take a second pillar past the 2048-workgroup grid
    "floor_decides": dict(M=9, P=32, counts="short", content="near", floor=True),
    "floor_must_not_apply": dict(M=9, P=32, counts="full", content="near", floor=True),
    "kitti_corners": dict(M=6, P=32, counts="mixed", content="corners"),         # cells (0, 0) and (295, 247)
    "dense_far_corner": dict(M=6, P=20, counts="mixed", grid="dense", content="far"),        # (511, 511): k = 41 where KITTI's x has 42
    "zero_coordinate": dict(M=4, P=32, counts="mixed", content="zero"),
    "tiny_z": dict(M=6, P=32, counts="mixed", content="tiny_z"),
    "all_negative": dict(M=9, P=20, counts="mixed", grid="dense", content="negative"),
    "identical_points": dict(M=4, P=32, counts="full", content="identical"),
    "cell_borders": dict(M=6, P=32, counts="mixed", content="borders"),
    "m_device_below_M": dict(M=9, P=32, counts="mixed", m_device=5),             # rows at or past m_device keep the sentinel
}

# wrong variant -> (row, the outputs on which every touched element must be outside the bound)
WRONG_CASES = {
    "floor_dropped": ("floor_decides", ("pillar",)),
    "floor_on_full_pillars": ("floor_must_not_apply", ("pillar",)),
    "mean_over_P": ("P20", ("pillar", "scale")),
    "centre_xz_swapped": ("P20", ("pillar",)),
    "xmax_of_previous_pillar": ("P20", ("pillar",)),
    "mask_on_output_not_input": ("floor_decides", ("pillar",)),
    "scale_norm_squared": ("P20", ("scale",)),
    "scale_n_is_P": ("P20", ("scale",)),
    "layer1_halves_swapped": ("P20", ("pillar",)),
}


def case(name, **over):
    return Case(**{**ROWS[name], **over}, name=name)


# ------------------------------------------------------------------------------------------------ the packed form
def pass_plan(counts, P):
    """The passes k_vfe_gather takes over an arena whose voxels hold `counts` points, in order -> [(window, [pillars of the pass])].
    A wave owns the pillars that START inside its window of K_WIN arena positions.  A pass begins at the first owned pillar not
    yet taken, at arena position s, and spans the K_PASS positions from s; it takes every owned pillar with count <= P that starts
    in the span and ends inside it (start - s + count <= K_PASS).  A pillar with count > P gets a pass of its own."""
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int) if len(counts) else np.zeros(0, int)
    plan = []
    for w in range(-(-int(np.sum(counts)) // K_WIN) if len(counts) else 0):
        todo = [j for j in range(len(counts)) if w * K_WIN <= starts[j] < (w + 1) * K_WIN]
        while todo:
            j0 = todo[0]
            if counts[j0] > P:
                take = [j0]
            else:
                s = starts[j0]
                take = [j for j in todo if counts[j] <= P and starts[j] - s + counts[j] <= K_PASS]
            plan.append((w, take))
            todo = [j for j in todo if j not in take]
    return plan


# name -> frames (a list of count sequences, one per frame), P, and the passes the whole arena must make (pillars numbered through
# the frames): the edge the sequence is there for
SEQUENCES = {
    "ones_64": dict(frames=[[1] * 64], P=32),                     # 28 pillars a pass: the window, not the 32 columns, ends the pass; three windows
    "halves": dict(frames=[[16, 16] * 3], P=32),                  # every pillar ends on a 16-lane row border; two fill a pass exactly
    "15_17": dict(frames=[[15, 17]], P=32),                       # the second pillar straddles the row border and ends on column 31
    "17_15": dict(frames=[[17, 15]], P=32),
    "31_1": dict(frames=[[31, 1]], P=32),                         # the one-point pillar starts at position 31, past window 0: the next wave's, whose window begins at 28
    "1_31": dict(frames=[[1, 31]], P=32),
    "full": dict(frames=[[32]], P=32),                            # no padded slot: hz false, the scan's carry across the row border
    "full_full": dict(frames=[[32, 32]], P=32),                   # the second starts outside window 0: another wave's
    "20_20": dict(frames=[[20, 20]], P=32),                       # the second pillar does not fit: a second pass of the same window
    "ones_27_full": dict(frames=[[1] * 27 + [32]], P=32),         # a full pillar starting on the last owned window position
    "33_of_32": dict(frames=[[33]], P=32),                        # more points than slots: the pass of its own, radix select
    "21_3_of_20": dict(frames=[[21, 3]], P=20),
    "6_5_5_of_5": dict(frames=[[6, 5, 5]], P=5),
    "fives_13": dict(frames=[[5] * 13], P=5),                     # six full pillars a pass, no padded slot anywhere
    "15_17_two_frames": dict(frames=[[15], [17]], P=32),          # one pass holds pillars of two frames
    "ones_two_frames": dict(frames=[[1] * 20, [1] * 44], P=32),   # the frame border inside a pass
}
PLANS = {
    "ones_64": [(0, list(range(28))), (1, list(range(28, 56))), (2, list(range(56, 64)))],
    "halves": [(0, [0, 1]), (1, [2, 3]), (2, [4, 5])],
    "15_17": [(0, [0, 1])], "17_15": [(0, [0, 1])], "31_1": [(0, [0]), (1, [1])], "1_31": [(0, [0, 1])],
    "full": [(0, [0])], "full_full": [(0, [0]), (1, [1])],
    "20_20": [(0, [0]), (0, [1])],
    "ones_27_full": [(0, list(range(27))), (0, [27])],
    "33_of_32": [(0, [0])], "21_3_of_20": [(0, [0]), (0, [1])], "6_5_5_of_5": [(0, [0]), (0, [1, 2])],
    "fives_13": [(0, [0, 1, 2, 3, 4, 5]), (1, [6, 7, 8, 9, 10, 11]), (2, [12])],
    "15_17_two_frames": [(0, [0, 1])],
    "ones_two_frames": [(0, list(range(28))), (1, list(range(28, 56))), (2, list(range(56, 64)))],
}


def clouds(frames, grid="kitti", seed=0, interleave=True):
    """Points (N, 5) [b, x, y, z, r] fp32 whose voxels, in the order of their first points, hold `frames[b]` points each, in distinct
    random cells, every point well inside its cell; and the frame offsets (B + 1,) int32.  interleave: a voxel's later points are
    mixed among the points of the voxels that follow (so the arena's segments are not in index order); else voxel after voxel."""
    G = GRIDS[grid]
    rng = np.random.default_rng(_seed(seed, len(frames), sum(map(sum, frames))))
    out, offs = [], [0]
    for b, counts in enumerate(frames):
        cells = rng.permutation(G["nx"] * G["ny"])[:len(counts)]
        left = list(counts)
        order, opened = [], 0
        while opened < len(counts) or any(left[:opened]):
            avail = [j for j in range(opened) if left[j] > 0]
            if opened < len(counts) and (not interleave or not avail or rng.random() < 0.4):
                j = opened
                opened += 1
            elif interleave:
                j = avail[int(rng.integers(len(avail)))]
            else:
                j = avail[0]
            if not interleave:                       # the whole voxel at once
                order += [j] * left[j]
                left[j] = 0
            else:
                order.append(j)
                left[j] -= 1
        order = np.asarray(order, int)
        u = 0.1 + 0.8 * rng.random((len(order), 3))
        cx, cy = cells[order] % G["nx"], cells[order] // G["nx"]
        p = np.empty((len(order), 5), np.float64)
        p[:, 0] = b
        p[:, 1] = G["lo"][0] + (cx + u[:, 0]) * G["vs"][0]
        p[:, 2] = G["lo"][1] + (cy + u[:, 1]) * G["vs"][1]
        p[:, 3] = G["lo"][2] + u[:, 2] * G["vs"][2]
        p[:, 4] = rng.random(len(order))
        out.append(p)
        offs.append(offs[-1] + len(order))
    return np.concatenate(out).astype(np.float32), np.asarray(offs, np.int32)


def capped_cloud(seed=0):
    """One frame for cap_mode = 1 with max_voxels = 2: voxel 0 gets 3 points, voxel 1 gets 2, the first point of voxel 2 is the
    cutoff, and then voxel 0 receives 4 more points and voxel 1 one more, which the cap drops.  The arena keeps all of them (counts
    7, 3, 2; live 3, 2): the voxelizer fills a voxel's arena segment from the top, so the points that arrived last — past the cutoff
    — stand in its first columns.  -> points (N, 5), offsets, max_voxels, the live counts."""
    G = GRIDS["kitti"]
    rng = np.random.default_rng(_seed(seed, 9))
    stream = [0, 0, 0, 1, 1, 2, 0, 0, 1, 0, 2, 0]
    cells = rng.permutation(G["nx"] * G["ny"])[:3]
    order = np.asarray(stream)
    u = 0.1 + 0.8 * rng.random((len(order), 3))
    cx, cy = cells[order] % G["nx"], cells[order] // G["nx"]
    p = np.zeros((len(order), 5), np.float64)
    p[:, 1] = G["lo"][0] + (cx + u[:, 0]) * G["vs"][0]
    p[:, 2] = G["lo"][1] + (cy + u[:, 1]) * G["vs"][1]
    p[:, 3] = G["lo"][2] + u[:, 2] * G["vs"][2]
    p[:, 4] = rng.random(len(order))
    return p.astype(np.float32), np.asarray([0, len(order)], np.int32), 2, [3, 2]


OBSERVED = """max err / bound on the MI355X.  Rows form (hvpr_pillar_vfe_fwd_f32), over the nineteen rows: pillar_features 0.0305
(kitti_corners; 0.013 to 0.027 elsewhere, 0.0258 on the 8195-pillar row), pillar_scale_features 0.0497 (zero_coordinate; 0.013 to
0.035 elsewhere).  Packed form (hvpr_encode_fwd_f32), over the sixteen sequences in index order and interleaved, the three floor
clouds and the V1-cap frame, the same figures with index_mode 0 and 1: pillar_features 0.0352 (ones_64), pillar_scale_features
0.0310 (ones_64); 0.0104 / 0.0088 on the V1-cap frame.  The fused form equalled the three separate calls, and the form without
the voxels / mask outputs the form with them, bit for bit on every sequence and on the natural frames.

How sharp the bound is (bound / largest element, test_vfe_eval_host.py): 8e-6 to 1.1e-5 on pillar_features, 5e-6 to 1.1e-5 on
pillar_scale_features: 70 to 90 units of fp32 round-off, of which the kernel and plain fp32 torch use 1 to 5 %.  The bound is a worst
case over a layer-1 path of 32 + 20 + 4 roundings all pushing one way; every wrong variant moves the touched elements by 1e-3 and more."""
