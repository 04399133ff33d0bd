"""Float64 references, the per-element rounding bounds and the case tables of the eval spatial gate and the head decode
(csrc/postprocess.hip: k_spatial_gate behind hvpr_spatial_gate_f32, k_head_decode behind hvpr_head_decode_f32), shared by
test_gate_head_host.py (the kernels' formulas in fp32 stand in for the kernels: the bounds prove themselves, and the reference with
one mistake made falls outside them) and test_gpu_gate_head.py (the kernels against the same bounds).  Plain torch / numpy, no GPU.
Q, qsum, gamma, used_fraction, caught_share and the constants come from bn_train_cases.py / conv_direct_cases.py; EXPF_ULP, the
project's stated assumption on expf (2 ulp), and pool_k come from gate_train_cases.py.

The references take exactly the fp32 words the entry points are handed (conv_bias, bn_scale, bn_shift, dir_offset, dir_limit_offset
and period cross the C interface as floats), widened to float64.

The gate.  gate = sigmoid(s (conv3x3(cat[max_c y, mean_c y], zero padding) + b) + t).  The bound, from k_spatial_gate:
  * max_c: exact.  sum_c: a lane takes T = ceil(C / 4 / 8) float4 groups, (x + y) + (z + w) and the accumulator: 3 roundings each,
    then a 3-step butterfly over its 8 lanes: k = 3 T + 3 (gate_train_cases.pool_k: k_gt_pool has the same loop); one division by C.
  * the convolution: a chain of 18 fmaf from 0: k = 18.  The pooled maps outside the image are 0 (not the -inf the max starts from).
  * (a + b) * s + t: three roundings (two if the multiply-add is fused: the unfused bound holds).
  * 1 / (1 + expf(-a)): expf within EXPF_ULP ulp of exp of its computed argument, the addition, the correctly rounded division.
    expf overflows for a < -88.7: the kernel returns 0 where the reference is below 2^-126, which every rounding's additive term covers.

The decode.  batch_cls_preds is a copy: bit-equal.  Boxes 0 .. 2: residual * diag + anchor with diag = sqrtf(fl(fl(dx dx) + fl(dy dy))),
and residual * dz + z: the product and the sum are the two roundings on top of diag's own.  Boxes 3 .. 5: fl(expf(residual) * size).
Box 6 without direction bins: one addition.  With bins the kernel pins contraction off and fixture G7 requires exactly these
roundings, so box 6 is compared BIT FOR BIT with heading32, an np.float32 restatement with one rounding per operation.  Scores: the
largest of the classes' sigmoids (1-Lipschitz).  Labels: 1 + the float64 arg-max; the table's logits are such that the two largest
sigmoids of every anchor are further apart than their two bounds (asserted from the reference alone), apart from the planted
anchors — exactly equal logits, and two classes whose sigmoids both round to 1.0f — where the lowest index wins.

Nothing here is fitted to what a kernel returns.  Observed on the MI355X: see OBSERVED at the end of this file."""
import numpy as np
import torch

from bn_train_cases import Q, TINY, caught_share, qsum, used_fraction  # noqa: F401  (re-exported to the tests)
from conv_direct_cases import SENTINEL, U, gamma  # noqa: F401
from gate_train_cases import EXPF_ULP, pool_k

GT = 16


def _seed(*row):
    return int(sum((int(v) + 1) * 131 ** i for i, v in enumerate(row)) % (2 ** 31 - 1))


def f32(x):
    return float(np.float32(x))


def _sigmoid(a):
    """1 / (1 + expf(-a)) of the computed argument a (Q)."""
    ev = torch.exp(-a.v)
    ee = ev * torch.expm1(a.e)
    ex = Q(ev, ee + 2.0 * EXPF_ULP * U * (ev + ee) + TINY)
    den = (ex + Q(torch.ones_like(ev))).rnd()
    lo = den.v - den.e
    assert bool((lo > 0).all())
    return Q(1.0 / den.v, den.e / (den.v * lo)).rnd()


# ================================================================================================ the gate
class GateCase:
    """y (N, H, W, C), w18 (18,): the max plane's nine taps, then the mean plane's; conv_bias, bn_scale, bn_shift.  content:
      negative     every channel of every pixel is negative: the max is below the padding's 0
      spike        every channel is 1 but one per pixel, which is 1e4
      bias_plus / bias_minus   conv_bias = +-30: the gate saturates       neg_scale    bn_scale < 0       zero_w    w18 = 0: a constant gate"""

    def __init__(self, N, H, W, C, content=None, seed=0, name=None):
        g = torch.Generator().manual_seed(_seed(N, H, W, C, seed))
        self.N, self.H, self.W, self.C, self.content = N, H, W, C, content
        self.name = name or f"{N}x{H}x{W}x{C}" + (f"_{content}" if content else "")
        y = torch.randn(N, H, W, C, generator=g)
        if content == "negative":
            y = -torch.rand(N, H, W, C, generator=g) - 0.1
        if content == "spike":
            y = torch.ones(N, H, W, C)
            at = torch.randint(0, C, (N, H, W, 1), generator=g)
            y.scatter_(3, at, 1e4)
        self.y = y.contiguous()
        self.w18 = (torch.randn(18, generator=g) * 0.4).contiguous()
        if content == "spike":
            self.w18 = self.w18 * 1e-3
        if content == "zero_w":
            self.w18 = torch.zeros(18)
        self.conv_bias = {"bias_plus": 30.0, "bias_minus": -30.0}.get(content, f32(torch.randn(1, generator=g).item()))
        self.bn_scale = f32(-1.3 if content == "neg_scale" else 0.5 + torch.rand(1, generator=g).item())
        self.bn_shift = f32(torch.randn(1, generator=g).item() * 0.2)

    def to(self, device):
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self


GATE_WRONG = ("pad_replicates_edge", "pad_minus_inf_as_is", "mean_over_C_plus_4", "taps_transposed", "max_and_mean_weights_swapped",
              "halo_off_by_one_at_16")


def _pad2(t, mode, value=0.0):
    """(N, H, W) -> (N, H + 4, W + 4): two cells of padding a side."""
    if mode == "replicate":
        return torch.nn.functional.pad(t[:, None], (2, 2, 2, 2), mode="replicate")[:, 0]
    return torch.nn.functional.pad(t, (2, 2, 2, 2), value=value)


def gate_reference(c, wrong=None):
    """-> dict: gate (N, H, W) Q, pooled (N, H, W, 2) Q.  wrong: one of GATE_WRONG — the same formulas with that mistake made:
    halo_off_by_one_at_16: the halo column right of a 16-wide tile holds the pixel one further, so the outputs of column 15 of every
    tile read x + 2 for their right-hand taps."""
    assert wrong is None or wrong in GATE_WRONG
    N, H, W, C = c.N, c.H, c.W, c.C
    f64 = torch.float64
    y = c.y.to(f64)
    mx = Q(y.max(-1)[0])
    sm = qsum(Q(y), -1, pool_k(C))
    div = float(C + 4 if wrong == "mean_over_C_plus_4" else C)
    mean = Q(sm.v / div, sm.e / div).rnd()
    w = c.w18.to(f64).view(2, 3, 3)
    if wrong == "taps_transposed":
        w = w.transpose(1, 2)
    if wrong == "max_and_mean_weights_swapped":
        w = w.flip(0)
    mode = "replicate" if wrong == "pad_replicates_edge" else "zero"
    planes = []
    for i, p in enumerate((mx, mean)):
        pad_v = float("-inf") if (wrong == "pad_minus_inf_as_is" and i == 0) else 0.0
        planes.append((_pad2(p.v, mode, pad_v), _pad2(p.e, mode, 0.0)))
    xs = torch.arange(W, device=y.device)
    v = torch.zeros(N, H, W, dtype=f64, device=y.device)
    e, S = torch.zeros_like(v), torch.zeros_like(v)
    for i in range(2):
        pv, pe = planes[i]
        for ky in range(3):
            for kx in range(3):
                tv, te = pv[:, ky + 1:ky + 1 + H, kx + 1:kx + 1 + W], pe[:, ky + 1:ky + 1 + H, kx + 1:kx + 1 + W]
                if wrong == "halo_off_by_one_at_16" and kx == 2:
                    edge = (xs % GT == GT - 1)[None, None, :]
                    tv = torch.where(edge, pv[:, ky + 1:ky + 1 + H, kx + 2:kx + 2 + W], tv)
                    te = torch.where(edge, pe[:, ky + 1:ky + 1 + H, kx + 2:kx + 2 + W], te)
                wk = w[i, ky, kx]
                if float(wk) == 0.0:
                    continue                          # (fmaf(0, p, a) = a: exact, and 0 * -inf is the wrong variant's business below)
                v = v + wk * tv
                e = e + wk.abs() * te
                S = S + wk.abs() * (tv.abs() + te)
    if wrong == "pad_minus_inf_as_is" and float(c.w18[:9].abs().sum()) == 0.0:      # 0 * -inf: not a number
        border = torch.zeros(N, H, W, dtype=torch.bool, device=y.device)
        border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = True, True, True, True
        v = torch.where(border, torch.full_like(v, float("nan")), v)
    acc = Q(v, e + gamma(18) * S + 18 * TINY * (S > 0))
    one = lambda x: Q(torch.full((), f32(x), dtype=f64, device=y.device))
    a = (((acc + one(c.conv_bias)).rnd() * one(c.bn_scale)).rnd() + one(c.bn_shift)).rnd()
    if wrong is not None:                              # (a wrong variant may be infinite or not a number: only its value is used)
        return {"gate": Q(1.0 / (1.0 + torch.exp(-a.v)), torch.zeros_like(a.v)), "a": a}
    return {"gate": _sigmoid(a), "a": a, "pooled": Q(torch.stack([mx.v, mean.v], -1), torch.stack([mx.e, mean.e], -1))}


def gate_standin(c):
    """k_spatial_gate's formulas in fp32 torch, in its order: a lane's float4 groups, the butterfly (xor 4, 2, 1), 18 fused multiply-adds
    (each rounded once: formed in float64 from fp32 operands, then rounded), the affine unfused, the sigmoid."""
    N, H, W, C = c.N, c.H, c.W, c.C
    y = c.y
    g4 = y.view(N, H, W, C // 4, 4)
    grp = (g4[..., 0] + g4[..., 1]) + (g4[..., 2] + g4[..., 3])                   # (N, H, W, C / 4)
    lanes = []
    for sub in range(8):
        s = torch.zeros(N, H, W)
        for i in range(sub, C // 4, 8):
            s = s + grp[..., i]
        lanes.append(s)
    l4 = [lanes[i] + lanes[i ^ 4] for i in range(8)]
    l2 = [l4[i] + l4[i ^ 2] for i in range(8)]
    sm = l2[0] + l2[1]
    mean, mx = sm / float(C), y.max(-1)[0]
    pm, pa = torch.nn.functional.pad(mx, (1, 1, 1, 1)), torch.nn.functional.pad(mean, (1, 1, 1, 1))
    a = torch.zeros(N, H, W)
    for ky in range(3):
        for kx in range(3):
            a = (c.w18[ky * 3 + kx].double() * pm[:, ky:ky + H, kx:kx + W].double() + a.double()).float()
            a = (c.w18[9 + ky * 3 + kx].double() * pa[:, ky:ky + H, kx:kx + W].double() + a.double()).float()
    a = (a + np.float32(c.conv_bias)) * np.float32(c.bn_scale) + np.float32(c.bn_shift)
    out = 1.0 / (1.0 + torch.exp(-a))
    assert out.dtype == torch.float32
    return out


GATE_SHAPES = ((1, 1, 1, 4), (1, 1, 17, 8), (2, 16, 16, 32), (1, 17, 33, 36), (1, 15, 16, 128), (3, 5, 3, 260))
# name -> GateCase arguments: every shape with random content, and every content on two shapes (a 1 x 1 image, all border; a tile
# edge at 16 / 17; more than one trip of a lane at C = 36 and 260)
GATE_ROWS = {f"{n}x{h}x{w}x{c}": dict(N=n, H=h, W=w, C=c) for n, h, w, c in GATE_SHAPES}
for _content, _shapes in (("negative", ((1, 1, 1, 4), (1, 17, 33, 36))), ("spike", ((1, 1, 17, 8), (3, 5, 3, 260))),
                          ("bias_plus", ((2, 16, 16, 32), (1, 1, 1, 4))), ("bias_minus", ((2, 16, 16, 32), (1, 1, 17, 8))),
                          ("neg_scale", ((1, 17, 33, 36), (1, 15, 16, 128))), ("zero_w", ((1, 15, 16, 128), (3, 5, 3, 260)))):
    for _n, _h, _w, _c in _shapes:
        GATE_ROWS[f"{_n}x{_h}x{_w}x{_c}_{_content}"] = dict(N=_n, H=_h, W=_w, C=_c, content=_content)

# wrong variant -> the rows on which every touched element must be outside the bound
GATE_WRONG_CASES = {
    "pad_replicates_edge": ("1x17x33x36", "1x1x1x4"),
    "pad_minus_inf_as_is": ("1x17x33x36_negative", "1x15x16x128_zero_w"),
    "mean_over_C_plus_4": ("1x17x33x36", "3x5x3x260"),
    "taps_transposed": ("1x17x33x36", "2x16x16x32"),
    "max_and_mean_weights_swapped": ("1x17x33x36", "3x5x3x260"),
    "halo_off_by_one_at_16": ("1x1x17x8", "1x17x33x36"),
}


def gate_case(name):
    return GateCase(**GATE_ROWS[name], name=name)


# ================================================================================================ the decode
DIR_OFFSET, DIR_LIMIT_OFFSET = 0.78539, 0.0


class HeadCase:
    """head (N, H, W, na (nc + 7 + nbins)): [class logits (na, nc) | box residuals (na, 7) | direction logits (na, nbins)] per pixel;
    x_shifts (W,), y_shifts (H,), anchor_table (na, 5) [z, dx, dy, dz, rot]; period = 2 pi / max(nbins, 1) as an fp32 word.
    Residuals in +-3 with a few size residuals at +-20; class logits in +-4 with +-30 and +-100 planted; headings drawn over several
    periods, with `near` of them placed within an ulp of a multiple of the period on either side; every seventh anchor's direction
    logits tied; planted label ties (nc > 1): anchor 0 has equal logits in classes 0 and 1, anchor 1 in the last two classes,
    anchor 2 saturates classes 0 (30) and 1 (100) to 1.0f, anchor 3 the same the other way round."""

    def __init__(self, N, H, W, na, nc, nbins, seed=0, name=None):
        g = torch.Generator().manual_seed(_seed(N, H, W, na, nc, nbins, seed))
        self.N, self.H, self.W, self.na, self.nc, self.nbins = N, H, W, na, nc, nbins
        self.name = name or f"{N}x{H}x{W}_a{na}_c{nc}_b{nbins}"
        self.CH = na * (nc + 7 + nbins)
        A = N * H * W * na
        self.period = f32(2.0 * np.pi / max(nbins, 1))
        self.dir_offset, self.dir_limit_offset = f32(DIR_OFFSET), f32(DIR_LIMIT_OFFSET)
        sizes = torch.tensor([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
        self.anchor_table = torch.stack([torch.cat([torch.tensor([-1.0 - 0.3 * (a % 3)]), sizes[a % 3] * (1.0 + 0.01 * a),
                                                    torch.tensor([0.0 if a % 2 == 0 else np.pi / 2])]) for a in range(na)]).float().contiguous()
        self.x_shifts = (torch.arange(W).float() * 0.32 + torch.rand(1, generator=g)).contiguous()
        self.y_shifts = (torch.arange(H).float() * 0.32 - 19.84 + torch.rand(1, generator=g)).contiguous()
        cls = torch.rand(A, nc, generator=g) * 8.0 - 4.0
        box = torch.rand(A, 7, generator=g) * 6.0 - 3.0
        box[:, 6] = torch.rand(A, generator=g) * 16.0 - 8.0
        dirs = torch.randn(A, max(nbins, 1), generator=g)[:, :nbins]
        idx = torch.arange(A)
        if A >= 8:
            box[idx % 11 == 5, 3 + (A % 3)] = 20.0
            box[idx % 11 == 7, 3 + ((A + 1) % 3)] = -20.0
            cls[idx % 13 == 4, 0] = 30.0
            cls[idx % 13 == 6, 0] = -30.0
            cls[idx % 13 == 8, nc - 1] = 100.0
            cls[idx % 13 == 10] = -100.0                       # (every class: all sigmoids underflow together, the first wins)
        self.planted = {}
        if nc > 1 and A >= 8:
            self.planted = {int(i): 1 for i in idx[idx % 13 == 10]}
            cls[0] = -3.0
            cls[0, 0] = cls[0, 1] = 2.5
            cls[1] = -3.0
            cls[1, nc - 2] = cls[1, nc - 1] = 1.25
            cls[2] = 0.0
            cls[2, 0], cls[2, 1] = 30.0, 100.0
            cls[3] = 0.0
            cls[3, 0], cls[3, 1] = 100.0, 30.0
            self.planted.update({0: 1, 1: nc - 1, 2: 1, 3: 1})    # flat anchor -> the label the lowest-index rule gives
        self.near = torch.zeros(A, dtype=torch.bool)
        if nbins > 0:
            dirs[idx % 7 == 3] = 0.5                                # tied direction logits: bin 0 wins
            ra = self.anchor_table[:, 4][idx % na]
            j = 0
            for k in (-2, -1, 0, 1, 2, 3):
                for step in (-1, 0, 1):
                    a_i = 4 + j if nc > 1 else j
                    if a_i >= A:
                        break
                    vt = np.float32(k * np.float64(np.float32(self.period)))
                    for _ in range(abs(step)):
                        vt = np.nextafter(vt, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
                    box[a_i, 6] = float(np.float32(np.float32(vt + np.float32(self.dir_offset)) - np.float32(ra[a_i])))
                    self.near[a_i] = True
                    j += 1
        per_anchor = torch.cat([cls.view(N, H * W, na * nc), box.view(N, H * W, na * 7), dirs.reshape(N, H * W, na * nbins)], -1)
        self.head = per_anchor.view(N, H, W, self.CH).float().contiguous()

    def parts(self):
        """cls (A, nc), box (A, 7), dirs (A, nbins), and per flat anchor its x, y and anchor row: flat = ((n H + iy) W + ix) na + a."""
        N, H, W, na, nc, nb = self.N, self.H, self.W, self.na, self.nc, self.nbins
        h = self.head.view(N * H * W, self.CH)
        cls = h[:, :na * nc].reshape(-1, nc)
        box = h[:, na * nc:na * (nc + 7)].reshape(-1, 7)
        dirs = h[:, na * (nc + 7):].reshape(N * H * W * na, nb)
        flat = torch.arange(N * H * W * na, device=h.device)
        a, pix = flat % na, (flat // na) % (H * W)
        return cls, box, dirs, self.x_shifts[pix % W], self.y_shifts[pix // W], self.anchor_table[a]

    def to(self, device):
        for k, v in vars(self).items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self


HEAD_WRONG = ("anchor_major_order", "diag_uses_dz", "dir_tie_takes_last", "labels_zero_based", "period_fused")


def heading32(rg_in, ra, dirs, dir_offset, dir_limit_offset, period, fused=False, tie_last=False):
    """Box 6 with direction bins in np.float32, one rounding per operation, as k_head_decode computes it.  fused: the product
    turns * period is not rounded before the subtraction (a fused multiply-subtract)."""
    f4 = np.float32
    bt, ra, d = np.asarray(rg_in, f4), np.asarray(ra, f4), np.asarray(dirs, f4)
    off, lim, per = f4(dir_offset), f4(dir_limit_offset), f4(period)
    dl = (d.shape[1] - 1 - np.argmax(d[:, ::-1], axis=1)) if tie_last else np.argmax(d, axis=1)          # (argmax: the first of equals)
    rg = bt + ra
    v = rg - off
    turns = np.floor(v / per + lim)
    assert turns.dtype == f4
    if fused:
        rot = (v.astype(np.float64) - turns.astype(np.float64) * np.float64(per)).astype(f4)
    else:
        back = turns * per
        rot = v - back
    out = (rot + off) + per * dl.astype(f4)
    assert out.dtype == f4
    return out, v, dl


def heading64(rg_in, ra, dirs, dir_offset, dir_limit_offset, period):
    """The same in float64 on the fp32 words -> (heading, the distance of v / period + limit offset from the nearest integer)."""
    bt, ra, d = (np.asarray(t, np.float32).astype(np.float64) for t in (rg_in, ra, dirs))
    off, lim, per = (np.float64(np.float32(t)) for t in (dir_offset, dir_limit_offset, period))
    v = bt + ra - off
    q = v / per + lim
    return v - np.floor(q) * per + off + per * np.argmax(d, axis=1), np.abs(q - np.round(q))


def head_reference(c, wrong=None):
    """-> dict: cls (N, A, nc) fp32 (bit-equal), box (N, A, 7) Q — column 6 exact (error 0) from heading32 when nbins > 0 —,
    score (N, A) Q, label (N, A) int64, undecided (N, A) bool: the two largest sigmoids are within their bounds of each other (and the
    anchor is not planted).  wrong: one of HEAD_WRONG — the same formulas with that mistake made."""
    assert wrong is None or wrong in HEAD_WRONG
    N, H, W, na, nc, nb = c.N, c.H, c.W, c.na, c.nc, c.nbins
    f64 = torch.float64
    cls, box, dirs, xa, ya, an = c.parts()
    dev = cls.device
    A = H * W * na
    r = {"cls": cls.reshape(N, A, nc).clone()}
    # scores and labels
    sg = _sigmoid(Q(cls.to(f64)))
    order = sg.v.argsort(dim=1, descending=True, stable=True)
    top = order[:, 0]
    pick = lambda t, i: t.gather(1, i[:, None])[:, 0]
    r["score"] = Q(sg.v.max(1)[0], sg.e.max(1)[0])
    label = cls.to(f64).argmax(1) + 1
    und = torch.zeros(N * A, dtype=torch.bool, device=dev)
    if nc > 1:
        second = order[:, 1]
        und = pick(sg.v, top) - pick(sg.e, top) <= pick(sg.v, second) + pick(sg.e, second)
    for flat, lab in c.planted.items():
        label[flat], und[flat] = lab, False
    if wrong == "labels_zero_based":
        label = label - 1
    # boxes
    B = Q(box.to(f64))
    z, dx, dy, dz, rot = (Q(an[:, i].to(f64)) for i in range(5))
    other = dz if wrong == "diag_uses_dz" else dy
    sq = ((dx * dx).rnd() + (other * other).rnd()).rnd()
    s = sq.v.sqrt()
    diag = Q(s, torch.maximum((sq.v + sq.e).sqrt() - s, s - (sq.v - sq.e).clamp_min(0.0).sqrt())).rnd()
    cols = [((B[:, 0] * diag).rnd() + Q(xa.to(f64))).rnd(), ((B[:, 1] * diag).rnd() + Q(ya.to(f64))).rnd(), ((B[:, 2] * dz).rnd() + z).rnd()]
    for i, size in ((3, dx), (4, dy), (5, dz)):
        ev = torch.exp(B.v[:, i])
        cols.append((Q(ev, 2.0 * EXPF_ULP * U * ev + TINY) * size).rnd())
    if nb == 0:
        cols.append((B[:, 6] + rot).rnd())
    else:
        h32, _, _ = heading32(box[:, 6].cpu().numpy(), an[:, 4].cpu().numpy(), dirs.cpu().numpy(), c.dir_offset, c.dir_limit_offset, c.period,
                              fused=wrong == "period_fused", tie_last=wrong == "dir_tie_takes_last")
        cols.append(Q(torch.from_numpy(h32).to(dev).to(f64)))
    bq = Q(torch.stack([q.v for q in cols], 1), torch.stack([q.e for q in cols], 1))
    out = {"box": bq, "score": r["score"], "label": label, "undecided": und}
    if wrong == "anchor_major_order":                  # the outputs in (anchor, pixel) order instead of (pixel, anchor)
        perm = torch.arange(N * A, device=dev).view(N, H * W, na).transpose(1, 2).reshape(-1)
        out = {"box": Q(bq.v[perm], bq.e[perm]), "score": Q(r["score"].v[perm], r["score"].e[perm]), "label": label[perm], "undecided": und[perm]}
        r["cls"] = r["cls"].reshape(N * A, nc)[perm].reshape(N, A, nc)
    r["box"] = Q(out["box"].v.view(N, A, 7), out["box"].e.view(N, A, 7))
    r["score"] = Q(out["score"].v.view(N, A), out["score"].e.view(N, A))
    r["label"], r["undecided"] = out["label"].view(N, A), out["undecided"].view(N, A)
    return r


def head_standin(c):
    """k_head_decode's formulas in np.float32, one rounding per operation -> cls, box, score (fp32), label (int64)."""
    f4 = np.float32
    cls, box, dirs, xa, ya, an = (t.cpu().numpy().astype(f4) for t in c.parts())
    N, A = c.N, c.H * c.W * c.na
    with np.errstate(over="ignore"):                 # expf(100) = inf, 1 / (1 + inf) = 0: as the kernel
        sg = f4(1) / (f4(1) + np.exp(-cls))
    assert sg.dtype == f4
    score, label = sg.max(1), sg.argmax(1) + 1
    diag = np.sqrt(an[:, 1] * an[:, 1] + an[:, 2] * an[:, 2])
    cols = [box[:, 0] * diag + xa, box[:, 1] * diag + ya, box[:, 2] * an[:, 3] + an[:, 0], np.exp(box[:, 3]) * an[:, 1],
            np.exp(box[:, 4]) * an[:, 2], np.exp(box[:, 5]) * an[:, 3]]
    if c.nbins == 0:
        cols.append(box[:, 6] + an[:, 4])
    else:
        cols.append(heading32(box[:, 6], an[:, 4], dirs, c.dir_offset, c.dir_limit_offset, c.period)[0])
    b = np.stack(cols, 1)
    assert b.dtype == f4
    return (torch.from_numpy(cls.reshape(N, A, c.nc)), torch.from_numpy(b.reshape(N, A, 7)), torch.from_numpy(score.reshape(N, A)),
            torch.from_numpy(label.reshape(N, A)))


# name -> (N, H, W, na, nc, nbins), and what the row is there for
HEAD_ROWS = {
    "one_anchor_no_bins": (1, 1, 1, 1, 1, 0),
    "one_pixel": (1, 1, 1, 2, 1, 2),
    "three_classes": (2, 3, 5, 6, 3, 2),                # six anchors a pixel, two frames, the label arg-max with planted ties
    "odd_image": (1, 7, 9, 2, 1, 2),
    "one_workgroup": (1, 16, 8, 2, 1, 2),               # exactly 256 threads
    "one_pixel_row_more": (1, 17, 8, 2, 1, 2),          # 272: a second workgroup of 16 live threads
    "three_bins": (1, 3, 4, 2, 2, 3),                   # period 2 pi / 3
}
HEAD_WRONG_CASES = {"anchor_major_order": "three_classes", "diag_uses_dz": "three_classes", "dir_tie_takes_last": "three_classes",
                    "labels_zero_based": "three_classes", "period_fused": "one_pixel_row_more"}


def head_case(name):
    return HeadCase(*HEAD_ROWS[name], name=name)


def head_fractions(box, score, r):
    """max err / bound: the boxes' bounded columns (0 .. 5, and 6 without bins: with bins column 6 has a zero bound, so only an exact
    match passes) and the scores."""
    return {"box": used_fraction(box, r["box"]), "score": used_fraction(score, r["score"])}


OBSERVED = """max err / bound on the MI355X.  Gate, over the eighteen rows: 0.4787 (3x5x3x260_spike: the channel sum of 1e4 + 259 loses
most of its bound's room to the one large term), 0.39 and 0.42 on the two rows with a negative bn_scale, 0.04 to 0.28 elsewhere, 0
on the rows saturated at 1.  The kernel and the fp32 stand-in give the same figures on every row but the two with conv_bias = -30,
where expf's result is the gate itself (0.2169 / 0.2814 against the stand-in's 0.2205 / 0.3205).

Decode, over the seven rows: boxes 0 .. 2 0.925 (one_pixel_row_more, column 1; 0.35 to 0.86 on the other rows with more than two
anchors): these bounds ARE two roundings on top of diag's, and among hundreds of elements one comes close to both half-ulps;
boxes 3 .. 5 0.330; box 6 without bins 0, with bins bit-equal to heading32 everywhere; scores 0.583; class copy and labels exact.
The 2 ulp assumed for expf: columns 3 .. 5, whose bound is 4 u of expf and 1 u of the product, use 0.33 of it, so at most 0.41 of the
assumption is used there — under half; the scores' 0.58 is of a bound in which expf is one of three terms (the addition and the
division are the others) and cannot be put down to expf alone."""
