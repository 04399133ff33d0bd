"""Host helpers of the post-processing tests: synthetic car boxes, and a numpy model of the candidate pre-filter of
hvpr_score_topk_f32 (hvpr_amd/csrc/postprocess.hip) that names the kernel path a frame takes.

The path of a frame:
  compact  n_scores <= SORTCAP: every passing score is a candidate (k_score_compact), ranked by k_rank_count / k_rank_place;
  rank     n_scores >  SORTCAP: 16-bit histogram pre-filter (k_score_hist, k_hist_find, k_score_compact_bin), at most SORTCAP
           candidates left, ranked by k_rank_count / k_rank_place;
  radix    as rank, but more than SORTCAP candidates survive the pre-filter: radix select + LDS bitonic sort in k_topk_select.
"""
import numpy as np

SORTCAP = 8192
HBINS = 65536


def car_boxes(rng, n, spread=40.0, clustered=True):
    """Car-sized boxes; clustered so that many pairs overlap."""
    if clustered:
        centres = rng.uniform([0, -20], [spread, 20], (max(n // 6, 1), 2))
        xy = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.8, (n, 2))
    else:
        xy = rng.uniform([0, -20], [spread, 20], (n, 2))
    z = rng.normal(-1.0, 0.2, (n, 1))
    size = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (n, 3))
    yaw = rng.uniform(-np.pi, np.pi, (n, 1))
    return np.concatenate([xy, z, size, yaw], 1).astype(np.float32)


def ord_bits(scores):
    """topk_ord of the kernel (csrc/postprocess.hip): float32 -> uint32 whose unsigned order is the score order; -0.0 takes the key of +0.0."""
    b = np.asarray(scores, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def passing_mask(scores, thresh):
    """k_score_*'s filter: score >= thresh, or every non-NaN score when thresh is None."""
    s = np.asarray(scores, np.float32)
    return ~np.isnan(s) if thresh is None else s >= np.float32(thresh)


def cut_bin(scores, thresh, pre_max):
    """k_score_hist + k_hist_find: the 16-bit bin that holds the pre_max-th largest passing score; 0 when fewer pass."""
    s = np.asarray(scores, np.float32)
    hist = np.bincount(ord_bits(s[passing_mask(s, thresh)]) >> 16, minlength=HBINS)
    at_or_above = np.cumsum(hist[::-1])[::-1]          # passing scores in bins >= b
    hit = np.nonzero(at_or_above >= pre_max)[0]
    return int(hit[-1]) if hit.size else 0


def candidate_mask(scores, thresh, pre_max):
    """The scores the kernel compacts into keys for ranking / selection."""
    s = np.asarray(scores, np.float32)
    keep = passing_mask(s, thresh)
    if s.size > SORTCAP:
        keep &= (ord_bits(s) >> 16) >= cut_bin(s, thresh, pre_max)
    return keep


def topk_candidates(scores, thresh, pre_max):
    """-> (number of candidates, path): the path is 'compact', 'rank' or 'radix' (module docstring)."""
    s = np.asarray(scores, np.float32)
    count = int(candidate_mask(s, thresh, pre_max).sum())
    if s.size <= SORTCAP:
        return count, "compact"
    return count, "rank" if count <= SORTCAP else "radix"


# ---------------------------------------------------------------------------------------------- score cases
# hvpr_car's anchor count, and a 512 x 512 grid with two anchors per cell
A_CAR, A_GRID = 146816, 524288
PRE_MAXES = (1, 500, 3000, 4095, 4096, 8192)


def scores_equal(A):
    """Every score 0.5 (an untrained head): all keys share one bin, the order is the id order."""
    return np.full(A, 0.5, np.float32)


def scores_saturated(A, seed=0, n_one=20000):
    """n_one scores exactly 1.0f (sigmoid saturation), the rest uniform in [0, 1)."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, A).astype(np.float32)
    s[rng.choice(A, n_one, replace=False)] = 1.0
    return s


def scores_cluster(A, seed=0, n_cluster=30000):
    """n_cluster scores inside the one 16-bit bin [0.69921875, 0.703125) — a third of them rounded to 4 decimals so that exact
    ties remain — the rest uniform below 0.69: the cut bin alone holds more than SORTCAP scores."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 0.69, A).astype(np.float32)
    c = rng.uniform(0.7, 0.703, n_cluster)
    c[: n_cluster // 3] = np.round(c[: n_cluster // 3], 4)
    s[rng.choice(A, n_cluster, replace=False)] = c.astype(np.float32)
    return s


def scores_cut_count(K, A=A_CAR, seed=0):
    """With pre_max = 4096: exactly K candidates after the pre-filter — 100 scores in the bins above [0.75, 0.75390625) and
    K - 100 inside it (every fifth one the same value), the rest uniform below 0.7."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 0.7, A).astype(np.float32)
    idx = rng.choice(A, K, replace=False)
    s[idx[:100]] = rng.uniform(0.95, 1.0, 100).astype(np.float32)
    c = rng.uniform(0.75, 0.7539, K - 100).astype(np.float32)
    c[::5] = np.float32(0.752)
    s[idx[100:]] = c
    return s


def scores_special(A, seed=0, n_zero=3000, n_nan=5000, n_inf=50):
    """Raw logits N(0, 3) (negative scores) with n_nan NaN, n_inf each of +inf and -inf and n_zero zeros of random sign."""
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 3, A).astype(np.float32)
    idx = rng.choice(A, n_nan + 2 * n_inf + n_zero, replace=False)
    s[idx[:n_nan]] = np.nan
    s[idx[n_nan:n_nan + n_inf]] = np.inf
    s[idx[n_nan + n_inf:n_nan + 2 * n_inf]] = -np.inf
    s[idx[n_nan + 2 * n_inf:]] = np.where(rng.uniform(size=n_zero) < 0.5, np.float32(-0.0), np.float32(0.0))
    return s


def scores_signed_zeros_on_top(A, seed=0, n_zero=10000):
    """n_zero zeros of random sign above negative scores (and 2000 NaN): with n_zero > SORTCAP, the zero bin is the cut bin
    and the whole selection is a tie between +0.0 and -0.0."""
    rng = np.random.default_rng(seed)
    s = -rng.uniform(0.001, 5, A).astype(np.float32)
    idx = rng.choice(A, n_zero + 2000, replace=False)
    s[idx[:n_zero]] = np.where(rng.uniform(size=n_zero) < 0.5, np.float32(-0.0), np.float32(0.0))
    s[idx[n_zero:]] = np.nan
    return s


def mixed_batch(A, seed=0):
    """Four frames for one call with thresh 0.3, pre_max 4096: radix (all 0.5), rank (uniform), nothing passes (all < 0.2),
    fewer than pre_max pass (200 of A, cut bin 0)."""
    rng = np.random.default_rng(seed)
    s = np.empty((4, A), np.float32)
    s[0] = scores_equal(A)
    s[1] = rng.uniform(0, 1, A)
    s[2] = rng.uniform(0, 0.2, A)
    s[3] = rng.uniform(0, 0.29, A)
    s[3, rng.choice(A, 200, replace=False)] = rng.uniform(0.3, 1, 200)
    return s


def _score_cases():
    """(name, scores factory, thresh, pre_maxes, path) of every single-frame score case of tests/test_gpu_post_paths.py."""
    out = []
    for A in (A_CAR, A_GRID):
        for thresh in (None, 0.25):
            out.append((f"equal{A}/{thresh}", lambda A=A: scores_equal(A), thresh, PRE_MAXES, "radix"))
            out.append((f"saturated{A}/{thresh}", lambda A=A: scores_saturated(A, 1), thresh, PRE_MAXES, "radix"))
            out.append((f"cluster{A}/{thresh}", lambda A=A: scores_cluster(A, 2), thresh, PRE_MAXES, "radix"))
    out += [("random8192", lambda: np.random.default_rng(3).uniform(0, 1, 8192).astype(np.float32), None, (4096,), "compact"),
            ("random8193", lambda: np.random.default_rng(3).uniform(0, 1, 8193).astype(np.float32), None, (4096,), "rank"),
            ("equal8193", lambda: scores_equal(8193), None, (4096,), "radix"),
            ("cut8192", lambda: scores_cut_count(8192), None, (4096,), "rank"),
            ("cut8193", lambda: scores_cut_count(8193), None, (4096,), "radix"),
            ("special/None", lambda: scores_special(A_CAR), None, (4096,), "rank"),
            ("special/-2", lambda: scores_special(A_CAR), -2.0, (4096,), "rank"),
            ("zeros_top/None", lambda: scores_signed_zeros_on_top(A_CAR), None, (1, 4095, 8192), "radix"),
            ("zeros_top/-1", lambda: scores_signed_zeros_on_top(A_CAR), -1.0, (1, 4095, 8192), "radix"),
            ("zeros_rank", lambda: scores_signed_zeros_on_top(A_CAR, n_zero=3000), None, (4096,), "rank")]
    return out


SCORE_CASES = _score_cases()
