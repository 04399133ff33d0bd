"""CPU: the host model of score top-k's pre-filter (tests/post_paths.py) against brute force, and the kernel path each score case
of tests/test_gpu_post_paths.py is built to take."""
import numpy as np
import pytest

import post_paths as P
from oracle import hvpr_oracle as O


@pytest.fixture(scope="module")
def built():
    from hvpr_amd import build
    return build.build()


def _brute_candidates(s, thresh, pre_max):
    """Sort the passing scores; the cut bin is the 16-bit bin of the pre_max-th of them (0 when fewer pass)."""
    passing = np.nonzero(P.passing_mask(s, thresh))[0]
    if s.size <= P.SORTCAP:
        return P.passing_mask(s, thresh), passing
    ranked = passing[O.stable_order_desc(s[passing])]
    cut = int(P.ord_bits(s[ranked[pre_max - 1]]) >> 16) if len(ranked) >= pre_max else 0
    return P.passing_mask(s, thresh) & ((P.ord_bits(s) >> 16) >= cut), ranked


def test_ord_bits_is_the_score_order():
    rng = np.random.default_rng(1)
    s = np.concatenate([rng.normal(0, 1e3, 2000), rng.normal(0, 1e-30, 500), [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45,
                                                                                 3.4e38, -3.4e38]]).astype(np.float32)
    k = P.ord_bits(s)
    a, b = rng.integers(0, len(s), 20000), rng.integers(0, len(s), 20000)
    np.testing.assert_array_equal(k[a] < k[b], s[a] < s[b])
    np.testing.assert_array_equal(k[a] == k[b], s[a] == s[b])
    assert P.ord_bits(np.float32(-0.0)) == P.ord_bits(np.float32(0.0))


@pytest.mark.parametrize("seed", range(6))
def test_topk_candidates_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    A = int(rng.choice([5, 8192, 8193, 20000, 60000]))
    kind = seed % 3
    if kind == 0:
        s = rng.uniform(0, 1, A).astype(np.float32)
        s[: A // 3] = np.round(s[: A // 3], 2)
    elif kind == 1:
        s = P.scores_special(max(A, 10000), seed)[:A]
    else:
        s = rng.choice(np.float32([0.25, 0.5, -0.0, 0.0, 1.0]), A)
    for thresh in (None, 0.0, 0.3, 2.0):
        for pre_max in (1, 7, 500, 4096, 8192):
            want, ranked = _brute_candidates(s, thresh, pre_max)
            got = P.candidate_mask(s, thresh, pre_max)
            np.testing.assert_array_equal(got, want)
            assert got[ranked[:pre_max]].all()               # the true top pre_max are candidates
            count, path = P.topk_candidates(s, thresh, pre_max)
            assert count == want.sum()
            assert path == ("compact" if A <= P.SORTCAP else "rank" if count <= P.SORTCAP else "radix")


@pytest.mark.parametrize("case", P.SCORE_CASES, ids=[c[0] for c in P.SCORE_CASES])
def test_score_cases_take_their_path(case):
    _, make, thresh, pres, path = case
    s = make()
    for pre in pres:
        count, got = P.topk_candidates(s, thresh, pre)
        assert got == path, (pre, count)
    if case[0].startswith("cut"):
        assert count == int(case[0][3:])


def test_mixed_batch_frames_take_different_paths():
    s = P.mixed_batch(P.A_CAR)
    got = [P.topk_candidates(f, 0.3, 4096) for f in s]
    assert [p for _, p in got] == ["radix", "rank", "rank", "rank"]
    assert got[2][0] == 0 and got[3][0] == 200 and P.cut_bin(s[3], 0.3, 4096) == 0 and P.cut_bin(s[1], 0.3, 4096) > 0


def test_workspace_sizes_grow_with_the_problem(built):
    """A workspace sized for (batch, n_scores) / n_max serves every smaller call: iou3d_nms_utils.nms_gpu runs NMS with
    n_max = pre_maxsize on the workspace of all n candidates (nms_gpu(8192 boxes, pre_maxsize=4096) needs the two-launch
    mask's segments inside a workspace sized for 8192)."""
    from hvpr_amd import _lib
    L = _lib.lib()
    nms = [L.hvpr_nms_workspace_bytes(n) for n in range(1, 16385)]
    assert all(a <= b for a, b in zip(nms, nms[1:]))
    for batch in (1, 2, 4):
        topk = [L.hvpr_score_topk_workspace_bytes(batch, n) for n in (1, 8192, 8193, P.A_CAR, P.A_GRID)]
        assert all(a <= b for a, b in zip(topk, topk[1:]))
