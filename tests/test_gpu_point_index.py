"""GPU: the integer-producing ops of the training point stream at their edges — csrc/pointnet2.hip (k_fps<1|4|16|32>, k_ball_query,
k_three_nn) against oracle/hvpr_oracle.py, and hvpr_segment_sum_rows_f32 over the plans of kernels.edges_by_destination against a
float64 sum (and kernels.EdgePlan.sum_rows, the form every backward calls, over a plan of its own).  A wrong index here neither crashes nor gives NaN, it trains a slightly different network, so every comparison of
indices is exact.

Two kinds of cloud: "metric" = synthetic.hvpr_frame coordinates; "lattice" = multiples of 0.25 (queries: of 0.125) in a small cube,
where every product and sum of the squared distance is exact in fp32, equal distances are equal bits in any summation order, and
duplicates and exact ties are everywhere — there the documented tie rule (lowest index wins) decides the result."""
import functools

import numpy as np
import pytest
import torch

import scatter_plan_cases as P
from hvpr_amd import kernels, pointnet2, synthetic
from oracle import hvpr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2         # include/hvpr_amd.h:30-32
SENTINEL = -77


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the cached clouds are read-only


@functools.lru_cache(maxsize=None)
def _metric(seed, B, N):
    a = np.stack([synthetic.hvpr_frame(seed + b, num_points=N)[:, :3] for b in range(B)])
    a.setflags(write=False)
    return a


def _lattice(seed, B, N, step=0.25, lo=0.0):
    """Coordinates lo + step * {0..8/step - 1}: a cube of side 8."""
    rng = np.random.default_rng(seed)
    return (lo + step * rng.integers(0, int(8 / step), (B, N, 3))).astype(np.float32)


def _cloud(kind, seed, B, N):
    return _metric(seed, B, N) if kind == "metric" else _lattice(seed, B, N)


# ==================================================================================================== furthest point sampling
# one N per instantiation and per side of each dispatch boundary: <1> up to 1024, <4> up to 4096, <16> up to 16384, <32> up to 32768
FPS_N = (1, 2, 1023, 1024, 1025, 4096, 4097, 16384, 16385, 32768)


@pytest.mark.parametrize("kind", ("metric", "lattice"))
@pytest.mark.parametrize("N", FPS_N)
def test_fps_picks_equal_the_oracle(N, kind):
    xyz = _cloud(kind, 100 + N % 97, 2, N)
    assert not np.array_equal(xyz[0], xyz[1])                    # a wrong batch offset shows
    npoint = min(N, 48)
    got = pointnet2.furthest_point_sample(_dev(xyz), npoint).cpu().numpy()
    np.testing.assert_array_equal(got, O.furthest_point_sample(xyz, npoint))


def test_fps_of_every_point_of_a_distinct_cloud_is_a_permutation():
    N = 1025
    xyz = []
    for b in range(2):
        u = np.unique(synthetic.hvpr_frame(40 + b)[:, :3], axis=0)
        xyz.append(u[np.random.default_rng(b).permutation(len(u))[:N]])
    xyz = np.stack(xyz)
    got = pointnet2.furthest_point_sample(_dev(xyz), N).cpu().numpy()
    for b in range(2):
        assert sorted(got[b].tolist()) == list(range(N)), f"sample {b}: not a permutation"
    np.testing.assert_array_equal(got, O.furthest_point_sample(xyz, N))


def test_fps_all_identical_points_keeps_picking_by_the_tie_rule():
    xyz = np.empty((2, 1500, 3), np.float32)
    xyz[0], xyz[1] = (1.5, -2.25, 0.125), (30.1, 4.7, -1.3)
    got = pointnet2.furthest_point_sample(_dev(xyz), 20).cpu().numpy()
    ref = O.furthest_point_sample(xyz, 20)
    assert (ref == 0).all()                                       # every running minimum is 0 after step 1: index 0 wins every tie
    np.testing.assert_array_equal(got, ref)


def test_fps_all_points_beyond_the_initial_minimum_tie_at_step_one():
    rng = np.random.default_rng(5)
    xyz = (np.array([3e5, 3e5, 0.0]) + rng.uniform(-5e4, 5e4, (2, 3000, 3))).astype(np.float32)
    xyz[:, 0] = 0.0
    assert (np.linalg.norm(xyz[:, 1:].astype(np.float64), axis=-1) >= 2e5).all()      # d2 >= 4e10 > the 1e10 initial minimum
    got = pointnet2.furthest_point_sample(_dev(xyz), 16).cpu().numpy()
    ref = O.furthest_point_sample(xyz, 16)
    assert (ref[:, 1] == 1).all()                                 # step 1: every point but 0 still holds 1e10 -> lowest index
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("N,npoint,status", [(8, 9, INVALID_ARG), (8, 0, INVALID_ARG), (8, -1, INVALID_ARG), (32769, 4, UNSUPPORTED)],
                         ids=["npoint_above_N", "npoint_zero", "npoint_negative", "N_32769"])
def test_fps_refusals_leave_the_output_untouched(N, npoint, status):
    xyz = torch.zeros((1, N, 3), dtype=torch.float32, device=DEV)
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = kernels.lib().hvpr_furthest_point_sample_f32(xyz.data_ptr(), 1, N, npoint, out.data_ptr(), kernels._stream())
    torch.cuda.synchronize()
    assert rc == status
    assert (out == SENTINEL).all()
    if status == UNSUPPORTED:                                      # the largest supported size is accepted
        assert kernels.lib().hvpr_furthest_point_sample_f32(xyz.data_ptr(), 1, N - 1, npoint, out.data_ptr(), kernels._stream()) == OK
        torch.cuda.synchronize()
        assert (out[npoint:] == SENTINEL).all() and out[0] == 0


# ==================================================================================================== ball query
# a workgroup = 256 queries of one sample (M = 255 / 257: a partly dead workgroup), points staged in LDS tiles of 512 (N = 511 / 513 /
# 1500: a ragged last tile).  Every value of every axis appears; M = 257 meets N = 1500.
BQ_GRID = [(1, 1, 1, "lattice"), (255, 511, 16, "metric"), (256, 512, 64, "lattice"), (257, 513, 1, "metric"),
           (257, 1500, 16, "lattice"), (257, 1500, 64, "metric"), (1, 1500, 64, "lattice"), (256, 1, 16, "metric"),
           (255, 513, 1, "lattice"), (257, 511, 64, "lattice"), (256, 1500, 1, "metric")]


def _queries(kind, seed, xyz, M):
    """Queries that are not a subset of the points: metric = jittered picks, lattice = the twice finer lattice."""
    B, N, _ = xyz.shape
    rng = np.random.default_rng(seed)
    if kind == "lattice":
        return _lattice(seed, B, M, step=0.125)
    pick = rng.integers(0, N, (B, M))
    return (np.take_along_axis(xyz, pick[..., None], axis=1) + rng.normal(0.0, 0.3, (B, M, 3))).astype(np.float32)


@pytest.mark.parametrize("M,N,nsample,kind", BQ_GRID, ids=[f"M{m}-N{n}-ns{s}-{k}" for m, n, s, k in BQ_GRID])
def test_ball_query_equals_the_oracle(M, N, nsample, kind):
    B = 3
    xyz = _cloud(kind, 200 + M + N, B, N)
    new_xyz = _queries(kind, 300 + M + N, xyz, M)
    radius = 1.25 if kind == "lattice" else 1.0                  # lattice: d2 == r2 = 1.5625 happens (0.75, 1.0, 0), strict <
    got = pointnet2.ball_query(radius, nsample, _dev(xyz), _dev(new_xyz)).cpu().numpy()
    np.testing.assert_array_equal(got, O.ball_query(radius, nsample, xyz, new_xyz))


def _d2(points, q):
    d = points.astype(np.float64) - np.asarray(q, np.float64)
    return (d * d).sum(-1)


def _bq_row(points, q, r2, nsample):
    hits = np.nonzero(_d2(points, q) < r2)[0][:nsample]
    row = np.full(nsample, hits[0] if len(hits) else 0, np.int32)
    row[:len(hits)] = hits
    return row


R_AT, R_ABOVE = 1.25, float(np.nextafter(np.float32(1.25), np.float32(2)))
ROW_ZERO, ROW_ONE, ROW_OVERFULL, ROW_AT_RADIUS, ROW_LONE = 3, 64, 130, 200, 256
ROW_LATE = 77


def _constructed_ball_query():
    """B = 3, N = 1500 (tiles of 512, 512, 476), M = 257 (workgroup 1 of every sample has one live lane), lattice coordinates.
    Sample 0 holds the named rows; sample 2, the last, a first workgroup whose 256 queries all fill inside tile 0 and a lone live lane
    whose only hits are in tile 2; sample 1 the same with ONE query of the first workgroup (ROW_LATE) that has its hits in tile 2 only:
    that workgroup may not stop after tile 0 although 255 of its queries are full (all, not any)."""
    B, N, M = 3, 1500, 257
    xyz = _lattice(11, B, N, lo=16.0)                              # [16, 24)^3: nothing within 27 of the origin
    new_xyz = _lattice(12, B, M, step=0.125, lo=16.0)
    xyz[0, 700] = (0.75, 1.0, 0.0)                                 # d2 to the origin = 0.5625 + 1 = 1.5625 = 1.25^2 exactly
    xyz[0, 1100] = (50.25, 0.0, 0.0)                               # third tile; the only point near ROW_ONE
    new_xyz[0, ROW_ZERO] = (100.0, 100.0, 100.0)
    new_xyz[0, ROW_ONE] = (50.0, 0.0, 0.0)
    new_xyz[0, ROW_OVERFULL] = (20.0, 20.0, 20.0)
    new_xyz[0, ROW_AT_RADIUS] = (0.0, 0.0, 0.0)
    new_xyz[0, ROW_LONE] = (19.0, 21.0, 20.0)
    rng = np.random.default_rng(13)
    xyz[2, :512] = 16.0 + 0.25 * rng.integers(0, 8, (512, 3))      # tile 0: a cluster in [16, 18)^3
    xyz[2, 512:1024, 0] += 16.0                                    # tile 1: x in [32, 40)
    xyz[2, 1024:, 1] += 16.0                                       # tile 2: y in [32, 40)
    new_xyz[2, :256] = 16.0 + 0.125 * rng.integers(4, 12, (256, 3))
    new_xyz[2, 256] = (20.0, 36.0, 20.0)
    xyz[1], new_xyz[1] = xyz[2], new_xyz[2]
    xyz[1, 1024:] = xyz[1, :1023:-1]                               # another order of tile 2, so the samples differ
    new_xyz[1, ROW_LATE] = (20.0, 36.0, 20.0)
    return xyz, new_xyz


@pytest.mark.parametrize("radius", (R_AT, R_ABOVE), ids=("radius_1.25", "radius_next_above_1.25"))
def test_ball_query_named_rows_early_exit_and_lone_live_lane(radius):
    nsample = 16
    xyz, new_xyz = _constructed_ball_query()
    r2 = float(np.float32(radius) * np.float32(radius))
    # the construction is what it claims to be (float64; every lattice distance is exact in either precision)
    assert (_d2(xyz[0], new_xyz[0, ROW_ZERO]) > 100.0 ** 2).all()
    assert np.nonzero(_d2(xyz[0], new_xyz[0, ROW_ONE]) < r2)[0].tolist() == [1100]
    for row in (ROW_OVERFULL, ROW_LONE):
        assert (_d2(xyz[0], new_xyz[0, row]) < r2).sum() > nsample
    near_origin = _d2(xyz[0], new_xyz[0, ROW_AT_RADIUS])
    assert near_origin[700] == 1.5625 and (np.delete(near_origin, 700) > 100.0).all()
    for m in range(256):
        assert (_d2(xyz[2, :512], new_xyz[2, m]) < r2).sum() >= nsample             # workgroup 0 of sample 2 is full after tile 0
    lone = np.nonzero(_d2(xyz[2], new_xyz[2, 256]) < r2)[0]
    assert len(lone) > 0 and lone[0] >= 1024                                        # workgroup 1 must walk on to tile 2
    for m in range(256):                                                            # sample 1: all but ROW_LATE are full after tile 0
        assert m == ROW_LATE or (_d2(xyz[1, :512], new_xyz[1, m]) < r2).sum() >= nsample
    late = np.nonzero(_d2(xyz[1], new_xyz[1, ROW_LATE]) < r2)[0]
    assert len(late) > 0 and late[0] >= 1024

    got = pointnet2.ball_query(radius, nsample, _dev(xyz), _dev(new_xyz)).cpu().numpy()
    assert (got[0, ROW_ZERO] == 0).all(), "zero hits -> all zeros"
    assert (got[0, ROW_ONE] == 1100).all(), "one hit (third tile) -> that index in every slot"
    for row in (ROW_OVERFULL, ROW_LONE):
        np.testing.assert_array_equal(got[0, row], _bq_row(xyz[0], new_xyz[0, row], r2, nsample),
                                      err_msg=f"row {row}: more than nsample in range -> the first nsample by index")
    if radius == R_AT:
        assert (got[0, ROW_AT_RADIUS] == 0).all(), "d2 == radius^2 is outside (strict <)"
    else:
        assert (got[0, ROW_AT_RADIUS] == 700).all(), "d2 just below radius^2 is inside"
    np.testing.assert_array_equal(got[2, 256], _bq_row(xyz[2], new_xyz[2, 256], r2, nsample), err_msg="lone live lane, last workgroup")
    np.testing.assert_array_equal(got[1, ROW_LATE], _bq_row(xyz[1], new_xyz[1, ROW_LATE], r2, nsample),
                                  err_msg="one query still empty after tile 0: its workgroup must walk on")
    np.testing.assert_array_equal(got, O.ball_query(radius, nsample, xyz, new_xyz))


# ==================================================================================================== three nearest neighbours
@pytest.mark.parametrize("kind", ("metric", "lattice"))
@pytest.mark.parametrize("B,n,m", [(2, 300, 3), (3, 257, 4), (1, 1, 700), (2, 700, 256)])
def test_three_nn_equals_the_oracle(B, n, m, kind):
    unknown = _cloud(kind, 400 + n, B, n)
    known = _cloud(kind, 500 + m, B, m)
    d, i = pointnet2.three_nn(_dev(unknown), _dev(known))
    rd, ri = O.three_nn(unknown, known)
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_allclose(d.cpu().numpy(), rd, rtol=1e-6, atol=1e-7)


def test_three_nn_tied_neighbours_come_in_ascending_index_order():
    B, n = 2, 300
    base = _lattice(21, B, 4)
    known = np.concatenate([base, base], axis=1)                    # known[4 + i] == known[i]: every distance occurs (at least) twice
    unknown = _lattice(22, B, n, step=0.125)
    d, i = (t.cpu().numpy() for t in pointnet2.three_nn(_dev(unknown), _dev(known)))
    rd, ri = O.three_nn(unknown, known)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_allclose(d, rd, rtol=1e-6, atol=1e-7)
    assert (d[..., 0] == d[..., 1]).all()
    for a in (0, 1):
        tied = d[..., a] == d[..., a + 1]
        assert (i[..., a][tied] < i[..., a + 1][tied]).all()
    triple = np.repeat(base[:, :1], 3, axis=1)                        # m = 3, one point three times
    _, i3 = pointnet2.three_nn(_dev(unknown), _dev(triple))
    assert (i3.cpu().numpy() == np.array([0, 1, 2])).all()


def test_three_nn_unknown_on_a_known_point_has_distance_zero_and_the_lowest_index():
    B = 2
    base = _metric(23, B, 100)
    assert all(len(np.unique(base[b], axis=0)) == 100 for b in range(B))
    known = np.concatenate([base, base[:, :50]], axis=1)            # m = 150; rows 100..149 repeat rows 0..49
    unknown = np.concatenate([base, _metric(24, B, 60)], axis=1)     # rows 0..99 lie on known points
    d, i = (t.cpu().numpy() for t in pointnet2.three_nn(_dev(unknown), _dev(known)))
    assert (d[:, :100, 0] == 0.0).all()
    np.testing.assert_array_equal(i[:, :100, 0], np.broadcast_to(np.arange(100), (B, 100)))
    assert (d[:, :50, 1] == 0.0).all()
    np.testing.assert_array_equal(i[:, :50, 1], np.broadcast_to(np.arange(100, 150), (B, 50)))
    rd, ri = O.three_nn(unknown, known)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_allclose(d, rd, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("m", (2, 0))
def test_three_nn_refuses_fewer_than_three_known_points(m):
    unknown = torch.zeros((1, 5, 3), dtype=torch.float32, device=DEV)
    known = torch.zeros((1, 3, 3), dtype=torch.float32, device=DEV)
    dist = torch.full((1, 5, 3), float(SENTINEL), dtype=torch.float32, device=DEV)
    idx = torch.full((1, 5, 3), SENTINEL, dtype=torch.int32, device=DEV)
    rc = kernels.lib().hvpr_three_nn_f32(unknown.data_ptr(), known.data_ptr(), 1, 5, m, dist.data_ptr(), idx.data_ptr(), kernels._stream())
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    assert (dist == SENTINEL).all() and (idx == SENTINEL).all()


# ==================================================================================================== segment sum over the edge plans
U = 2.0 ** -24
PLANS = P.cases()
# (C, with edge_row, with edge_w, src_off, columns right of the slice)
SEG_FORMS = [(1, True, False, 3, 2), (24, True, True, 3, 2), (64, False, False, 0, 0), (64, True, True, 5, 3), (24, False, True, 2, 0),
             (1, True, True, 0, 4)]


def _gamma(k):
    return k * U / (1.0 - k * U)


def _seg_problem(plan, C, rows, weights, off, right, integer=False):
    """Inputs of kernels.segment_sum_rows for a plan in the shapes its callers use (rows + weights: row = edge // 3 as in _FpRows;
    rows alone: row = edge as in _GroupRows; no rows: src already sorted by the plan), and per-edge terms for the float64 reference.
    Everything a dropped edge could bring in is NaN (its weight, or its row where there are no weights), and so are the columns
    outside [off, off + C)."""
    dst, n_dst = PLANS[plan]
    E = len(dst)
    rng = np.random.default_rng(E + C)
    order, chunk_ptr, dest_ptr = kernels.edges_by_destination(torch.from_numpy(dst), n_dst)
    o = order.numpy().astype(np.int64)
    live = (dst >= 0) & (dst < n_dst)
    row_of = np.arange(E) // 3 if rows and weights else np.arange(E)       # source row of edge e (before any sorting)
    n_rows = max(int(row_of.max()) + 1 if E else 0, 1)
    draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float32)) if integer else (lambda *s: rng.standard_normal(s).astype(np.float32))
    x = draw(n_rows, C)
    w = (rng.integers(1, 4, E) if integer else rng.uniform(0.1, 1.0, E)).astype(np.float32) if weights else None
    if weights:
        w[~live] = np.nan
    else:
        x[:E][~live] = np.nan                                      # one row per edge: the dropped edges' rows
    src = np.full((n_rows, off + C + right), np.nan, np.float32)
    src[:, off:off + C] = x
    if not rows:                                                   # no edge_row: the kernel reads row p for position p of the plan
        src = src[o] if E else src
    term = x[row_of].astype(np.float64) * (w.astype(np.float64)[:, None] if weights else 1.0)      # (E, C), float64 of fp32 inputs
    args = dict(src=_dev(src), src_off=off, C=C, edge_row=_dev(row_of[o].astype(np.int32)) if rows else None,
                edge_w=_dev(w[o]) if weights else None, chunk_ptr=chunk_ptr.to(DEV), dest_ptr=dest_ptr.to(DEV), n_dst=n_dst)
    return args, torch.from_numpy(dst[live]), torch.from_numpy(term[live]), n_dst


def _seg_reference(dst_live, term_live, n_dst):
    C = term_live.shape[1]
    ref = torch.zeros((n_dst, C), dtype=torch.float64).index_add_(0, dst_live, term_live)
    mag = torch.zeros((n_dst, C), dtype=torch.float64).index_add_(0, dst_live, term_live.abs())
    fan = torch.bincount(dst_live, minlength=n_dst).double()
    k = torch.clamp(fan, max=P.CHUNK) + torch.ceil(fan / P.CHUNK) + 1     # first-level sum + second-level sum + the weight product
    return ref, mag, fan, (_gamma(k)[:, None] * mag)


@pytest.mark.parametrize("C,rows,weights,off,right", SEG_FORMS,
                         ids=[f"C{c}-{'rows' if r else 'sorted'}{'-w' if w else ''}-off{o}" for c, r, w, o, _ in SEG_FORMS])
@pytest.mark.parametrize("plan", list(PLANS))
def test_segment_sum_rows_within_the_summation_bound(plan, C, rows, weights, off, right, observed):
    """|err| <= gamma_k * sum_e |w_e x_e| per destination, k = min(n_d, 32) + ceil(n_d / 32) + 1, gamma_k = k u / (1 - k u), u = 2^-24:
    the bound of a sequential fp32 sum of <= 32 terms, then of the ceil(n_d / 32) partials, plus one rounding of w * x (FMA
    contraction only tightens it).  Empty destinations are exactly 0, dropped edges (NaN here) bring nothing, two calls give the
    same bits."""
    args, dst_live, term_live, n_dst = _seg_problem(plan, C, rows, weights, off, right)
    ref, mag, fan, bound = _seg_reference(dst_live, term_live, n_dst)
    got_t = kernels.segment_sum_rows(**args)
    again = kernels.segment_sum_rows(**args)
    assert got_t.shape == (n_dst, C) and got_t.dtype == torch.float32
    got = got_t.cpu().double()
    assert torch.isfinite(got).all(), "a dropped edge or a column outside the slice was read"
    assert (got[fan == 0] == 0.0).all(), "a destination without edges is not exactly 0"
    err = (got - ref).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item() if n_dst else 0.0
    if plan == "fanins":
        observed(f"segment_sum_rows[{plan}-C{C}-rows{int(rows)}-w{int(weights)}]: max err / bound = {worst:.3f}")
    bad = torch.nonzero(err > bound)
    assert bad.numel() == 0, f"destination {bad[0, 0].item()} (fan-in {int(fan[bad[0, 0]])}) channel {bad[0, 1].item()}: err " \
                             f"{err[tuple(bad[0])].item():.3e} > bound {bound[tuple(bad[0])].item():.3e}"
    assert torch.equal(got_t.view(torch.int32), again.view(torch.int32)), "two calls differ"


def test_segment_sum_bound_would_catch_one_lost_edge_at_fan_in_2000():
    """The bound above is tight enough to see ONE lost term of typical size among 2000: the median |w x| of the 2000-edge destination
    is more than twice its bound in every channel, so no result can be inside the bound of both the full reference and the reference
    with that edge removed — and the reference with the median edge of channel 0 removed is outside the bound of what the kernel gives."""
    C = 24
    args, dst_live, term_live, n_dst = _seg_problem("fanins", C, True, True, 3, 2)
    ref, _, fan, bound = _seg_reference(dst_live, term_live, n_dst)
    d = P.FANINS.index(2000)
    assert fan[d] == 2000
    terms = term_live[dst_live == d]                                               # (2000, C)
    assert (terms.abs().median(dim=0).values > 2.0 * bound[d]).all()
    e = terms[:, 0].abs().argsort()[1000]
    got = kernels.segment_sum_rows(**args).cpu().double()
    assert ((got[d] - ref[d]).abs() <= bound[d]).all()
    assert (got[d, 0] - (ref[d, 0] - terms[e, 0])).abs() > bound[d, 0]


@pytest.mark.parametrize("rows,weights", [(True, True), (False, False)], ids=("rows-w", "sorted"))
@pytest.mark.parametrize("plan", list(PLANS))
def test_segment_sum_rows_of_small_integers_is_exact(plan, rows, weights):
    """x in -8..8, w in 1..3: every partial sum is an integer below 2^24, exact in fp32 in any order, so the result equals the
    float64 reference bit for bit — every live edge exactly once, whatever the rounding."""
    args, dst_live, term_live, n_dst = _seg_problem(plan, 24, rows, weights, 3, 2, integer=True)
    ref, mag, _, _ = _seg_reference(dst_live, term_live, n_dst)
    assert mag.numel() == 0 or mag.max() < 2 ** 24
    got = kernels.segment_sum_rows(**args).cpu().double()
    wrong = torch.nonzero((got != ref).any(dim=1)).flatten().tolist()
    assert not wrong, f"destinations {wrong[:5]}: {got[wrong[0], :4].tolist()} != {ref[wrong[0], :4].tolist()}"


# ==================================================================================================== kernels.EdgePlan.sum_rows
def test_edge_plan_sum_rows_per_3_with_weights_across_the_chunk_boundary():
    """The three-interpolate form (per = 3, one weight per edge) of EdgePlan.sum_rows with every neighbour index on known point 0 or
    1: fan-ins above 32, so every live destination is more than one chunk.  Same bound as
    test_segment_sum_rows_within_the_summation_bound; known points 2..4 get exactly 0; a second plan and a column slice of a wider
    source give the same bits."""
    B, m, n, C = 2, 5, 70, 8
    rng = np.random.default_rng(70)
    idx = rng.integers(0, 2, (B, n, 3)).astype(np.int32)
    w = rng.uniform(0.1, 1.0, (B, n, 3)).astype(np.float32)
    src = rng.standard_normal((B * n, C)).astype(np.float32)
    dst = (idx.astype(np.int64) + np.arange(B)[:, None, None] * m).reshape(-1)
    term = src.astype(np.float64)[np.arange(B * n * 3) // 3] * w.astype(np.float64).reshape(-1, 1)
    ref, _, fan, bound = _seg_reference(torch.from_numpy(dst), torch.from_numpy(term), B * m)
    live = [b * m + j for b in range(B) for j in (0, 1)]
    assert (fan[live] >= 33).all() and fan[live].sum() == fan.sum() == B * n * 3       # four destinations of two chunks and more
    plan = kernels.EdgePlan.batched(_dev(idx), m)
    got_t = plan.sum_rows(_dev(src), per=3, weights=_dev(w))
    assert got_t.shape == (B * m, C) and got_t.dtype == torch.float32
    got = got_t.cpu().double()
    assert (got[fan == 0] == 0.0).all(), "a known point without edges is not exactly 0"
    err = (got - ref).abs()
    bad = torch.nonzero(err > bound)
    assert bad.numel() == 0, f"destination {bad[0, 0].item()} (fan-in {int(fan[bad[0, 0]])}): err {err[tuple(bad[0])].item():.3e} > bound " \
                             f"{bound[tuple(bad[0])].item():.3e}"
    assert torch.equal(got_t, plan.sum_rows(_dev(src), per=3, weights=_dev(w))), "two calls differ"
    wide = np.full((B * n, 2 + C + 3), np.nan, np.float32)
    wide[:, 2:2 + C] = src
    again = kernels.EdgePlan.batched(_dev(idx), m).sum_rows(_dev(wide), 2, C, per=3, weights=_dev(w))
    assert torch.equal(got_t, again), "a fresh plan over a column slice differs"


def test_every_tensor_of_the_prefetched_index_plan_reaches_record_stream():
    """PointNet2MSG.forward keeps the prefetched plan's memory alive on the consumer stream through pointnet2._tensors_of: the tensors
    of every EdgePlan inside the plan must be among them (a plan object that the walk skipped would leave its order / chunk tables
    free for reuse by the side stream while the backward still reads them)."""
    from hvpr_amd.config import AttrDict
    cfg = AttrDict(SA_CONFIG=dict(NPOINTS=[16, 4], RADIUS=[[0.5, 1.0], [1.0, 2.0]], NSAMPLE=[[4, 8], [4, 8]],
                                  MLPS=[[[8, 8], [8, 8]], [[8, 16], [8, 16]]]), FP_MLPS=[[8, 8], [16, 16]])
    net = pointnet2.PointNet2MSG(cfg, input_channels=4)
    B, N = 2, 64
    pts = np.concatenate([np.repeat(np.arange(B, dtype=np.float32), N)[:, None], _lattice(31, B, N).reshape(-1, 3),
                          np.zeros((B * N, 1), np.float32)], axis=1)
    plan = net.index_plan(_dev(pts), B)
    plans = [p for pre in plan["sa"] for p in pre[3]] + [pre[2] for pre in plan["fp"].values()]
    assert len(plans) == 2 * 2 + 2 and all(isinstance(p, kernels.EdgePlan) for p in plans)
    walked = {t.data_ptr() for t in pointnet2._tensors_of(plan)}
    for p in plans:
        assert len(p.tensors()) == 3, "index_plan hands over BUILT plans (the sort runs on the prefetch stream)"
        assert all(t.numel() > 0 and t.data_ptr() in walked for t in p.tensors())
