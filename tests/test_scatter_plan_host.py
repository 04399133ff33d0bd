"""Host: kernels.edges_by_destination, the edge plan of every scattering gradient (the backward of _GroupRows, _FpRows, _GatherRows and
_AttendRows), on CPU tensors.  The plan is integers only: one wrong boundary does not crash, it sums a gradient over the wrong edges.
Every returned triple is walked by a plain loop (scatter_plan_cases.check_plan): each destination's chunks concatenate to exactly its
edge ids in ascending order, chunks hold 1..32 edges, the tail of chunk_ptr is empty chunks, the lengths are the documented ones.
kernels.EdgePlan, the owner of that triple in the product: laziness, the batched form, and the edge -> source row / edge -> weight mapping
that sum_rows hands to the segment sum, against a plain loop."""
import numpy as np
import pytest
import torch

import scatter_plan_cases as P
from hvpr_amd import kernels

CASES = P.cases()


def _plan(dst, n_dst):
    order, chunk_ptr, dest_ptr = kernels.edges_by_destination(torch.from_numpy(dst), n_dst)
    for t in (order, chunk_ptr, dest_ptr):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    return order.numpy(), chunk_ptr.numpy(), dest_ptr.numpy()


def test_chunk_size_is_the_one_the_cases_are_built_around():
    assert kernels._SEG_CHUNK == P.CHUNK == 32


@pytest.mark.parametrize("name", list(CASES))
def test_plan_invariants(name):
    dst, n_dst = CASES[name]
    P.check_plan(dst, n_dst, *_plan(dst, n_dst))


def test_fanins_of_32_64_and_2000_cut_into_1_2_and_63_chunks_with_empty_destinations_between():
    dst, n_dst = CASES["fanins"]
    _, chunk_ptr, dest_ptr = _plan(dst, n_dst)
    per_dest = np.diff(dest_ptr).tolist()
    assert per_dest == [0, 1, 1, 1, 2, 2, 2, 3, 63, 0, 0, 1]                       # ceil(fan-in / 32), in destination order
    sizes = np.diff(chunk_ptr)[:dest_ptr[-1]]
    d2000 = sizes[dest_ptr[8]:dest_ptr[9]].tolist()
    assert d2000 == [32] * 62 + [16]                                               # 2000 = 62 * 32 + 16
    assert sizes[dest_ptr[7]:dest_ptr[8]].tolist() == [32, 32, 1]                  # 65
    assert dest_ptr[9] == dest_ptr[10] == dest_ptr[11]                             # two empty destinations before the last one


def test_out_of_range_destinations_are_dropped_and_leave_the_plan_of_the_rest_unchanged():
    dst, n_dst = CASES["fanins"]
    mixed, _ = CASES["fanins_with_dropped"]
    assert ((mixed < 0) | (mixed >= n_dst)).sum() == 300 and (mixed < 0).any() and (mixed >= n_dst).any()
    order, chunk_ptr, dest_ptr = _plan(mixed, n_dst)
    used = P.check_plan(mixed, n_dst, order, chunk_ptr, dest_ptr)
    covered = order[chunk_ptr[0]:chunk_ptr[used]]
    assert ((mixed[covered] >= 0) & (mixed[covered] < n_dst)).all() and len(covered) == len(dst)
    # the live edges keep their relative order, so the chunk sizes per destination are those of the clean input
    _, cp0, dp0 = _plan(dst, n_dst)
    np.testing.assert_array_equal(dest_ptr, dp0)
    np.testing.assert_array_equal(np.diff(chunk_ptr)[:used], np.diff(cp0)[:used])


def test_all_edges_out_of_range_and_no_edges_give_no_chunks():
    for name in ("all_dropped", "no_edges"):
        dst, n_dst = CASES[name]
        order, chunk_ptr, dest_ptr = _plan(dst, n_dst)
        assert (dest_ptr == 0).all() and (np.diff(chunk_ptr) == 0).all() and len(order) == len(dst), name
    assert len(_plan(*CASES["no_edges"])[1]) == 2                                  # E = 0: one spare (empty) chunk


def test_one_destination_with_2000_edges_is_63_chunks():
    dst, n_dst = CASES["one_destination_2000"]
    order, chunk_ptr, dest_ptr = _plan(dst, n_dst)
    assert dest_ptr.tolist() == [0, 63]
    np.testing.assert_array_equal(order, np.arange(2000))
    np.testing.assert_array_equal(chunk_ptr[:64], np.minimum(np.arange(64) * 32, 2000))


def test_plan_accepts_any_shape_and_int32_destinations():
    dst, n_dst = CASES["fanins"]
    ref = _plan(dst, n_dst)
    got = kernels.edges_by_destination(torch.from_numpy(dst.astype(np.int32)).view(2, -1), n_dst)
    for a, b in zip(ref, got):
        np.testing.assert_array_equal(a, b.numpy())


# ---------------------------------------------------------------------------------------------------- kernels.EdgePlan over the plan
# (3, 4) destinations into 5 rows: row 2 takes 5 edges, row 3 none, one edge each goes to -1 and to 5 (both outside: dropped)
PLAN_DST = np.array([[2, 0, -1, 2], [4, 2, 1, 5], [2, 0, 4, 2]], np.int64)
PLAN_ROWS = 5


def _walk(plan, d):
    """Positions in the plan's order that destination d sums over, chunk by chunk."""
    _, chunk_ptr, dest_ptr = (t.tolist() for t in plan.tensors()[:3])
    return [p for c in range(dest_ptr[d], dest_ptr[d + 1]) for p in range(chunk_ptr[c], chunk_ptr[c + 1])]


@pytest.mark.parametrize("per", (1, 3, 4))
def test_edge_plan_source_rows_and_weights_against_a_plain_loop(per):
    """What sum_rows hands to the segment sum: for every destination, in ascending edge id, the source row e // per and the weight of
    edge e — and nothing of the two dropped edges."""
    flat = PLAN_DST.reshape(-1).tolist()
    assert flat.count(2) == 5 and flat.count(3) == 0 and flat.count(-1) == 1 and flat.count(PLAN_ROWS) == 1
    w = torch.arange(len(flat), dtype=torch.float32).view(3, 4) * 0.5 + 100.0            # weight of edge e: 100 + e / 2, exact
    plan = kernels.EdgePlan(torch.from_numpy(PLAN_DST), PLAN_ROWS)
    rows, ew = plan.edge_rows(per), plan.edge_weights(w)
    assert rows.dtype == torch.int32 and rows.shape == (len(flat),) and ew.shape == (len(flat),) and ew.dtype == torch.float32
    assert plan.edge_rows(per) is rows, "the source rows are made once per `per`"
    seen = []
    for d in range(PLAN_ROWS):
        edges = [e for e, x in enumerate(flat) if x == d]                               # the plain loop: ascending edge ids
        pos = _walk(plan, d)
        assert [int(rows[p]) for p in pos] == [e // per for e in edges], (d, per)
        assert [float(ew[p]) for p in pos] == [100.0 + e / 2 for e in edges], (d, per)
        seen += edges
    assert sorted(seen) == [e for e, x in enumerate(flat) if 0 <= x < PLAN_ROWS] and len(seen) == len(flat) - 2


@pytest.mark.parametrize("per", (1, 3, 4))
def test_edge_plan_of_no_edges(per):
    plan = kernels.EdgePlan(torch.zeros((0, 4), dtype=torch.int64), PLAN_ROWS).build()
    order, chunk_ptr, dest_ptr = plan.tensors()
    assert order.numel() == 0 and (dest_ptr == 0).all() and dest_ptr.numel() == PLAN_ROWS + 1 and (chunk_ptr == 0).all()
    assert plan.edge_rows(per).shape == (0,) and plan.edge_rows(per).dtype == torch.int32
    assert plan.edge_weights(torch.zeros((0, 4))).shape == (0,)
    assert all(_walk(plan, d) == [] for d in range(PLAN_ROWS))


@pytest.mark.parametrize("dtype", (torch.int64, torch.int32))
def test_batched_edge_plan_equals_the_plan_of_the_hand_offset_list(dtype):
    idx = [[[0, 3], [3, 3], [1, 0]], [[2, 2], [0, 2], [3, 1]]]                             # (2, 3, 2) into 4 rows per sample
    by_hand = [0, 3, 3, 3, 1, 0, 4 + 2, 4 + 2, 4 + 0, 4 + 2, 4 + 3, 4 + 1]
    got = kernels.EdgePlan.batched(torch.tensor(idx, dtype=dtype), 4)
    want = kernels.EdgePlan(torch.tensor(by_hand), 8)
    assert got.n_dst == want.n_dst == 8
    for a, b in zip(got.build().tensors(), want.build().tensors()):
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)
    P.check_plan(np.array(by_hand), 8, *(t.numpy() for t in got.tensors()))
    assert torch.equal(got.idx32(), torch.tensor(idx, dtype=torch.int32)) and got.idx32() is got.idx32()


def test_edge_plan_is_lazy_build_is_idempotent_and_tensors_are_the_three_plan_tensors():
    plan = kernels.EdgePlan(torch.from_numpy(PLAN_DST), PLAN_ROWS)
    assert plan.tensors() == [], "nothing is sorted before the first use"
    assert plan.build() is plan
    first = plan.tensors()
    assert len(first) == 3
    P.check_plan(PLAN_DST, PLAN_ROWS, *(t.numpy() for t in first))
    assert plan.build() is plan
    assert all(a is b for a, b in zip(first, plan.tensors())) and len(plan.tensors()) == 3
    ref = kernels.edges_by_destination(torch.from_numpy(PLAN_DST), PLAN_ROWS)
    assert all(torch.equal(a, b) for a, b in zip(first, ref))
    rows3 = plan.edge_rows(3)                                                           # what the plan makes later is reported too
    assert any(t is rows3 for t in plan.tensors()) and all(a is b for a, b in zip(first, plan.tensors()))
