"""Host: kernels.edges_by_destination, the edge plan of every scattering gradient (the backward of _GroupRows, _FpRows, _GatherRows and
_AttendRows), on CPU tensors.  The plan is integers only: one wrong boundary does not crash, it sums a gradient over the wrong edges.
Every returned triple is walked by a plain loop (scatter_plan_cases.check_plan): each destination's chunks concatenate to exactly its
edge ids in ascending order, chunks hold 1..32 edges, the tail of chunk_ptr is empty chunks, the lengths are the documented ones."""
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
