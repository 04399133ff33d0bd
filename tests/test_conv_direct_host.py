"""The rounding bound of conv_direct_cases.py proves itself on the CPU, with torch's fp32 convolution / autograd standing in for
the kernel, over every row of every table test_gpu_conv_direct.py runs:

  * the stand-in is inside the bound on every element (a bound an honest fp32 implementation could miss would be wrong), and
  * the float64 reference with one term lost is outside it: one 8-channel chunk of one tap (weight gradient: one pixel tile) on at
    least half of the elements it touches, and one single product on at least half for every row with K <= 400 — so a kernel that
    skips a chunk, a tap, a tile or one product cannot hide inside the bound."""
import copy

import pytest
import torch

import conv_direct_cases as C

FAMILIES = C.families()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fp32_standin_is_inside_the_bound_everywhere(family, observed):
    worst = 0.0
    for op in FAMILIES[family]:
        ref, S = op.reference()
        frac = C.used_fraction(op.standin(), ref, S, op.K)
        assert frac <= 1.0, (type(op).__name__, op.dims, frac)
        worst = max(worst, frac)
    observed(f"conv direct host [{family}]: torch fp32 uses at most {worst:.4f} of the bound over {len(FAMILIES[family])} rows")


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_lost_term_is_outside_the_bound(family, observed):
    """Rows with a ReLU are evaluated with it off, gate and residual kept (where both sides clip to zero a lost term does not show;
    the bound is formed before the ReLU)."""
    low_chunk = low_single = 1.0
    for op in FAMILIES[family]:
        if getattr(op, "relu", False):
            op = copy.copy(op)
            op.relu = False
        ref, S = op.reference()
        bad, S_bad = op.reference("chunk")
        share = C.caught_share(ref, S, bad, S_bad, op.K)
        assert share >= 0.5, ("chunk", type(op).__name__, op.dims, op.K, share)
        low_chunk = min(low_chunk, share)
        bad, S_bad = op.reference("single")
        share = C.caught_share(ref, S, bad, S_bad, op.K)
        if op.dims not in C.SINGLE_PRODUCT_EXEMPT:          # (rows above SINGLE_PRODUCT_MAX_K only: the test below)
            assert share >= 0.5, ("single", type(op).__name__, op.dims, op.K, share)
            low_single = min(low_single, share)
    observed(f"conv direct host [{family}]: a lost chunk / tile is outside the bound on >= {low_chunk:.3f} of the touched elements, "
             f"a lost product on >= {low_single:.3f}")


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 1.5])
def test_a_broken_element_is_never_inside_the_bound(value):
    """One element that is not a number, infinite, or simply wrong among exact ones gives a fraction above 1 — also where the bound
    itself is zero (x / 0) — and counts as caught."""
    ref, S = torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    got = torch.tensor([1.0, value, 1.0, 1.0])
    assert C.used_fraction(ref.float(), ref, S, 8) == 0.0
    assert C.used_fraction(got, ref, S, 8) > 1.0
    assert C.used_fraction(got, ref, torch.zeros(4, dtype=torch.float64), 0) > 1.0          # bound 0: x / 0
    assert C.used_fraction(ref.float(), ref, torch.zeros(4, dtype=torch.float64), 0) == 0.0  # 0 / 0 is an exact match
    assert C.caught_share(ref, S, got.double(), S * torch.tensor([1.0, 0.5, 1.0, 1.0]), 8) == 1.0


def test_single_product_exemption_is_the_uneven_walk_row_alone():
    over = [r for r in C.WGRAD if C.Wgrad(*r).K > C.SINGLE_PRODUCT_MAX_K]
    assert len(over) == 4 and C.SINGLE_PRODUCT_EXEMPT < set(over) and len(C.SINGLE_PRODUCT_EXEMPT) == 1


def test_wgrad_rows_hit_the_reduce_loop_edges():
    """The first nine weight-gradient rows give k_wgrad_reduce the chunk counts at the edges of its 16-way unrolled loop, the uneven
    row fewer chunks than tiles."""
    got = [C.Wgrad(*r).n_chunks for r in C.WGRAD[:len(C.WGRAD_NPT_CHUNKS)]]
    assert got == C.WGRAD_NPT_CHUNKS
    assert {(r[3], r[4]) for r in C.WGRAD[:9]} == {(ci, co) for ci in (4, 12, 64) for co in (4, 36, 64)}
    N, H, W, ci, co, taps, s = C.WGRAD[9]
    assert C.wgrad_chunks(N, H, W, ci, co, taps, s) == 32 and N * -(-H // 8) * -(-W // 8) == 48
