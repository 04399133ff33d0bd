"""The rounding bound of pfn_train_cases.py proves itself on the CPU, over every row test_gpu_pfn_train.py runs:

  * the kernels' formulas in fp32 torch — the forward, and for the gradients the CLOSED FORM of csrc/vfe_train.hip's header (dense
    BatchNorm term from the moments, Q and w for g_x1, the same one level down; no autograd) — are inside the bound on every element,
    and the float64 values the bound is drawn around agree with torch autograd of the module in float64: the algebra is checked too;
  * every row has ZERO undecided layer-0 decisions and at most MASKED_CAP masked layer-1 entries, from the reference alone;
  * the float64 reference with one mistake made is outside the bound on the outputs named for it, on every element the mistake
    touches or on the share stated there with its reason;
  * the rows reach the loop edges they are in the table for, by the restated launch arithmetic."""
import pytest
import torch

import pfn_train_cases as F


_ROWS = {}


def _row(name):
    if name not in _ROWS:                # (the sweep rows take seconds each: computed once, never changed)
        c = F.case(name)
        _ROWS[name] = (c, F.reference(c))
    c, r = _ROWS[name]
    if c.backward:                      # (a forward-only row has no gradient a flipped decision could move: ReLU and max are 1-Lipschitz)
        assert r["undecided0"] == 0, (name, r["undecided0"])
        assert r["masked_share"] <= F.MASKED_CAP, (name, r["masked_share"])
    return c, r


@pytest.mark.parametrize("name", list(F.ROWS))
def test_fp32_closed_form_is_inside_the_bound_and_matches_autograd(name, observed):
    c, r = _row(name)
    fr = F.fractions(F.standin(c, r["d_out"]), r)
    assert set(fr) == set(F.FORWARD + (F.GRADS if c.backward else ())), (name, sorted(fr))
    worst = max(fr, key=fr.get)
    observed(f"pfn train host [{name}] M={c.M} P={c.P}: fp32 closed form uses at most {fr[worst]:.4f} of the bound ({worst}); "
             f"masked share {r['masked_share']:.2e}")
    assert fr[worst] <= 1.0, (name, fr)
    want = F.autograd64(c, r["d_out"])
    for k, v in want.items():
        # float64 noise of two different evaluation orders, against the largest element (1e-3 at least: the exactly-zero rows)
        assert float((r[k].v - v).abs().max()) <= 1e-9 * max(float(v.abs().max()), 1e-3), (name, k)


def test_exact_rows():
    """d_out = 0: every gradient has value and bound exactly 0.  gamma1 == 0: its dW1 row has; a channel whose maximum is 0 has in
    dW1, d gamma1, d beta1.  gamma0 == 0: its dW0 row has.  The constant batch: both variances are 0."""
    r = F.reference(F.case("d_out_zero"))
    for k in F.GRADS:
        assert float(r[k].v.abs().max()) == 0.0 and float(r[k].e.max()) == 0.0, k
    c = F.case("affine_edges")
    r = F.reference(c)
    assert float(c.gamma0[3]) == 0.0 and float(c.gamma1[5]) == 0.0 and float(c.beta1[7]) == -50.0
    for ch in (5, 7):
        assert float(r["dw1"].v[ch].abs().max()) == 0.0 and float(r["dw1"].e[ch].max()) == 0.0, ch
    assert float(r["out"].v[:, 7].abs().max()) == 0.0 and float(r["dgamma1"].v[7]) == 0.0 == float(r["dbeta1"].e[7])
    assert float(r["dw0"].v[3].abs().max()) == 0.0 and float(r["dw0"].e[3].max()) == 0.0
    assert float(r["dbeta1"].v[5].abs()) > 0 and float(c.gamma0.min()) < 0 and float(c.gamma1.min()) < 0
    r = F.reference(F.case("constant_batch"))
    assert float(r["var0"].v.max()) <= 1e-20 and float(r["var1"].v.max()) <= 1e-20


# (wrong variant, row, output) -> the share of the touched elements that must be caught where that is not all of them, and which
# elements escape.  The floors are the shares of these float64 computations, rounded down.  What escapes is always an element
# that the mistake moves by less than the worst-case rounding of its own sum (every one of up to 65 k slots' roundings taken to
# push the same way: 1e-3 to 1e-2 of the largest element on the layer-0 gradients, which the fp32 closed form uses 1e-4 of).
STATED_SHARES = {
    # one padded row in twenty missing from s1, S1: the entries of dW1 whose dense term is smallest
    ("pad_multiplicity_minus_1", "all_one_point", "dw1"): 0.99,
    # a lane past P raises m0 only in the channels whose padded value tops every live slot of a pillar: few entries of x1 move,
    # the statistics of the y1 channels with little weight on them stay, and `out` moves only where such an entry carries weight
    # in the arg-max slot's y1
    ("lanes_past_P_in_max", "all_full_20", "mean1"): 0.93,
    ("lanes_past_P_in_max", "all_full_20", "var1"): 0.79,
    ("lanes_past_P_in_max", "all_full_20", "out"): 0.47,
    ("dense_dropped_dW1", "eight_pillars", "dw1"): 0.999,          # one entry of 2048 whose dense term is below the bound
    # the entries of dW0 whose dense term (c0 / N)(dbeta0 s0 + dgamma0 inv0 (W0 S0 - mu0 s0))[c][k] is about 1e-5 of the largest
    # entry ([3][6] and [5][3] on the small row)
    ("dense_dropped_dW0", "eight_pillars", "dw0"): 0.98,
    ("dense_dropped_dW0", "three_sweeps", "dw0"): 0.95,
    # unrouted, d beta0[c] loses sum_m gm[m, c] over the pillars whose maximum passes the ReLU; over ALL pillars that sum is exactly
    # 0, so a channel whose maximum fails in a few pillars only loses little (5e-6 of the largest element in channel 8 of the small
    # row); d gamma0 weighs the same terms by xhat0 of the maximum and is caught whole
    ("m0_grad_not_routed", "eight_pillars", "dbeta0"): 0.90,
    ("m0_grad_not_routed", "three_sweeps", "dw0"): 0.98,           # the rows of those channels
    # pillar 0 counted twice / the one pillar of the second sweep lost, among 2049: the planted weight of that pillar reaches an
    # entry of dW0 through x0 of its arg-max slots, a channel of d gamma0 through their xhat0: the entries where those are near 0
    ("inactive_half_as_pillar_0", "sweep_plus_1", "dw0"): 0.98,
    ("pillars_past_2048_lost", "sweep_plus_1", "dw0"): 0.93,
    ("pillars_past_2048_lost", "sweep_plus_1", "dgamma0"): 0.87,
    # half the pillars lost: the channel of d beta0 and the entries of dW0 whose two halves happen to differ by less than the bound
    ("pillars_past_2048_lost", "three_sweeps", "dbeta0"): 0.93,
    ("pillars_past_2048_lost", "three_sweeps", "dw0"): 0.97,
    ("unbiased_normalising", "eight_pillars", "out"): 0.99,        # n / (n - 1) = 40 / 39 on the scale: entries next to beta1 move less than the bound
}


@pytest.mark.parametrize("wrong", F.WRONG)
def test_a_wrong_variant_is_outside_the_bound(wrong, observed):
    for name, outputs in F.WRONG_CASES[wrong]:
        c, r = _row(name)
        bad = F.reference(c, wrong)
        # touched: moved by more than the float64 noise of two evaluation orders (d beta0 of a channel whose maximum passes the ReLU
        # in every pillar is NOT touched by the unrouted m0 gradient: sum_slots g_x1 = W1^T sum g_y1 = 0, BatchNorm's backward sums to 0)
        touched = {k: (bad[k].v - r[k].v).abs() > 1e-12 * r[k].v.abs().max() for k in outputs}
        shares = {k: F.caught_share(r[k], bad[k].v, touched[k]) for k in outputs}
        observed(f"pfn train host: {wrong} on [{name}]: caught share " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        for k in outputs:
            assert shares[k] >= STATED_SHARES.get((wrong, name, k), 1.0), (wrong, name, shares)


def test_the_rows_reach_the_loop_edges_they_claim():
    S = {k: (v["M"], v["P"]) for k, v in F.ROWS.items()}
    assert F.SWEEP == 2048 and [F.sweeps(m) for m in (1, 2047, 2048, 2049, 4096, 4097, 4100)] == [1, 1, 1, 2, 2, 3, 3]
    assert sorted({m for m, _ in S.values() if m < 10}) == [1, 2, 3, 8, 9]
    assert {p for _, p in S.values()} >= {1, 2, 5, 20, 31, 32}
    assert S["one_pillar"][0] == 1 and F.last_sweep(1) == (1, True)                       # half-wave 1 inactive from the start
    assert F.last_sweep(S["sweep_minus_1"][0]) == (1024, True) and F.last_sweep(S["sweep_exact"][0]) == (1024, False)
    assert F.last_sweep(S["sweep_plus_1"][0]) == (1, True) and F.sweeps(S["sweep_plus_1"][0]) == 2 and S["sweep_plus_1"][1] == 20
    assert F.sweeps(S["three_sweeps"][0]) == 3 and F.last_sweep(S["three_sweeps"][0]) == (2, False)
    for name, (m, p) in S.items():
        c = F.case(name)
        assert m * p <= 2049 * 32
        if m > 2048:                        # templates: m, m + 1 and m + 2048 differ somewhere, and the order is not periodic
            t = c.template
            assert 48 <= F.ROWS[name]["pool"] <= 96 and bool((t[:-1] != t[1:]).any()) and bool((t[:-2048] != t[2048:]).any())
            assert not torch.equal(t[:F.ROWS[name]["pool"]], t[F.ROWS[name]["pool"]:2 * F.ROWS[name]["pool"]])
    num = lambda name: F.case(name).num
    assert bool((num("all_full_32") == 32).all()) and bool((num("all_full_20") == 20).all()) and bool((num("all_one_point") == 1).all())
    assert num("one_next_to_full").tolist()[:4] == [1, 32, 1, 32] and bool((num("all_but_one_slot") == 19).all())
    n = num("sweep_plus_1")
    assert int(n.min()) == 1 and int(n.max()) == 20
    c = F.case("dirty_padding")
    pad = torch.arange(c.P)[None, :] >= c.num[:, None]
    assert bool(pad.any()) and bool((c.voxels[pad].abs().sum(-1) > 0).all())
    c = F.case("duplicated_points")
    assert torch.equal(c.voxels[:, 0], c.voxels[:, 1]) and int(c.num.min()) >= 2
    c = F.case("grid_corners")
    assert c.coords[0].tolist() == [0, 0, 0, 0] and c.coords[1].tolist() == [0, 0, F.GRID[1] - 1, F.GRID[0] - 1]
    c = F.case("constant_batch")
    assert bool((c.voxels == c.voxels[0]).all()) and bool((c.coords == c.coords[0]).all()) and c.P == 1
    r = F.reference(F.case("far_cluster"))
    assert float((r["mean0"].v.abs() / r["var0"].v.sqrt()).max()) > 100.0
    assert F.workspace_bytes() == 256 * 3232 * 4 + (2 + 3232 + 128) * 8 + 1504 * 4 + 256
