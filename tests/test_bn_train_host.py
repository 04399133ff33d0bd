"""The rounding bound of bn_train_cases.py proves itself on the CPU, over every row test_gpu_bn_train.py runs:

  * the kernels' formulas in fp32 torch (fp32 partial sums in the slab / lane structure, the finalise in double) are inside the bound
    on every element, with the undecided share of every row under its cap;
  * the float64 reference with one mistake made — a pixel or a workspace row lost, the unbiased variance used for normalising or
    the biased one for the running update, s1 / n or s2 / n dropped, a >= mask, the gate left out of the sums, d gate without the
    ReLU, the slice offset ignored — is outside it on every element the mistake touches;
  * the rows reach the loop edges they are in the table for, by the restated launch arithmetic."""
import pytest
import torch

import bn_train_cases as B


def _check(name, c, observed):
    r = B.reference(c)
    share = B.undecided_share(r)
    assert share <= B.UNDECIDED_CAP, (name, share)
    fr = B.fractions(B.standin(c), r)
    assert set(fr) == {k for k in r if k != "undecided"}, (name, sorted(fr))
    worst = max(fr, key=fr.get)
    observed(f"bn train host [{name}]: fp32 stand-in uses at most {fr[worst]:.4f} of the bound ({worst}); undecided share {share:.2e}")
    assert fr[worst] <= 1.0, (name, fr)


@pytest.mark.parametrize("name", list(B.SMALL))
def test_fp32_standin_is_inside_the_bound_everywhere(name, observed):
    _check(name, B.case(name), observed)


@pytest.mark.parametrize("name", list(B.LARGE))
def test_fp32_standin_is_inside_the_bound_on_the_large_rows(name, observed):
    _check(name, B.case(name), observed)


@pytest.mark.parametrize("C", B.FINALIZE_C)
@pytest.mark.parametrize("rows", B.FINALIZE_ROWS)
def test_finalised_partial_rows_are_inside_the_bound(rows, C, observed):
    p = B.Partials(rows, C)
    assert p.count != rows
    r, bad = p.reference(), p.reference("lost_partial_row") if rows > 1 else None
    fr = B.fractions(p.standin(), r)
    observed(f"bn train host finalize rows={rows} C={C}: double finalise uses at most {max(fr.values()):.4f} of the bound")
    assert len(fr) == 3 and max(fr.values()) <= 1.0, fr
    if bad is not None:
        every = torch.ones(C, dtype=torch.bool)
        assert B.caught_share(r["mean"], bad["mean"].v, every) == 1.0 and B.caught_share(r["var"], bad["var"].v, every) == 1.0


@pytest.mark.parametrize("wrong", B.WRONG)
def test_a_wrong_variant_is_outside_the_bound(wrong, observed):
    kw, outputs = B.WRONG_CASES[wrong]
    c = B.Case(**kw)
    r, bad = B.reference(c), B.reference(c, wrong)
    assert B.undecided_share(r) <= B.UNDECIDED_CAP
    assert max(B.fractions(B.standin(c), r).values()) <= 1.0          # the inputs built for it are fair: the honest form is inside
    for k in outputs:
        touched = bad[k].v != r[k].v
        if k == "dz":
            touched &= ~r["undecided"]
        if wrong == "mask_ge":                    # differs only where the pre-activation is exactly zero: gamma = 0, beta = 0
            assert touched.nonzero().flatten().tolist() == [0]
        elif wrong != "dgate_without_relu":       # (a pixel all of whose channels pass the ReLU has the same d gate either way)
            assert bool(touched.all()), (wrong, k, float(touched.double().mean()))
        else:
            assert float(touched.double().mean()) > 0.9
        share = B.caught_share(r[k], bad[k].v, touched)
        assert share == 1.0, (wrong, k, share)
    observed(f"bn train host: {wrong} is outside the bound on every touched element of {', '.join(outputs)}")


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 1.5])
def test_a_broken_element_is_never_inside_the_bound(value):
    """One element that is not a number, infinite, or simply wrong among exact ones gives a fraction above 1 — also where the bound
    itself is zero (x / 0) — and counts as caught; a skipped element does not speak."""
    one, zero = torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    got = torch.tensor([1.0, value, 1.0, 1.0])
    q = B.Q(one, one * 1e-6)
    assert B.used_fraction(one.float(), q) == 0.0
    assert B.used_fraction(got, q) > 1.0
    assert B.used_fraction(got, B.Q(one, zero)) > 1.0                 # bound 0: x / 0
    assert B.used_fraction(one.float(), B.Q(one, zero)) == 0.0        # 0 / 0 is an exact match
    skip = torch.tensor([False, True, False, False])
    assert B.used_fraction(got, q, skip) == 0.0 and B.used_fraction(got, q, ~skip) > 1.0
    assert B.caught_share(q, got.double(), skip) == 1.0
    assert B.fractions({"dz": got, "y": got}, {"dz": q, "y": q, "undecided": skip})["dz"] == 0.0


def test_the_rounding_of_one_operation_and_of_a_sum():
    u = 2.0 ** -24
    x = torch.tensor([3.0, 0.0], dtype=torch.float64)
    q = B.Q(x).rnd()
    assert q.e[0] == 3.0 * u + B.TINY and q.e[1] == 0.0               # an exact zero stays exact
    p = B.Q(x, x * 0 + 0.5) * B.Q(x + 1.0, x * 0 + 0.25)
    assert p.v.tolist() == [12.0, 0.0] and p.e.tolist() == [3.0 * 0.25 + 4.0 * 0.5 + 0.125, 0.5 + 0.125]
    s = B.qsum(B.Q(torch.tensor([[1.0, -2.0, 4.0]], dtype=torch.float64)), 1, 5)
    assert s.v.item() == 3.0 and s.e.item() == B.gamma(5) * 7.0 + 5 * B.TINY


def test_the_rows_reach_the_loop_edges_they_claim():
    """Every branch the table is there for, from the restated slab / lane / grid arithmetic (which the GPU test pins against
    hvpr_bn_workspace_bytes)."""
    S = {k: (v["P"], v["C"]) for k, v in B.ROWS.items()}
    slab = lambda n: B.bn_slab(S[n][0])
    lanes = lambda n: B.bn_lanes(S[n][1])
    trips = lambda n: B.reduce_trips(*S[n])
    assert S["one_pixel"][0] == 1 and S["fewer_pixels_than_lanes"][0] < lanes("fewer_pixels_than_lanes") == 128
    # slab 64: the unrolled loop and the remainder loop in one workgroup
    assert slab("one_ragged_block") == 64 and lanes("one_ragged_block") == 16 and trips("one_ragged_block") == {(1, 0), (0, 3)}
    assert lanes("one_lane") == 1 and trips("one_lane") == {(16, 0), (1, 2)} and B.bn_blocks(S["one_lane"][0]) == 2
    assert S["twelve_groups"][1] // 4 == 12 and lanes("twelve_groups") == 21 and 12 * 21 == 252
    # a slab other than 64: remainder loop alone at 128, unrolled loop at 256; more than 1024 workspace rows for k_bn_finalize4
    assert slab("slab_128") == 128 and lanes("slab_128") == 128 and trips("slab_128") == {(0, 1), (0, 0)}
    assert slab("slab_256") == 256 and lanes("slab_256") == 32 and (2, 0) in trips("slab_256") and (0, 1) in trips("slab_256")
    assert B.bn_blocks(S["slab_128"][0]) == 2049 == B.bn_blocks(S["slab_256"][0])
    assert S["whole_slabs"][0] % slab("whole_slabs") == 0 and S["one_past_a_slab"][0] % slab("one_past_a_slab") == 1
    assert 256 < B.bn_blocks(S["two_trips_butterfly"][0]) <= 1024          # k_bn_finalize4: a second trip of its 256 threads, a third above
    # the grid-stride loops of k_bn_apply / k_bn_bwd_apply: a second, ragged trip; the whole last trip's dead waves and a pixel
    # group's dead lanes inside a live wave run the butterfly with live == false
    for name, groups, pow2 in (("two_trips_butterfly", 256, True), ("two_trips_atomics", 12, False)):
        P, C = S[name]
        n_trips, last, threads = B.apply_trips(P, C)
        assert C // 4 == groups and (groups & (groups - 1) == 0) == pow2 and B.ROWS[name]["gated"]
        assert B.apply_grid(P, C) == 16384 and n_trips == 2 and 0 < last < threads
        assert P * C * 4 <= 68 * 2 ** 20
    for name in B.DGATE:                         # one trip; below 64 groups its last wave holds live and dead pixels
        P, C = S[name]
        assert B.apply_trips(P, C)[0] == 1 and (C // 4 >= 64 or (P * (C // 4)) % 64 != 0)
    assert sorted(S[n][1] // 4 for n in B.DGATE) == [2, 8, 12, 64, 256]
    assert [B.dgate_atomics_meet(4 * g) for g in (2, 8, 64, 12, 256)] == [False, False, False, True, True]
    assert [B.dgate_k(4 * g) for g in (2, 8, 64, 256, 12)] == [6, 8, 11, 14, 16]
    # finalize: one row, under one wave, a second and a fifth trip of the 256 threads; k_bn_finalize for C % 4 != 0
    assert B.FINALIZE_ROWS == (1, 63, 257, 1030) and [c % 4 for c in B.FINALIZE_C] == [0, 2, 3, 0]
    # affine: a second workgroup; the sliced and gated rows
    assert S["two_affine_blocks"][1] > 256
    assert B.ROWS["gated_sliced_dy"]["gated"] and B.ROWS["gated_sliced_dy"]["sliced"] and not B.ROWS["no_relu"]["relu"]
    assert B.ROWS["gamma_zero"]["edge"] and all(sum(v["parts"]) == v["P"] and v["parts"][0] != v["parts"][1] for v in B.TWO_PART.values())
    assert B.reduce_k(1, 8) == 5 and B.reduce_k(60, 64) == 4 + 16 + 3 and B.reduce_k(262149, 8) == 1 + 128 + 3
    assert B.workspace_bytes(524291, 32) == 2049 * 2 * 32 * 4
