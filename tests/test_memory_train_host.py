"""The rounding bound of memory_train_cases.py proves itself on the CPU, over every row test_gpu_memory_train.py runs:

  * the kernels' formulas in fp32 torch are inside the bound on every element of every output, the values the bound is drawn around
    agree with torch autograd of the module's formula in float64, and no row has an item whose support decision the reference
    cannot take (the share of undecided rows is exactly 0; the redraws that took are reported);
  * the rows that are exact have value and bound exactly 0;
  * the float64 reference with one mistake made is outside the bound on the elements the mistake touches, at the stated share;
  * the rows reach the loop edges they are in the table for, by the restated launch arithmetic."""
import pytest
import torch

import memory_train_cases as M

# (wrong variant, output) -> the floor of the share of touched elements outside the bound, where it is not all of them; from the
# float64 computations of this file, rounded down
STATED_SHARES = {
    # the tail items 1984 .. 1998 are dominant in four rows and ordinary members of the support in five more: there the loss is
    # a small share of the row's y
    ("tile_tail_lost", "y"): 0.98,
    ("tile_tail_lost", "dx"): 0.95,
    # 64 x 130 entries all move; the few that stay inside are entries whose lost tile held next to nothing of them
    ("split_tail_lost", "dW"): 0.98,
    # 24 more copies of the last row: the entries of dW whose coefficient in that one row is next to nothing stay inside
    ("rows_clamped_counted", "dW"): 0.88,
    # q = sum t dt is a weighted mean of the dt: where it is small against a row's dt the loss is within the bound
    ("q_dropped", "dx"): 0.93,
    # t dy over 40 rows has both signs: a few entries of dW lose next to nothing with it
    ("cy_dropped", "dW"): 0.99,
    # Z of the next row is Z of this one within a few per cent on some rows; an entry whose terms are small there stays inside
    ("stale_stats", "dx"): 0.99,
    ("stale_stats", "dW"): 0.99,
    # c = sum_S a da is a sum of lam eps / (u + eps)^2 terms with the signs of dt - q (see the row live_c): in the rows where they
    # cancel, or where the item nearest lam sets the bound of hs', c and what hangs on it (c (a W) in dx, -a c in dW) are inside the
    # bound.  In crow only c moves visibly (half its elements); dW sums the -a c x over 40 rows with both signs
    ("shrink_eps_dropped", "crow"): 0.37,
    ("shrink_eps_dropped", "dx"): 0.77,
    ("shrink_eps_dropped", "dW"): 0.12,
    ("c_term_dropped", "dx"): 0.39,
    ("dense_dl_dropped", "dW"): 0.12,
}


@pytest.mark.parametrize("name", list(M.ROWS))
def test_fp32_standin_is_inside_the_bound_and_no_row_is_undecided(name, observed):
    c = M.case(name)
    r, s = M.reference(c), M.standin(c)
    assert M.undecided_share(c, r) == 0.0, name
    assert bool(r["undecided"][c.free].all()) and int(c.free.sum()) == (M.N_FREE if name == "near_threshold" else 0)
    fr = M.fractions(s, r, c.free)
    worst = max(fr, key=fr.get)
    observed(f"memory train host [{name}]: fp32 stand-in uses at most {fr[worst]:.4f} of the bound ({worst}); "
             f"{int((c.draws > 0).sum())} of {c.R} rows redrawn, {int(c.draws.max()) if c.R else 0} times at most")
    assert fr[worst] <= 1.0, (name, fr)
    assert bool((s["stats"][:, 3] == 0).all())
    if bool(c.free.any()):
        assert bool(torch.isfinite(s["y"][c.free]).all()) and bool(torch.isfinite(s["dx"][c.free]).all())
        assert bool((s["crow"][c.free] == 0).all()) and bool((r["crow"].v[c.free] == 0).all()) and bool((r["crow"].e[c.free] == 0).all())
    want = M.autograd64(c)
    for k, v in want.items():
        scale = float(v.abs().max()) + 1e-30
        assert float((r[k].v - v).abs().max()) <= 1e-9 * max(scale, 1e-3), (name, k)


def test_exact_rows_have_value_and_bound_zero():
    for name, outputs in M.EXACT.items():
        r = M.reference(M.case(name))
        for k in outputs:
            assert float(r[k].v.abs().max()) == 0.0 and float(r[k].e.max()) == 0.0, (name, k)
    r = M.reference(M.case("empty_all"))
    assert float(r["count"].max()) == 0 and float(r["stats"].v[:, 2].abs().max()) == 0.0 and float(r["stats"].e[:, 2].max()) == 0.0
    r = M.reference(M.case("dy_zero"))
    assert float(r["count"].min()) > 0 and float(r["y"].v.abs().max()) > 0
    # rows without a support inside live groups: exact zeros next to live rows
    c = M.case("mixed_groups")
    r = M.reference(c)
    empty = r["count"] == 0
    assert torch.equal(empty, torch.tensor([not M.MIXED_LIVE(i) for i in range(c.R)]))
    for k in ("y", "dx", "crow"):
        assert float(r[k].v[empty].abs().max()) == 0.0 and float(r[k].e[empty].max()) == 0.0, k


@pytest.mark.parametrize("wrong", M.WRONG)
def test_a_wrong_variant_is_outside_the_bound(wrong, observed):
    c, outputs = M.wrong_case(wrong), M.WRONG_CASES[wrong][1]
    r, bad = M.reference(c), M.reference(c, wrong)
    assert max(M.fractions(M.standin(c), r, c.free).values()) <= 1.0          # the inputs built for it are fair
    shares = {}
    for k in outputs:
        touched = ~(bad[k].v == r[k].v)                                        # (a NaN is touched)
        shares[k] = M.caught_share(r[k], bad[k].v, touched)
        assert shares[k] >= STATED_SHARES.get((wrong, k), 1.0), (wrong, k, shares[k], float(touched.double().mean()))
    observed(f"memory train host: {wrong} outside the bound on " + ", ".join(f"{v:.4f} of the touched {k}" for k, v in shares.items()))


def test_the_rows_reach_the_loop_edges_they_claim():
    S = {k: (v["R"], v.get("n_items", 2000)) for k, v in M.ROWS.items()}
    assert {r for r, _ in S.values()} >= {1, 15, 16, 17, 63, 64, 65, 2048, 2049}
    assert {n for r, n in S.values() if r == 40} >= {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048}
    assert max(r * n for r, n in S.values()) == 2049 * 2000 and S["wide_support"] == (33, 2048)
    # row groups and row tiles
    assert [M.row_groups(r) for r in (1, 15, 16, 17)] == [1, 1, 1, 2] and [M.row_tiles(r) for r in (63, 64, 65)] == [1, 1, 2]
    assert M.row_tiles(2048) == 32 and M.tiles_per_split(2048) == 1 and all(len(M.split_tiles(2048, s)) == 1 for s in range(32))
    assert M.row_tiles(2049) == 33 and M.tiles_per_split(2049) == 2
    assert [len(M.split_tiles(2049, s)) for s in range(32)] == [2] * 16 + [1] + [0] * 15
    assert M.dw_k(2048) == 256 + 32 and M.dw_k(2049) == 512 + 32 and M.dw_k(1) == 288
    # item tiles, slices, blocks, shares of n4
    assert [M.n_tiles(n) for n in (1, 15, 16, 17, 2047, 2048)] == [1, 1, 1, 2, 128, 128]
    assert sorted({M.first(w, b) for w in range(16) for b in (0, 1)}) == list(range(16)) and M.first(15, 1) == 0
    assert M.n_tiles(2048) // M.WAVES == 8 and M.n_tiles(17) < M.WAVES              # every wave 8 tiles; 14 waves none
    assert [M.n4(n) for n in (1, 4, 5, 2047)] == [1, 1, 2, 512] and [M.n4_per_wave(n) for n in (1, 63, 64, 65, 2000, 2048)] == [1, 1, 1, 2, 32, 32]
    assert [M.ipad(n) for n in (1, 127, 128, 129, 2047)] == [128, 128, 128, 256, 2048]
    assert [M.z_k(n) for n in (1, 64, 65, 2000, 2048)] == [7, 7, 8, 38, 38] and M.abar_k(2000) == 272 and M.abar_k(1) == 24
    assert M.workspace_bytes(1) == 16 * 256 + 32 * 128 * 256 + 256 and M.workspace_bytes(2048) == 2048 * 256 * 33 + 256
    # contents
    for n in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        cnt = M.reference(M.case(f"n{n}"))["count"]                 # 1 / n_items > lam: every item is in the support
        assert 1.0 / n > M.LAMBDA and (bool((cnt == n).all()) if n <= 129 else bool((cnt >= 0.9 * n).all())), (n, cnt.min())
    r = M.reference(M.case("n1"))
    assert bool((r["a"].v == 1).all()) and bool((r["count"] == 1).all())
    c = M.case("planted_borders")
    r = M.reference(c)
    b = M._borders(c.n_items)
    assert c.n_items % 16 and c.n_items % 128 and {0, c.n_items - 1, 15, 16, 63, 64, 127, 128, 1983, 1984, 1919, 1920} <= set(b)
    assert 4 * M.n4_per_wave(c.n_items) == 128                  # a wave's share of a W ends where a 128-item block does
    top = r["a"].v.argmax(1)
    assert top.tolist() == [b[i % len(b)] for i in range(c.R)] and bool((r["a"].v.max(1)[0] > 0.2).all())
    r = M.reference(M.case("one_item"))
    l = M.case("one_item").x.double() @ M.case("one_item").bank.double().t()
    assert bool((r["count"] == 1).all()) and bool((r["a"].v.max(1)[0] > 1 - 1e-6).all()) and bool(((l - l.max(1, keepdim=True)[0]) < -150).any())
    c = M.case("full_support_ties")
    r = M.reference(c)
    assert bool((c.x[0::4] == 0).all()) and bool((r["a"].v[0::4] == r["a"].v[0, 0]).all()) and bool((r["count"][0::4] == 37).all())
    r = M.reference(M.case("wide_support"))
    assert float(r["count"].min()) >= 200
    r = M.reference(M.case("lambda_high"))
    assert float(r["count"].max()) <= 3 and float(r["count"].max()) >= 2 and float((r["count"] > 0).double().mean()) > 0.5
    assert bool((M.case("negative_x").x < 0).any()) and not bool((M.case("R17").x < 0).any())
    for name in ("R1", "R17", "R2049", "n2047", "negative_x"):
        cnt = M.reference(M.case(name))["count"]
        assert 1 <= float(cnt.min()) and float(cnt.max()) <= 120 and 5 <= float(cnt.median()) <= 80, (name, cnt.min(), cnt.max())
    # near_threshold: the moved rows lie within 3 ulps of lam, on both sides
    c = M.case("near_threshold")
    a = M.reference(c)["a"].v[:M.N_FREE]
    ulp = 2.0 ** -32
    assert 2.0 ** -9 <= c.lam < 2.0 ** -8
    gap = torch.stack([row[(row - c.lam).abs().argmin()] - c.lam for row in a])
    assert bool((gap[0::2] > 0).all()) and bool((gap[1::2] < 0).all()) and bool((gap.abs() <= 3 * ulp).all())
    assert bool((c.dy[:M.N_FREE] == 0).all()) and bool((c.dy[M.N_FREE:] != 0).any())
    # live_c: c is a number, not noise
    r = M.reference(M.case("live_c"))
    assert float((r["crow"].v[:, 0].abs() > r["crow"].e[:, 0]).double().mean()) >= 0.5
