"""The rounding bound of gate_train_cases.py proves itself on the CPU, over every row test_gpu_gate_train.py runs:

  * the kernels' formulas in fp32 torch (partial sums in the kernels' lane / wave / tile structure, the finalising in double) are
    inside the bound on every element of every output, and the values the bound is drawn around agree with torch autograd of the
    formula in float64;
  * the float64 reference with one mistake made — ties to the highest index, the mean over C - 1, edge clamping for zero padding,
    unflipped transposed-convolution taps, a dense term of da dropped, the last tile column or the pixels past 2048 * 1024 lost — and
    the fp32 form that takes its statistics after the bias are outside it on every element the mistake touches;
  * the rows reach the loop edges they are in the table for, by the restated launch arithmetic."""
import pytest
import torch

import gate_train_cases as G


def _check(c, observed):
    r = G.reference(c)
    s = G.standin(c)
    assert torch.equal(s["argmax"], r["argmax"])
    fr = G.fractions(s, r)
    worst = max(fr, key=fr.get)
    observed(f"gate train host [{c.name}]: fp32 stand-in uses at most {fr[worst]:.4f} of the bound ({worst})")
    assert fr[worst] <= 1.0, (c.name, fr)
    return r


@pytest.mark.parametrize("name", list(G.ROWS))
def test_fp32_standin_is_inside_the_bound_everywhere(name, observed):
    c = G.case(name)
    r = _check(c, observed)
    if c.content != "constant":                    # (autograd of sqrt(var + eps) is fine at var = 0, but var itself is 1e-33 noise there)
        want = G.autograd64(c)
        for k, v in want.items():
            scale = float(v.abs().max()) + 1e-30
            assert float((r[k].v.reshape(v.shape) - v).abs().max()) <= 1e-9 * max(scale, 1e-3), (name, k)


@pytest.mark.parametrize("name", list(G.LARGE))
def test_fp32_standin_is_inside_the_bound_on_the_large_row(name, observed):
    _check(G.case(name), observed)


def test_exact_zero_rows():
    """gamma = 0: dy, dW, dbias have value and bound exactly 0.  dgate = 0: every gradient has.  The constant field: variance exactly 0."""
    r = G.reference(G.case("gamma_zero"))
    for k in ("dy", "dw18", "dbias"):
        assert float(r[k].v.abs().max()) == 0.0 and float(r[k].e.max()) == 0.0, k
    assert float(r["dgamma"].v.abs()) > 0
    r = G.reference(G.case("dgate_zero"))
    for k in ("dy", "dw18", "dbias", "dgamma", "dbeta"):
        assert float(r[k].v.abs().max()) == 0.0 and float(r[k].e.max()) == 0.0, k
    for name in ("constant_field", "one_pixel"):
        r = G.reference(G.case(name))
        assert float(r["stats"].v[1]) <= 1e-30 and abs(float(r["stats"].v[2]) - float(torch.tensor(G.EPS).float().double()) ** -0.5) < 1e-9
    r = G.reference(G.case("bias_300"))
    # u |bias| on a, not on var: u bias^2 = 5e-3 would be 1e-2 of this variance
    assert float(r["a"].e.min()) >= G.U * 299.0 and float(r["stats"].e[1] / r["stats"].v[1]) < 1e-4


@pytest.mark.parametrize("wrong", G.WRONG)
def test_a_wrong_variant_is_outside_the_bound(wrong, observed):
    kw, outputs = G.WRONG_CASES[wrong]
    c = G.Case(**kw)
    r, bad = G.reference(c), G.reference(c, wrong)
    if c.P < 100000:
        assert max(G.fractions(G.standin(c), r).values()) <= 1.0          # the inputs built for it are fair
    for k in outputs:
        touched = bad[k].v != r[k].v
        if wrong in ("ties_to_highest", "edge_clamped_padding", "mean_over_c_minus_1"):
            # the tie pixels' two channels; the border pixels; the mean plane of the pixels that are not all zero
            assert 0.0 < float(touched.double().mean()) < 1.0, (wrong, k)
        else:
            assert bool(touched.all()), (wrong, k, float(touched.double().mean()))
        share = G.caught_share(r[k], bad[k].v, touched)
        if (wrong, k) == ("dgamma_term_dropped", "dy"):
            # the dropped term, xhat dgamma / n spread by the nine taps, changes sign across the image with xhat: on the few pixels
            # next to a zero crossing it is smaller than the rounding bound (0.4 % of them here); dW sums it and is caught whole
            assert share >= 0.99, (wrong, k, share)
            continue
        assert share == 1.0, (wrong, k, share)
    if wrong == "ties_to_highest":
        assert not torch.equal(bad["argmax"], r["argmax"])
    observed(f"gate train host: {wrong} is outside the bound on every touched element of {', '.join(outputs)}")


def test_statistics_after_the_bias_in_fp32_are_outside_the_bound(observed):
    """The float64 value of the variance does not depend on where the bias is added; its fp32 partial sums do.  With bias 300 the
    fp32 form that squares conv + bias misses the variance and invstd bounds that the kernel's order keeps."""
    c = G.case("bias_300")
    r = G.reference(c)
    good, bad = G.fractions(G.standin(c), r), G.fractions(G.standin(c, "bias_in_fp32_squares"), r)
    observed(f"gate train host: statistics after the bias: var at {bad['var']:.1f}, invstd at {bad['invstd']:.1f} of the bound "
             f"(before it: {good['var']:.4f}, {good['invstd']:.4f})")
    assert good["var"] <= 1.0 and good["invstd"] <= 1.0 and bad["var"] > 1.0 and bad["invstd"] > 1.0


def test_the_rows_reach_the_loop_edges_they_claim():
    S = {k: (v["N"], v["H"], v["W"], v["C"]) for k, v in G.ALL.items()}
    P = {k: v[0] * v[1] * v[2] for k, v in S.items()}
    tiles = {k: G.n_tiles(*v[:3]) for k, v in S.items()}
    assert S["one_pixel"] == (1, 1, 1, 4) and G.pool_trips(4) == 1
    assert S["one_row"][1] == 1 and S["one_column"][2] == 1 and tiles["one_row"] == 3 == tiles["one_column"]
    assert tiles["one_tile"] == 1 and S["one_tile"][3] // 4 == 3 and tiles["one_past_a_tile"] == 4
    n, h, w, ch = S["ragged_tiles_two_trips"]
    assert ch // 4 == 9 and G.pool_trips(ch) == 2 and h % G.GT and w % G.GT and n > 1 and G.pool_k(ch) == 9
    assert P["pixels_not_by_32"] % 32 != 0 and G.pool_trips(128) == 4 and G.pool_trips(512) == 16 and S["widest"][1:3] == (3, 3)
    assert P["one_red_block"] == 2048 and G.red_blocks(2048) == 1 and P["two_red_blocks"] == 2049 and G.red_blocks(2049) == 2
    assert tiles["tiles_256"] == 256 and G.final_trips(256) == 1 and tiles["tiles_257"] == 257 and G.final_trips(257) == 2
    assert tiles["tiles_300_three_images"] == 300 and S["tiles_300_three_images"][0] == 3
    big = P["past_the_reduction_grid"]
    assert 2048 * 1024 < big < 2048 * 1024 + 2048 and G.red_blocks(big) == 1024 and G.red_trips(big) == 9 and G.red_trips(2048 * 1024) == 8
    assert big - 1448 <= 2048 * 1024                                   # one image row fewer would not get there
    assert big * 4 * 4 <= 34 * 2 ** 20
    assert all(G.red_trips(p) <= 8 for k, p in P.items() if k != "past_the_reduction_grid")
    # contents
    c = G.case("one_tile")
    top = c.y.view(-1, 12)[0::3]
    assert bool((top[:, 1] == top.max(1)[0]).all()) and bool((top[:, 1] == top[:, 9]).all()) and (1 // 4) % 8 != (9 // 4) % 8
    c = G.case("ragged_tiles_two_trips")
    top = c.y.view(-1, 36)[0::3]
    assert bool((top[:, 2] == top.max(1)[0]).all()) and bool((top[:, 2] == top[:, 34]).all()) and (2 // 4) % 8 == (34 // 4) % 8 == 0
    assert bool((G.reference(c)["argmax"].view(-1)[0::3] == 2).all())
    c = G.case("wide")
    assert bool((c.y.view(-1, 128)[0::2] < 0).all())
    for name in G.ROWS:
        c = G.case(name)
        if c.content is None and c.P > 30:
            assert bool((c.y.view(c.P, -1) == 0).all(1).any()), name          # whole-zero pixels: every channel ties
    assert G.workspace_bytes(1, 16, 16) == (19 + 2048) * 4 // 256 * 256 + 256 + 1024 + 256
