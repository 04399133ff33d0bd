"""The rounding bound of conv_wino_cases.py proves itself on the CPU, over every row test_gpu_conv_wino_bound.py runs:

  * the float64 Winograd form the bound is built on equals float64 conv2d / autograd to 1e-10 of the output scale;
  * a plain-torch fp32 stand-in with the kernels' summation structure (fp32 transforms, one sum per tile, the tiles of a chunk in
    order, the chunks in the reducer's four-accumulator order) is inside the bound on every element;
  * the float64 value with something lost is outside it: a pixel tile, a split-K chunk, four channels of a tile, the reducer's signs
    and the adjoint pack's flip on at least DETECT_SHARE of the elements they touch (rows of DETECT), a single block term on at least
    SINGLE_SHARE for every chain up to SINGLE_BLOCK_MAX_CHAIN;
  * the tables reach every class of shape they were written for, so that an edit cannot silently lose one."""
import pytest

import conv_wino_cases as C

FAMILIES = C.families()
ROWS = [(name, i) for name in sorted(FAMILIES) for i in range(len(FAMILIES[name]))]


def _share(op, ref, S, drop):
    bad, S_bad = op.reference(drop)
    m = op.live()
    return C.caught_share(ref[m], S[m], bad[m], S_bad[m], op.K)


@pytest.mark.parametrize("family,i", ROWS, ids=[f"{n}-{FAMILIES[n][i].dims}" for n, i in ROWS])
def test_row_standin_inside_and_corruptions_outside_the_bound(family, i, observed):
    op = FAMILIES[family][i]
    wgrad = isinstance(op, C.WgradWino)
    ref, S = op.reference()
    direct = op.direct_reference()
    agree = float((ref - direct).abs().max() / direct.abs().max())
    assert agree <= 1e-10, (op.dims, agree)
    frac = C.used_fraction(op.standin(), ref, S, op.K)
    assert frac <= 1.0, (op.dims, frac)
    shares = {}
    if wgrad:
        chain = C.BLOCKS * op.geo["tiles_max"]
        shares["single"] = _share(op, ref, S, "single")
        if chain <= C.SINGLE_BLOCK_MAX_CHAIN or op.dims not in C.SINGLE_BLOCK_EXEMPT[family]:
            assert shares["single"] >= C.SINGLE_SHARE, (op.dims, chain, shares)
        if op.dims in C.DETECT:
            for drop in ("tile", "chunk", "co_group", "ci_group", "sign"):
                shares[drop] = _share(op, ref, S, drop)
                assert shares[drop] >= C.DETECT_SHARE, (op.dims, drop, shares)
        op._cache.clear()                 # (the transformed operands of the larger rows are hundreds of megabytes)
    else:
        for drop in ("group", "flip") if op.adjoint else ("group",):
            shares[drop] = _share(op, ref, S, drop)
            assert shares[drop] >= C.DETECT_SHARE, (op.dims, drop, shares)
        shares["single"] = _share(op, ref, S, "single")
        assert shares["single"] >= C.SINGLE_SHARE, (op.dims, shares)
    observed(f"conv wino host [{family}] {op.dims} n = {op.n}: fp32 stand-in uses {frac:.4f} of the bound, float64 forms agree to {agree:.1e}; "
             "caught " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))


def test_wgrad_pipe_reaches_every_depth_of_the_pipeline():
    geo = [C.geometry(r) for r in C.WGRAD_PIPE]
    depth = {g["tiles_max"] for g in geo}
    assert {1, 2, 3, 4} <= depth and max(depth) >= 5
    # workgroups one tile short of the others: "past the end" zero loads right after a real tile
    uneven = {g["tiles_max"] for g in geo if g["tiles_min"] == g["tiles_max"] - 1 and g["tiles_min"] >= 1}
    assert {2, 3, 4} <= uneven
    assert any(r[0] >= 3 and g["crosses_images"] and g["tiles_max"] >= 2 for r, g in zip(C.WGRAD_PIPE, geo))
    # the backbone's 16 output tiles on 16 chunks, and 4 output tiles on 64 chunks with some workgroups walking two tiles
    assert any((g["n_ot"], g["n_chunks"]) == (16, 16) for g in geo)
    assert any((g["n_ot"], g["n_chunks"], g["tiles_min"], g["tiles_max"]) == (4, 64, 1, 2) for g in geo)
    assert any(r in C.WGRAD_SPARSE for r in C.WGRAD_PIPE)
    for g in geo:
        assert g["n_chunks"] == min(-(-256 // g["n_ot"]), g["n_pt"])


def test_wgrad_edge_reaches_every_class():
    rows, geo = C.WGRAD_EDGE, [C.geometry(r) for r in C.WGRAD_EDGE]
    for k in (3, 4):                          # cin, then cout
        chans = {r[k] for r in rows}
        assert chans <= {4, 24, 68, 132}
        assert any(c < 64 and c % 64 for c in chans), "a dead channel group inside the only tile"
        assert {-(-c // 64) for c in chans if c > 64 and c % 64} == {2, 3}, "two and three tiles with the last partly live"
        assert 4 in chans
    assert {1, 7, 9} <= {r[1] for r in rows} and {1, 15, 17, 31, 33} <= {r[2] for r in rows}
    assert any(r[1] == 1 and r[2] == 1 for r in rows)
    assert {1, 2, 3} <= {g["n_chunks"] % 4 for g in geo}
    mod8 = {g["grid_mod8"] == 0 for g in geo}
    assert mod8 == {True, False}, "the XCD remap and its fall-through"
    assert any(r in C.WGRAD_SPARSE for r in rows)
    assert all(g["tiles_max"] == 1 for g in geo)          # (the pipeline's depth is WGRAD_PIPE's business)


def test_forward_tables_reach_every_class():
    for r in C.DGRAD_WINO:
        N, H, W, cin_w, cout_w = r
        assert cout_w % 8 == 0 and cin_w % 4 == 0, "the Winograd kernel must take it (conv_train._winograd)"
        assert cin_w % 64 != 0 and (H % C.TH or W % C.TW)
        assert r in C.DGRAD_SFM or cin_w != cout_w
    assert C.DGRAD_SFM <= set(C.DGRAD_WINO) and len(C.DGRAD_SFM) == 1
    assert set(C.DGRAD_PAIRS) == set(C.DGRAD_WINO) and set(C.DGRAD_PAIRS.values()) == {True, False}
    assert any(r[3] > 128 for r in C.DGRAD_WINO), "more than one output channel tile"
    assert any(r in C.DGRAD_SPARSE for r in C.DGRAD_WINO) and any(r in C.FWD_SPARSE for r in C.FWD_TRAIN)
    # the forward rows are the data-gradient rows' shapes seen as forward layers
    assert {(r[0], r[1], r[2], r[4], r[3]) for r in C.DGRAD_WINO if r not in C.DGRAD_SFM} <= set(C.FWD_TRAIN)


def test_detect_rows_are_one_of_each_kind():
    every = set(C.WGRAD_PIPE) | set(C.WGRAD_EDGE)
    assert set(C.DETECT) <= every
    geo = {r: C.geometry(r) for r in C.DETECT}
    assert any(g["tiles_max"] == 1 for g in geo.values()) and any(g["tiles_min"] >= 3 for g in geo.values())
    assert any(r[3] % 64 and r[4] % 64 for r in C.DETECT), "ragged channels"
    assert any(r[1] % C.TH and r[2] % C.TW for r in C.DETECT), "ragged image"
    assert any(r in C.WGRAD_SPARSE for r in C.DETECT)


def test_single_block_exemptions_are_named_and_at_most_one_a_family():
    for family, exempt in C.SINGLE_BLOCK_EXEMPT.items():
        rows = {op.dims for op in FAMILIES[family]}
        assert exempt <= rows and len(exempt) <= 1
        for r in exempt:
            assert C.BLOCKS * C.geometry(r)["tiles_max"] > C.SINGLE_BLOCK_MAX_CHAIN
    assert C.SINGLE_BLOCK_MAX_CHAIN == C.BLOCKS * max(C.geometry(r)["tiles_max"] for r in C.WGRAD_PIPE)


def test_rounding_counts():
    """n of the docstring on the shapes named there, and the chunk function on the workload's levels."""
    assert C.wgrad_roundings(1, 1) == 64 + 0 + 1 + 10 and C.wgrad_roundings(5, 16) == 320 + 4 + 0 + 10
    assert C.wgrad_roundings(1, 7) == 64 + 1 + 3 + 10            # the three remainder chunks all go to s0
    assert C.ww_chunks(2, 248, 296, 128, 128) == 64 and C.ww_chunks(2, 62, 74, 512, 512) == 4 and C.ww_chunks(1, 8, 8, 64, 64) == 1
    assert C.wgrad_fits(1, 1 << 27, 4, 4) is False and C.wgrad_fits(1, (1 << 27) - 1, 4, 4) is True
