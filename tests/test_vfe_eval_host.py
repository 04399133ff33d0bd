"""The rounding bound of vfe_eval_cases.py proves itself on the CPU, over every row test_gpu_vfe_eval.py runs:

  * the float64 values the bound is drawn around agree with oracle.hvpr_oracle.pillar_vfe_scale and with fixture G1 to fp32
    round-off: the algebra is pinned;
  * the kernel's formulas in plain fp32 torch (one rounding per operation) are inside the bound on every element of every row; the
    used fraction and bound / largest element are reported per output;
  * the float64 reference with one mistake made is outside the bound on every element the mistake touches, on the row named for
    it, or on the share stated here with the elements that escape and why;
  * the rows and point-count sequences reach the edges they are in the tables for: the grid exponents, the floor, the pass plans
    of the restated window / pass rule, and (through the CPU voxelizer oracle) the sequences of point counts the clouds produce."""
import os

import numpy as np
import pytest
import torch

import vfe_eval_cases as V
from oracle import hvpr_oracle as O

_ROWS = {}


def _row(name):
    if name not in _ROWS:                # (computed once, never changed)
        c = V.case(name)
        _ROWS[name] = (c, V.reference(c))
    return _ROWS[name]


def _fold(lin_w, bn_w, bn_b, mean, var, eps=1e-3):
    """Eval-mode BatchNorm folded into the bias-free Linear in fp32, as the module does."""
    s = bn_w / np.sqrt(var + np.float32(eps))
    return torch.from_numpy((lin_w * s[:, None]).astype(np.float32)), torch.from_numpy((bn_b - mean * s).astype(np.float32))


def _folded_from(params):
    f = {}
    for key, (lin, bn) in {"0": ("pfn_layers.0.linear.weight", "pfn_layers.0.norm"), "1": ("pfn_layers.1.linear.weight", "pfn_layers.1.norm"),
                           "s0": ("pfn_scale_layers.0.0.weight", "pfn_scale_layers.0.1"),
                           "s1": ("pfn_scale_layers.1.0.weight", "pfn_scale_layers.1.1")}.items():
        f["w" + key], f["b" + key] = _fold(params[lin], params[bn + ".weight"], params[bn + ".bias"], params[bn + ".running_mean"],
                                           params[bn + ".running_var"])
    return f


def test_reference_agrees_with_the_oracle_and_fixture_g1(golden_dir, observed):
    """Fixture G1 (the reference module's own eval forward) and the oracle are fp32 computations with unfolded BatchNorm: the float64
    reference on the folded weights agrees with them to fp32 round-off of values of this size (1e-5 of the largest element)."""
    z = np.load(os.path.join(golden_dir, "g1_vfe.npz"))
    params = {k[6:]: z[k] for k in z.files if k.startswith("param.")}
    vs, rng = [0.16, 0.16, 3.0], [0.0, -19.84, -2.5, 47.36, 19.84, 0.5]
    vox, num, coords = (torch.from_numpy(np.asarray(z[k])) for k in ("voxels", "voxel_num_points", "voxel_coords"))
    c = V.Raw(vox, num, coords, _folded_from(params), vs, [vs[i] / 2 + rng[i] for i in range(3)])
    r = V.reference(c)
    tp = {k: torch.from_numpy(v) for k, v in params.items()}
    opf, osf, omask = O.pillar_vfe_scale(z["voxels"], z["voxel_num_points"].astype(np.float32), z["voxel_coords"].astype(np.float32), tp, vs, rng)
    for tag, pf, sf, mask in (("oracle", opf.numpy(), osf.numpy(), omask.numpy()),
                              ("G1", z["eval_pillar_features"], z["eval_pillar_scale_features"], z["eval_pillar_mask"])):
        for k, got in (("pillar", pf), ("scale", sf)):
            d = float((torch.from_numpy(got).double() - r[k].v).abs().max())
            top = float(r[k].v.abs().max())
            observed(f"vfe eval host: float64 reference against {tag} [{k}]: max |d| {d:.2e} of {top:.2e}")
            assert d <= 1e-5 * top, (tag, k, d, top)
        assert np.array_equal(mask.reshape(c.M, c.P), r["mask"].numpy())
    # and the fp32 stand-in is inside the bound on the fixture's pillars as well
    fr = V.fractions(*V.standin(c)[:2], r)
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("name", list(V.ROWS))
def test_fp32_standin_is_inside_the_bound(name, observed):
    c, r = _row(name)
    pf, sf, mask = V.standin(c)
    fr, sh = V.fractions(pf, sf, r), V.sharpness(r)
    observed(f"vfe eval host [{name}] M={c.M} P={c.P}: plain fp32 uses " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items())
             + " of the bound; bound / largest element " + ", ".join(f"{k} {v:.1e}" for k, v in sh.items()))
    assert max(fr.values()) <= 1.0, (name, fr)
    assert torch.equal(mask.double(), r["mask"])
    assert max(sh.values()) <= 1e-4, (name, sh)                     # the bound is a rounding bound, not a tolerance


# (wrong variant, output) -> the share of the touched elements that must be caught where that is not all of them, and which escape
STATED_SHARES = {
    # one element of the 355 touched: pillar 5, channel 15, where W1b . x_max of pillars 4 and 5 happen to differ by 1.4e-5, a quarter
    # of that element's bound of 6.1e-5 (the pillars are random neighbours: their x_max rows differ everywhere, but one of 64 weighted
    # sums of the differences may cancel); every other channel of pillar 5 is caught
    ("xmax_of_previous_pillar", "pillar"): 0.99,
}


@pytest.mark.parametrize("wrong", V.WRONG)
def test_a_wrong_variant_is_outside_the_bound(wrong, observed):
    name, outputs = V.WRONG_CASES[wrong]
    c, r = _row(name)
    bad = V.reference(c, wrong)
    shares = {}
    for k in outputs:
        touched = (bad[k].v - r[k].v).abs() > 1e-12 * r[k].v.abs().max()
        shares[k] = (V.caught_share(r[k], bad[k].v, touched), float(touched.double().mean()))
    observed(f"vfe eval host: {wrong} on [{name}]: " + ", ".join(f"{k} caught {s:.3f} of the {t:.2f} touched" for k, (s, t) in shares.items()))
    for k in outputs:
        assert shares[k][0] >= STATED_SHARES.get((wrong, k), 1.0), (wrong, name, shares)


def test_the_floor_rows_decide_from_the_reference_alone():
    c, r = _row("floor_decides")
    assert bool((c.num < c.P).all()) and bool((c.b0 > 0).sum() >= 6)
    assert int(r["pad_wins_xmax"].any(1).sum()) == c.M and int(r["pad_wins_xmax"].sum()) >= 6 * c.M      # several channels of every pillar
    assert int(r["pad_wins_out"].any(1).sum()) == c.M                                                     # the layer-1 max of every pillar
    f, rf = _row("floor_must_not_apply")
    assert bool((f.num == f.P).all()) and not bool(rf["pad_wins_xmax"].any()) and not bool(rf["pad_wins_out"].any())
    # the same content: the short row's live points are the full row's first points, under the same weights
    live = (torch.arange(c.P)[None, :] < c.num[:, None])[..., None]
    assert torch.equal(c.voxels, f.voxels * live) and torch.equal(c.coords, f.coords) and all(torch.equal(getattr(c, k), getattr(f, k)) for k in V.WEIGHTS)


def test_the_rows_reach_the_edges_they_claim():
    S = {k: (v["M"], v["P"]) for k, v in V.ROWS.items()}
    assert {p for _, p in S.values()} >= {1, 5, 20, 31, 32} and {m for m, _ in S.values()} >= {1, 2, 5, 8195}
    assert V.case("one_point_P32").num.tolist() == [1] and V.case("full_P32").num.tolist() == [32]
    assert V.case("one_beside_full").num.tolist() == [1, 32] and V.case("single_slot").num.tolist() == [1, 1, 1]
    # the launch arithmetic of hvpr_pillar_vfe_fwd_f32: min(ceil(M / 4), 2048) workgroups of four waves, a wave strides by their number
    blocks = lambda M: min(-(-M // 4), 2048)
    assert blocks(5) == 2 and blocks(8195) == 2048 and V.ROWS_WAVES == 8192 and 8195 - V.ROWS_WAVES == 3
    c = V.case("grid_stride")
    t = c.template
    assert c.voxels.numel() * 4 <= 4.3e6 and bool((t[:3] != t[V.ROWS_WAVES:]).any()) and int(c.num.min()) == 1 and int(c.num.max()) == 32
    # the fixed-point exponents: sum_scale restated
    b = lambda v: V.grid_k(torch.tensor([v], dtype=torch.float64)).item()
    assert [b(v) for v in (0.16, 0.5, 1.0, 31.9, 32.0, 47.4, 51.3, 63.9, 64.0)] == [49, 47, 46, 42, 41, 41, 41, 41, 40]
    k = V.case("kitti_corners")
    assert k.coords[0].tolist() == [0, 0, 0, 0] and k.coords[1].tolist() == [0, 0, 247, 295]
    d = V.case("dense_far_corner")
    assert d.coords[0].tolist() == [0, 0, 511, 511] and float(d.voxels[0, 0, 0]) > 51.0 and float(d.voxels[0, 0, 1]) > 51.0
    z = V.case("zero_coordinate")
    assert z.voxels[0, 0, :3].tolist() == [0.0, 0.0, 0.0] and z.coords[0].tolist() == [0, 0, 124, 0]
    tz = V.case("tiny_z")
    lv = torch.arange(tz.P)[None, :] < tz.num[:, None]
    assert float(tz.voxels[..., 2].abs().max()) < 2.0 ** -20 and float(tz.voxels[..., 2][lv].abs().min()) > 0
    ng = V.case("all_negative")
    lv = torch.arange(ng.P)[None, :] < ng.num[:, None]
    assert bool((ng.voxels[..., :3][lv] < 0).all())
    idt = V.case("identical_points")
    assert bool((idt.voxels == idt.voxels[:, :1]).all()) and bool((idt.num == 32).all())
    bd = V.case("cell_borders")
    G = V.GRIDS["kitti"]
    lo = (torch.tensor(G["lo"], dtype=torch.float64) + bd.coords[:, [3, 2, 1]].double() * torch.tensor(G["vs"], dtype=torch.float64)).float()
    assert bool(((bd.voxels[:, 0, 0] == lo[:, 0]) & (bd.voxels[:, 0, 1] > lo[:, 1])).all())
    md = V.case("m_device_below_M")
    assert md.m_device == 5 < md.M


def test_the_pass_plans_of_the_sequences():
    assert set(V.SEQUENCES) == set(V.PLANS)
    for name, s in V.SEQUENCES.items():
        counts = [n for f in s["frames"] for n in f]
        assert V.pass_plan(counts, s["P"]) == V.PLANS[name], (name, V.pass_plan(counts, s["P"]))
    assert V.K_WIN == 28 and V.K_PASS == 32
    # the rule's corners: a pillar that starts on the last owned position is this window's, one position later the next one's
    assert V.pass_plan([27, 5], 32) == [(0, [0, 1])] and V.pass_plan([28, 4], 32) == [(0, [0]), (1, [1])]
    assert V.pass_plan([27, 6], 32) == [(0, [0]), (0, [1])]


@pytest.mark.parametrize("interleave", [False, True])
def test_the_clouds_produce_their_sequences(interleave):
    """Through the CPU voxelizer oracle: the voxels of every frame, in order, hold min(count, P) points."""
    for name, s in V.SEQUENCES.items():
        pts, offs = V.clouds(s["frames"], seed=3, interleave=interleave)
        G = V.GRIDS["kitti"]
        rng = list(G["lo"]) + [G["lo"][i] + G["vs"][i] * n for i, n in enumerate((G["nx"], G["ny"], 1))]
        for b, counts in enumerate(s["frames"]):
            f = pts[offs[b]:offs[b + 1]]
            assert bool((f[:, 0] == b).all())
            v, cds, n = O.voxelize(f[:, 1:], list(G["vs"]), rng, s["P"], 40000)
            assert n.tolist() == [min(k, s["P"]) for k in counts], (name, b, n.tolist())
    pts, offs, cap, live = V.capped_cloud()
    v, cds, n = O.voxelize(pts[:, 1:], list(G["vs"]), rng, 32, cap, mode="v1")
    assert n.tolist() == live
    v2, _, n2 = O.voxelize(pts[:, 1:], list(G["vs"]), rng, 32, 40000)
    assert n2.tolist() == [7, 3, 2]
