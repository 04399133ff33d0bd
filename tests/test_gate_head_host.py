"""The bounds of gate_head_cases.py prove themselves on the CPU, over every row test_gpu_gate_head.py runs:

  * the kernels' formulas in plain fp32 (one rounding per operation) are inside the bound on every element, and equal bit for bit
    where the reference is exact (the class copy, box 6 with direction bins, the labels);
  * the float64 gate agrees with oracle.hvpr_oracle.spatial_gate: the algebra is pinned;
  * the reference with one mistake made is outside the bound — or, where the output is exact, different — on every element the
    mistake touches, on the rows named for it;
  * the np.float32 heading restatement equals the float64 formula away from the floor's jumps, the table holds headings within an
    ulp of a multiple of the period on both sides, and a fused multiply-subtract changes a stated share of the table's headings;
  * no label of the table is undecided, from the reference alone."""
import numpy as np
import pytest
import torch

import gate_head_cases as G
from oracle import hvpr_oracle as O

_GATE, _HEAD = {}, {}


def _gate(name):
    if name not in _GATE:
        c = G.gate_case(name)
        _GATE[name] = (c, G.gate_reference(c))
    return _GATE[name]


def _head(name):
    if name not in _HEAD:
        c = G.head_case(name)
        _HEAD[name] = (c, G.head_reference(c))
    return _HEAD[name]


# ------------------------------------------------------------------------------------------------ gate
@pytest.mark.parametrize("name", list(G.GATE_ROWS))
def test_gate_fp32_standin_is_inside_the_bound(name, observed):
    c, r = _gate(name)
    got = G.gate_standin(c)
    fr = G.used_fraction(got, r["gate"])
    sharp = float((r["gate"].e / r["gate"].v.abs().clamp_min(G.TINY)).max())
    observed(f"gate host [{name}]: plain fp32 uses {fr:.4f} of the bound; largest bound / value {sharp:.1e}")
    assert fr <= 1.0, (name, fr)
    if c.content == "zero_w":
        assert float(r["gate"].v.max() - r["gate"].v.min()) == 0.0                  # a constant gate
    if c.content == "negative":
        assert float(c.y.max()) < 0 and float(r["pooled"].v[..., 0].max()) < 0      # the max is below the padding's 0
    if c.content in ("bias_plus", "bias_minus"):
        assert float((r["gate"].v - 0.5).abs().min()) > 0.499                       # saturated
    if c.content == "spike":
        assert float(r["pooled"].v[..., 0].min()) == 1e4 and abs(float(r["pooled"].v[..., 1].mean()) - (1.0 + 9999.0 / c.C)) < 1e-6


def test_gate_reference_agrees_with_the_oracle():
    c, r = _gate("1x17x33x36")
    s, t, eps = 1.3, -0.2, 1e-3
    params = {"attention.spatial.conv.weight": c.w18.view(1, 2, 3, 3), "attention.spatial.conv.bias": torch.tensor([c.conv_bias]),
              "attention.spatial.norm.weight": torch.tensor([c.bn_scale]), "attention.spatial.norm.bias": torch.tensor([c.bn_shift]),
              "attention.spatial.norm.running_mean": torch.zeros(1), "attention.spatial.norm.running_var": torch.full((1,), 1.0 - eps)}
    ref = O.spatial_gate(c.y.permute(0, 3, 1, 2), params)[:, 0]
    assert float((ref.double() - r["gate"].v).abs().max()) <= 1e-5


GATE_STATED = {}


@pytest.mark.parametrize("wrong", G.GATE_WRONG)
def test_gate_wrong_variant_is_outside_the_bound(wrong, observed):
    for name in G.GATE_WRONG_CASES[wrong]:
        c, r = _gate(name)
        bad = G.gate_reference(c, wrong)["gate"].v
        touched = ~((bad - r["gate"].v).abs() <= 1e-12)                             # (a NaN is touched)
        share = G.caught_share(r["gate"], bad, touched)
        observed(f"gate host: {wrong} on [{name}]: caught {share:.3f} of the {float(touched.double().mean()):.2f} touched")
        assert share >= GATE_STATED.get((wrong, name), 1.0), (wrong, name, share)


def test_gate_rows_reach_the_edges_they_claim():
    shapes = {(v["N"], v["H"], v["W"], v["C"]) for v in G.GATE_ROWS.values()}
    assert shapes == set(G.GATE_SHAPES)
    by_content = {}
    for v in G.GATE_ROWS.values():
        by_content.setdefault(v.get("content"), set()).add((v["N"], v["H"], v["W"], v["C"]))
    assert all(len(by_content[k]) >= 2 for k in ("negative", "spike", "bias_plus", "bias_minus", "neg_scale", "zero_w"))
    assert len(by_content["bias_plus"] | by_content["bias_minus"]) >= 2
    assert [G.pool_k(c) for c in (4, 8, 32, 36, 128, 260)] == [6, 6, 6, 9, 15, 30]                 # 1, 1, 1, 2, 4, 9 trips of a lane
    assert G.gate_case("1x17x33x36_neg_scale").bn_scale < 0 and G.gate_case("2x16x16x32_bias_plus").conv_bias == 30.0


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", list(G.HEAD_ROWS))
def test_head_fp32_standin_is_inside_the_bound(name, observed):
    c, r = _head(name)
    cls, box, score, label = G.head_standin(c)
    fr = G.head_fractions(box, score, r)
    observed(f"head decode host [{name}]: plain fp32 uses " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()) + " of the bound")
    assert max(fr.values()) <= 1.0, (name, fr)
    assert torch.equal(cls, r["cls"]) and torch.equal(label, r["label"])
    assert not bool(r["undecided"].any()), (name, int(r["undecided"].sum()))
    if c.nbins > 0:
        assert torch.equal(box[..., 6].double(), r["box"].v[..., 6]) and float(r["box"].e[..., 6].max()) == 0.0


def test_head_rows_reach_the_edges_they_claim():
    R = G.HEAD_ROWS
    assert R["one_anchor_no_bins"] == (1, 1, 1, 1, 1, 0) and R["one_pixel"] == (1, 1, 1, 2, 1, 2) and R["three_classes"] == (2, 3, 5, 6, 3, 2)
    assert R["odd_image"] == (1, 7, 9, 2, 1, 2) and R["one_workgroup"] == (1, 16, 8, 2, 1, 2) and 16 * 8 * 2 == 256
    assert R["one_pixel_row_more"] == (1, 17, 8, 2, 1, 2) and R["three_bins"][5] == 3
    c, r = _head("three_classes")
    cls = c.parts()[0]
    assert float(cls[0, 0]) == float(cls[0, 1]) and float(cls[1, 1]) == float(cls[1, 2]) and cls[2, :2].tolist() == [30.0, 100.0]
    assert cls[3, :2].tolist() == [100.0, 30.0] and r["label"].view(-1)[:4].tolist() == [1, 2, 1, 1]
    sg = 1.0 / (1.0 + np.exp(-np.asarray([30.0, 100.0], np.float32)))
    assert sg.dtype == np.float32 and sg.tolist() == [1.0, 1.0]                               # both saturate to 1.0f
    flat = cls.reshape(-1)
    assert {30.0, -30.0, 100.0, -100.0} <= set(flat.tolist())
    box, dirs = c.parts()[1], c.parts()[2]
    assert float(box[:, 3:6].max()) == 20.0 and float(box[:, 3:6].min()) == -20.0 and float(box[:, :3].abs().max()) <= 3.0
    assert int((dirs[:, 0] == dirs[:, 1]).sum()) >= 10                                        # tied direction logits


def test_heading_restatement_and_its_table():
    """heading32 equals the float64 formula away from the floor's jumps; the table has headings within an ulp of a multiple of the
    period on both sides; a fused multiply-subtract changes a stated share of the headings."""
    changed = {}
    for name in ("one_pixel_row_more", "three_classes", "three_bins"):
        c, _ = _head(name)
        cls, box, dirs, xa, ya, an = (t.numpy() for t in c.parts())
        h32, v, dl = G.heading32(box[:, 6], an[:, 4], dirs, c.dir_offset, c.dir_limit_offset, c.period)
        h64, dist = G.heading64(box[:, 6], an[:, 4], dirs, c.dir_offset, c.dir_limit_offset, c.period)
        away = dist > 1e-5
        assert away.sum() >= 6 and float(np.abs(h32[away] - h64[away]).max()) <= 4 * 2.0 ** -23 * 16.0
        per = np.float64(np.float32(c.period))
        k = np.round(v.astype(np.float64) / per)
        off_by = v.astype(np.float64) - k * per
        ulp = np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
        near = c.near.numpy()
        assert near.sum() >= 12 and bool((np.abs(off_by[near]) <= 2 * ulp[near] + 1e-12).all())
        assert (off_by[near] < 0).sum() >= 2 and (off_by[near] >= 0).sum() >= 2, name        # both sides of the jump
        fused, _, _ = G.heading32(box[:, 6], an[:, 4], dirs, c.dir_offset, c.dir_limit_offset, c.period, fused=True)
        changed[name] = float((fused != h32).mean())
        tied = dirs[:, 0] == dirs.max(1)
        assert bool((dl[(dirs == dirs[:, :1]).all(1)] == 0).all()) and tied.any()
    # the kernel's comment: a fused multiply-subtract differs in the last bit for a share of the headings
    # (stated: at least one heading in twenty on the two rows with 180 and 272 anchors; the 24 anchors of three_bins hold few turns)
    assert changed["one_pixel_row_more"] >= 0.05 and changed["three_classes"] >= 0.05, changed


HEAD_STATED = {}


@pytest.mark.parametrize("wrong", G.HEAD_WRONG)
def test_head_wrong_variant_is_caught(wrong, observed):
    name = G.HEAD_WRONG_CASES[wrong]
    c, r = _head(name)
    bad = G.head_reference(c, wrong)
    report = {}
    if wrong == "labels_zero_based":
        assert bool((bad["label"] != r["label"]).all())
        report["label"] = 1.0
    elif wrong in ("dir_tie_takes_last", "period_fused"):
        d = bad["box"].v[..., 6] != r["box"].v[..., 6]
        dirs = c.parts()[2]
        tied = (dirs == dirs[:, :1]).all(1).view(d.shape)
        if wrong == "dir_tie_takes_last":                   # every tied anchor moves by a period, no other
            assert torch.equal(d, tied) and bool(tied.any())
        else:
            assert float(d.double().mean()) >= 0.05
        report["box6 changed"] = float(d.double().mean())
    else:
        for k in ("box", "score"):
            touched = (bad[k].v - r[k].v).abs() > 1e-12
            if bool(touched.any()):
                report[k] = G.caught_share(r[k], bad[k].v, touched)
        if wrong == "anchor_major_order":
            assert not torch.equal(bad["cls"], r["cls"]) and "score" in report
        assert "box" in report
        for k, s in report.items():
            assert s >= HEAD_STATED.get((wrong, k), 1.0), (wrong, report)
    observed(f"head decode host: {wrong} on [{name}]: " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))
