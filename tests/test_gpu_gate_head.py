"""hvpr_spatial_gate_f32 and hvpr_head_decode_f32 (csrc/postprocess.hip) against float64, element by element inside the derived
rounding bounds of gate_head_cases.py: no tolerance added, no element excluded; the class copy, box 6 with direction bins and the
labels bit for bit.  test_gate_head_host.py shows on the CPU what the bounds admit and what they catch.  The references are computed
on the device in float64 from the same fp32 words.  Every output lies inside a larger sentinel buffer.  Every test reports
max(err / bound) under "observed margins"."""
import pytest
import torch

import gate_head_cases as G
from hvpr_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED = 0, -1, -2                          # include/hvpr_amd.h hvpr_status
SENTINEL, GUARD = G.SENTINEL, 256


# ------------------------------------------------------------------------------------------------ gate
def _gate_call(c, out, C=None, y=None):
    from hvpr_amd._lib import lib
    return lib().hvpr_spatial_gate_f32((c.y if y is None else y).data_ptr(), c.N, c.H, c.W, c.C if C is None else C, c.w18.data_ptr(),
                                       c.conv_bias, c.bn_scale, c.bn_shift, out.data_ptr(), kernels._stream())


@pytest.mark.parametrize("name", list(G.GATE_ROWS))
def test_gate_row_within_the_bound(name, observed):
    c = G.gate_case(name).to(DEV)
    r = G.gate_reference(c)
    n = c.N * c.H * c.W
    out = torch.full((n + GUARD,), SENTINEL, device=DEV)
    assert _gate_call(c, out) == OK
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()), (name, "wrote past its end")
    got = out[:n].view(c.N, c.H, c.W)
    assert torch.equal(got, kernels.spatial_gate(c.y, c.w18, c.conv_bias, c.bn_scale, c.bn_shift))
    fr = G.used_fraction(got, r["gate"])
    observed(f"gate [{name}]: max err / bound {fr:.4f}")
    assert fr <= 1.0, (name, fr)
    if c.content == "zero_w":
        assert float(got.max()) == float(got.min())


@pytest.mark.parametrize("C,status", [(6, UNSUPPORTED), (2, INVALID)])
def test_gate_refuses(C, status):
    c = G.gate_case("2x16x16x32").to(DEV)
    out = torch.full((c.N * c.H * c.W + GUARD,), SENTINEL, device=DEV)
    assert _gate_call(c, out, C=C) == status
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ decode
def _head_buffers(c):
    A = c.N * c.H * c.W * c.na
    return {"cls": torch.full((A * c.nc + GUARD,), SENTINEL, device=DEV), "box": torch.full((A * 7 + GUARD,), SENTINEL, device=DEV),
            "score": torch.full((A + GUARD,), SENTINEL, device=DEV), "label": torch.full((A + GUARD,), -7, dtype=torch.int32, device=DEV)}


def _head_call(c, b, CH=None, na=None, null=None, want_cls=True, want_scores=True):
    from hvpr_amd._lib import lib
    ptr = lambda name, t: None if name == null else t.data_ptr()
    return lib().hvpr_head_decode_f32(c.head.data_ptr(), c.N, c.H, c.W, c.CH if CH is None else CH, c.na if na is None else na, c.nc, c.nbins,
                                      c.x_shifts.data_ptr(), c.y_shifts.data_ptr(), c.anchor_table.data_ptr(), c.dir_offset,
                                      c.dir_limit_offset, c.period, ptr("cls", b["cls"]) if want_cls else None, ptr("box", b["box"]),
                                      ptr("score", b["score"]) if want_scores else None, ptr("label", b["label"]) if want_scores else None,
                                      kernels._stream())


def _intact(t):
    return bool((t == (-7 if t.dtype == torch.int32 else SENTINEL)).all())


@pytest.mark.parametrize("name", list(G.HEAD_ROWS))
def test_head_row_within_the_bound(name, observed):
    c = G.head_case(name).to(DEV)
    r = G.head_reference(c)
    assert not bool(r["undecided"].any())                   # from the reference alone: every label is decided or planted
    N, A = c.N, c.H * c.W * c.na
    b = _head_buffers(c)
    assert _head_call(c, b) == OK
    torch.cuda.synchronize()
    sizes = {"cls": N * A * c.nc, "box": N * A * 7, "score": N * A, "label": N * A}
    for k, n in sizes.items():
        assert _intact(b[k][n:]), (name, k, "wrote past its end")
    cls, box = b["cls"][:sizes["cls"]].view(N, A, c.nc), b["box"][:sizes["box"]].view(N, A, 7)
    score, label = b["score"][:N * A].view(N, A), b["label"][:N * A].view(N, A)
    assert torch.equal(cls, r["cls"]), name
    fr = G.head_fractions(box, score, r)
    cols = {i: G.used_fraction(box[..., i], r["box"][..., i]) for i in range(7)}
    observed(f"head decode [{name}]: max err / bound box {fr['box']:.4f} (columns " + " ".join(f"{v:.3f}" for v in cols.values())
             + f"), score {fr['score']:.4f}")
    assert max(fr.values()) <= 1.0, (name, fr, cols)
    if c.nbins > 0:                                          # zero bound: bit for bit against the np.float32 restatement
        assert torch.equal(box[..., 6].double(), r["box"].v[..., 6]), name
    assert torch.equal(label.long(), r["label"]), name
    # the wrapper gives the same, and the boxes do not depend on the optional outputs
    wc, wb, ws, wl = kernels.head_decode(c.head, c.na, c.nc, c.nbins, c.x_shifts, c.y_shifts, c.anchor_table, c.dir_offset, c.dir_limit_offset,
                                         c.period)
    assert torch.equal(wc, cls) and torch.equal(wb, box) and torch.equal(ws, score) and torch.equal(wl, label)
    for want_cls, want_scores in ((False, True), (True, False), (False, False)):
        b2 = _head_buffers(c)
        assert _head_call(c, b2, want_cls=want_cls, want_scores=want_scores) == OK
        torch.cuda.synchronize()
        assert torch.equal(b2["box"], b["box"]), (name, want_cls, want_scores)
        assert _intact(b2["cls"]) != want_cls and _intact(b2["score"]) != want_scores and _intact(b2["label"]) != want_scores
        if want_scores:
            assert torch.equal(b2["score"], b["score"]) and torch.equal(b2["label"], b["label"])
        if want_cls:
            assert torch.equal(b2["cls"], b["cls"])


HEAD_REFUSALS = {"head_channels": dict(CH=-1), "n_anchor_0": dict(na=0), "null_boxes": dict(null="box")}


@pytest.mark.parametrize("name", list(HEAD_REFUSALS))
def test_head_refuses(name):
    c = G.head_case("three_classes").to(DEV)
    over = dict(HEAD_REFUSALS[name])
    if over.get("CH") == -1:
        over["CH"] = c.CH + 1
    b = _head_buffers(c)
    assert _head_call(c, b, **over) == INVALID
    torch.cuda.synchronize()
    for k, v in b.items():
        assert _intact(v), (name, k)
