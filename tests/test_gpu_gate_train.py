"""hvpr_spatial_gate_train_fwd_f32 / _bwd_f32 (csrc/gate_train.hip) against float64, element by element inside the derived rounding
bound of gate_train_cases.py: no tolerance added, no element excluded, the arg-max compared exactly.  test_gate_train_host.py shows on
the CPU that an honest fp32 form of the same formulas is inside that bound and that each wrong variant falls outside it.  The
reference is computed on the device in float64 from the same fp32 inputs.  Every output lies inside a larger sentinel buffer; every
row is run on a zeroed and on a 0xFF-filled workspace and must give the same bits.  Every test reports max(err / bound) under
"observed margins"."""
import pytest
import torch

import gate_train_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
SENTINEL, GUARD = G.SENTINEL, 1024
SHAPES = {"pooled": lambda c: c.P * 2, "argmax": lambda c: c.P, "a": lambda c: c.P, "stats": lambda c: 3, "gate": lambda c: c.P,
          "dy": lambda c: c.P * c.C, "dw18": lambda c: 18, "dbias": lambda c: 1, "dgamma": lambda c: 1, "dbeta": lambda c: 1}


def _buffers(c):
    return {k: torch.full((n(c) + GUARD,), int(SENTINEL) if k == "argmax" else SENTINEL, device=DEV,
                          dtype=torch.int32 if k == "argmax" else torch.float32) for k, n in SHAPES.items()}


def _call(c, b, ws, dims=None, short=0):
    """Forward, then backward on what the forward returned -> the two statuses."""
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    N, H, W, C = dims or (c.N, c.H, c.W, c.C)
    p = {k: v.data_ptr() for k, v in b.items()}
    w18 = c.w.reshape(18).contiguous()
    s = kernels._stream()
    st_f = lib().hvpr_spatial_gate_train_fwd_f32(c.y.data_ptr(), N, H, W, C, w18.data_ptr(), c.bias.data_ptr(), c.gamma.data_ptr(),
                                                 c.beta.data_ptr(), c.eps, p["pooled"], p["argmax"], p["a"], p["stats"], p["gate"],
                                                 ws.data_ptr(), ws.numel() - short, s)
    st_b = lib().hvpr_spatial_gate_train_bwd_f32(c.dgate.data_ptr(), p["gate"], p["a"], p["stats"], p["pooled"], p["argmax"], w18.data_ptr(),
                                                 c.gamma.data_ptr(), N, H, W, C, p["dy"], p["dw18"], p["dbias"], p["dgamma"], p["dbeta"],
                                                 ws.data_ptr(), ws.numel() - short, s)
    return st_f, st_b


def _run(c, fill):
    from hvpr_amd._lib import lib
    need = lib().hvpr_spatial_gate_train_workspace_bytes(c.N, c.H, c.W)
    assert need == G.workspace_bytes(c.N, c.H, c.W)          # the tiles and rows of the bound's k
    b = _buffers(c)
    ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    assert _call(c, b, ws) == (OK, OK)
    for k, n in SHAPES.items():
        assert bool((b[k][n(c):] == b[k].new_tensor(SENTINEL)).all()), (c.name, k, "wrote past its end")
    return {k: b[k][:n(c)] for k, n in SHAPES.items()}


def _row(name, observed):
    c = G.case(name).to(DEV)
    got, again = _run(c, 0), _run(c, 0xFF)
    for k in got:
        assert torch.equal(got[k], again[k]), (name, k, "differs on a second call with a 0xFF workspace")
    r = G.reference(c)
    assert torch.equal(got["argmax"].long(), r["argmax"].reshape(-1)), name
    fr = G.fractions(got, r)
    observed(f"gate train [{name}] {c.N}x{c.H}x{c.W}x{c.C}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, (name, fr)
    return c, got, r


@pytest.mark.parametrize("name", list(G.ROWS))
def test_row_within_the_bound(name, observed):
    c, got, r = _row(name, observed)
    zero = {"gamma_zero": ("dy", "dw18", "dbias"), "dgate_zero": ("dy", "dw18", "dbias", "dgamma", "dbeta")}.get(name, ())
    for k in zero:
        assert bool((got[k] == 0).all()), (name, k)
    if name == "constant_field":
        assert float(got["stats"][1]) <= float(r["stats"].e[1])


@pytest.mark.parametrize("name", list(G.LARGE))
def test_large_row_within_the_bound(name, observed):
    """k_gt_bwd_red's grid-stride loop past its 1024 x 2048 pixels."""
    _row(name, observed)


REFUSALS = {
    "C_0": (dict(C=0), UNSUPPORTED),
    "C_2": (dict(C=2), UNSUPPORTED),
    "C_6": (dict(C=6), UNSUPPORTED),
    "H_0": (dict(H=0), INVALID),
    "short_workspace": (dict(short=1), WORKSPACE),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gate_refuses(name):
    """The buffers are those of the accepted 3x5x7x8 call, larger than anything these dimensions address; both entry points
    refuse, and every output keeps its sentinel."""
    from hvpr_amd._lib import lib
    over, status = REFUSALS[name]
    c = G.case("pixels_not_by_32").to(DEV)
    ws = torch.zeros(lib().hvpr_spatial_gate_train_workspace_bytes(c.N, c.H, c.W), dtype=torch.uint8, device=DEV)
    b = _buffers(c)
    assert _call(c, b, ws) == (OK, OK) and not any(bool((v == v.new_tensor(SENTINEL)).all()) for v in b.values())
    b = _buffers(c)
    d = dict(N=c.N, H=c.H, W=c.W, C=c.C, short=0)
    d.update(over)
    assert _call(c, b, ws, (d["N"], d["H"], d["W"], d["C"]), d["short"]) == (status, status)
    for k, v in b.items():
        assert bool((v == v.new_tensor(SENTINEL)).all()), (name, k)
