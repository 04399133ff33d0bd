"""hvpr_pillar_vfe_train_fwd_f32 / hvpr_pillar_vfe_bwd_f32 (csrc/vfe_train.hip) against float64, element by element inside the derived
rounding bound of pfn_train_cases.py: no tolerance added, no element excluded; d_out is zero on the layer-1 entries whose decision
the reference cannot make (their share is asserted and reported), and no layer-0 decision is undecided.  test_pfn_train_host.py
shows on the CPU what that bound admits and what it catches.  The reference is computed on the device in float64 from the same fp32
inputs.  Every output lies inside a larger sentinel buffer; every row is run on a zeroed and on a 0xFF-filled workspace and must
give the same bits.  Every test reports max(err / bound) under "observed margins"."""
import pytest
import torch

import pfn_train_cases as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
SENTINEL, GUARD = F.SENTINEL, 256
SIZES = {"out": lambda M: M * 64, "mean0": lambda M: 16, "var0": lambda M: 16, "mean1": lambda M: 64, "var1": lambda M: 64,
         "dw0": lambda M: 160, "dgamma0": lambda M: 16, "dbeta0": lambda M: 16, "dw1": lambda M: 2048, "dgamma1": lambda M: 64,
         "dbeta1": lambda M: 64}
SHAPES = {"out": (-1, 64), "dw0": (16, 10), "dw1": (64, 32)}


def _buffers(M):
    return {k: torch.full((n(M) + GUARD,), SENTINEL, device=DEV) for k, n in SIZES.items()}


def _call(c, d_out, b, ws, M=None, P=None, short=0, null=None, backward=True):
    """Forward, then (unless backward is False) backward -> the two statuses.  null: the name of an argument passed as a null pointer."""
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    M, P = c.M if M is None else M, c.P if P is None else P
    ptr = lambda name, t: None if name == null else t.data_ptr()
    par = [ptr(k, getattr(c, k)) for k in ("w0", "gamma0", "beta0", "w1", "gamma1", "beta1")]
    geom = (c.eps, *F.VOXEL_SIZE, *F.OFFSETS)
    src = (ptr("voxels", c.voxels), ptr("num", c.num), ptr("coords", c.coords), M, P, *par, *geom)
    s = kernels._stream()
    st_f = lib().hvpr_pillar_vfe_train_fwd_f32(*src, *[ptr(k, b[k]) for k in F.FORWARD], ws.data_ptr(), ws.numel() - short, s)
    st_b = OK
    if backward:
        st_b = lib().hvpr_pillar_vfe_bwd_f32(*src, d_out.data_ptr(), *[ptr(k, b[k]) for k in F.GRADS], ws.data_ptr(), ws.numel() - short, s)
    return st_f, st_b


def _run(c, d_out, fill):
    from hvpr_amd._lib import lib
    need = lib().hvpr_pillar_vfe_train_workspace_bytes()
    assert need == F.workspace_bytes()
    b = _buffers(c.M)
    ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    assert _call(c, d_out, b, ws, backward=c.backward) == (OK, OK)          # (a forward-only row runs no backward)
    keys = F.FORWARD + (F.GRADS if c.backward else ())
    for k, n in SIZES.items():           # (the row after out[M], which an odd M's inactive half-wave must not write, is part of the guard)
        assert bool((b[k][n(c.M):] == SENTINEL).all()), (c.name, k, "wrote past its end")
    return {k: b[k][:SIZES[k](c.M)].view(SHAPES.get(k, (-1,))) for k in keys}


def _row(name, observed):
    c = F.case(name).to(DEV)
    r = F.reference(c)
    if c.backward:
        assert r["undecided0"] == 0 and r["masked_share"] <= F.MASKED_CAP, (name, r["undecided0"], r["masked_share"])
    d_out = r["d_out"].contiguous()
    got, again = _run(c, d_out, 0), _run(c, d_out, 0xFF)
    for k in got:
        assert torch.equal(got[k], again[k]), (name, k, "differs on a second call with a 0xFF workspace")
    fr = F.fractions(got, r)
    assert set(fr) == set(got), (name, sorted(fr))
    observed(f"pfn train [{name}] M={c.M} P={c.P}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items())
             + f"; masked share {r['masked_share']:.2e}")
    assert max(fr.values()) <= 1.0, (name, fr)
    return c, got, r


@pytest.mark.parametrize("name", [n for n in F.ROWS if n not in ("affine_edges", "d_out_zero")])
def test_row_within_the_bound(name, observed):
    _row(name, observed)


def test_affine_edges_are_exact(observed):
    """gamma1 == 0: its dW1 row is exactly zero.  A channel whose beta1 keeps every slot under the ReLU: out, dW1 row, d gamma1 and
    d beta1 exactly zero.  gamma0 == 0: its dW0 row exactly zero."""
    c, got, r = _row("affine_edges", observed)
    assert bool((got["dw1"][5] == 0).all()) and bool((got["dw1"][7] == 0).all()) and bool((got["dw0"][3] == 0).all())
    assert bool((got["out"][:, 7] == 0).all()) and float(got["dgamma1"][7]) == 0.0 == float(got["dbeta1"][7])
    assert float(got["dbeta1"][5]) != 0.0


def test_zero_d_out_gives_exactly_zero_gradients(observed):
    c, got, r = _row("d_out_zero", observed)
    for k in F.GRADS:
        assert bool((got[k] == 0).all()), k


def test_through_the_autograd_function(observed):
    """vfe._PfnTrain as the module calls it: the same numbers as the C entry points give."""
    from hvpr_amd import vfe
    c = F.case("eight_pillars").to(DEV)
    r = F.reference(c)
    par = [getattr(c, k).clone().requires_grad_(True) for k in ("w0", "gamma0", "beta0", "w1", "gamma1", "beta1")]
    out, m0, v0, m1, v1 = vfe._PfnTrain.apply(c.voxels, c.num, c.coords, *par, c.eps, F.VOXEL_SIZE, F.OFFSETS)
    grads = torch.autograd.grad(out, par, r["d_out"])
    got = dict(zip(F.FORWARD + F.GRADS, (out.detach(), m0, v0, m1, v1, *grads)))
    direct = _run(c, r["d_out"].contiguous(), 0)
    for k in got:
        assert torch.equal(got[k], direct[k]), k
    fr = F.fractions(got, r)
    observed("pfn train [_PfnTrain, eight_pillars]: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, fr


REFUSALS = {
    "P_0": (dict(P=0), UNSUPPORTED),
    "P_33": (dict(P=33), UNSUPPORTED),
    "M_0": (dict(M=0), INVALID),
    "null_voxels": (dict(null="voxels"), INVALID),
    "null_gamma1": (dict(null="gamma1"), INVALID),
    "short_workspace": (dict(short=1), WORKSPACE),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_pfn_refuses(name):
    """The buffers are those of the accepted M = 8, P = 5 call; both entry points refuse, and every output keeps its sentinel."""
    from hvpr_amd._lib import lib
    over, status = REFUSALS[name]
    c = F.case("eight_pillars").to(DEV)
    ws = torch.zeros(lib().hvpr_pillar_vfe_train_workspace_bytes(), dtype=torch.uint8, device=DEV)
    b = _buffers(c.M)
    assert _call(c, c.d_out, b, ws) == (OK, OK) and not any(bool((v == SENTINEL).all()) for v in b.values())
    b = _buffers(c.M)
    assert _call(c, c.d_out, b, ws, **over) == (status, status)
    for k, v in b.items():
        assert bool((v == SENTINEL).all()), (name, k)
