"""The training BatchNorm + ReLU kernels (hvpr_bn_stats_nhwc_f32, hvpr_bn_finalize_partials_f32, hvpr_bn_train_affine_f32,
hvpr_bn_relu_fwd_nhwc_f32, hvpr_bn_relu_bwd_sums / _apply_nhwc_f32) against float64, element by element inside the derived rounding
bound of bn_train_cases.py: no tolerance added, and no element excluded but the dz of those whose ReLU decision the reference
cannot make (their share is asserted and reported).  test_bn_train_host.py shows on the CPU that an honest fp32 form of the same
formulas is inside that bound and that each wrong variant falls outside it.  The reference is computed on the device in float64
from the same fp32 inputs.  Every test reports max(err / bound) under "observed margins"."""
import ctypes

import pytest
import torch

import bn_train_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/hvpr_amd.h hvpr_status
OFF, EXTRA, SENTINEL = B.SLICE_OFF, B.SLICE_EXTRA, B.SENTINEL


def _module(c):
    bn = torch.nn.BatchNorm2d(c.C, eps=c.eps, momentum=c.momentum, track_running_stats=c.running_mean is not None).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        if c.running_mean is not None:
            bn.running_mean.copy_(c.running_mean)
            bn.running_var.copy_(c.running_var)
    return bn


def _nhwc(t):
    return None if t is None else t.view(1, 1, t.shape[0], -1)


def _run(c):
    """The row through conv_train.bn_statistics, _bn_forward (statistics again, affine, running statistics, forward; a sliced row
    into a wider sentinel tensor at OFF) and _bn_backward (a sliced row's dy out of the wider tensor) -> dict of outputs on the device."""
    from hvpr_amd import conv_train
    P, C = c.P, c.C
    bn = _module(c)
    z = _nhwc(c.z)
    o = {}
    o["mean"], o["var"], o["invstd"], count = conv_train.bn_statistics(z, c.eps)
    assert count == P
    out = torch.full((1, 1, P, C + EXTRA), SENTINEL, device=DEV) if c.sliced else None
    y, (scale, shift, mean, invstd), count = conv_train._bn_forward(z, bn.weight.detach(), bn.bias.detach(), c.eps, None, bn, c.relu,
                                                                    _nhwc(c.gate), _nhwc(c.resid), out=out, out_coff=OFF if c.sliced else 0)
    assert torch.equal(mean, o["mean"]) and torch.equal(invstd, o["invstd"])
    if c.sliced:
        assert bool((y[..., :OFF] == SENTINEL).all()) and bool((y[..., OFF + C:] == SENTINEL).all()), (c.name, "sentinel")
        y = y[..., OFF:OFF + C]
    o["y"], o["scale"], o["shift"] = y.reshape(P, C), scale, shift
    if c.running_mean is not None:
        o["running_mean"], o["running_var"] = bn.running_mean.clone(), bn.running_var.clone()
        assert int(bn.num_batches_tracked) == 1, (c.name, int(bn.num_batches_tracked))
    if not c.backward:
        return o
    dy, pitch, off = (c.dy_wide, C + EXTRA, OFF) if c.sliced else (c.dy, C, 0)
    dz, o["dgamma"], o["dbeta"], dgate = conv_train._bn_backward(_nhwc(dy), pitch, off, z, scale, shift, mean, invstd, c.relu, _nhwc(c.gate), count)
    o["dz"] = dz.reshape(P, C)
    if c.gated:
        o["dgate"] = dgate.reshape(P)
    return o


def _compare(c, got, r, observed, what="bn train"):
    share = B.undecided_share(r)
    assert share <= B.UNDECIDED_CAP, (c.name, share)
    fr = B.fractions(got, r)
    assert set(fr) == {k for k in r if k != "undecided"}, (c.name, sorted(fr))
    observed(f"{what} [{c.name}] P={c.P} C={c.C}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items())
             + f"; undecided share {share:.2e}")
    assert max(fr.values()) <= 1.0, (c.name, fr)


def _row(name, observed):
    from hvpr_amd._lib import lib
    c = B.case(name).to(DEV)
    assert lib().hvpr_bn_workspace_bytes(c.P, c.C) == B.workspace_bytes(c.P, c.C)          # the slab of the bound's k
    got, again = _run(c), _run(c)
    for k in got:
        if k == "dgate" and B.dgate_atomics_meet(c.C):
            continue                # several atomic additions meet on a pixel: their order is not fixed
        assert torch.equal(got[k], again[k]), (name, k, "differs on a second call")
    r = B.reference(c)
    _compare(c, got, r, observed)
    return c, got, r


@pytest.mark.parametrize("name", [n for n in B.SMALL if n not in B.TWO_PART and n not in B.EDGE])          # (those: tests of their own below)
def test_row_within_the_bound(name, observed):
    _row(name, observed)


@pytest.mark.parametrize("name", list(B.LARGE))
def test_large_row_within_the_bound(name, observed):
    """Slabs other than 64 with 2049 workspace rows, and the second, ragged trip of the grid-stride loops."""
    _row(name, observed)


def test_gamma_zero_channels_are_exact(observed):
    """gamma = 0: beta = 0 gives y = dz = d gamma = d beta = 0 (a >= mask would let dy through into d beta), beta < 0 is all masked,
    beta > 0 passes everything: dz = 0 exactly and d beta = sum dy_m within its bound."""
    c, got, r = _row("gamma_zero", observed)
    for ch in (0, 1):
        assert torch.equal(got["y"][:, ch:ch + 1], c.resid[:, ch:ch + 1]), ch          # gate * 0 + resid
        for k in ("dz", "dgamma", "dbeta"):
            assert bool((got[k][..., ch] == 0).all()), (k, ch)
    assert bool((got["scale"][:3] == 0).all()) and torch.equal(got["shift"][:3], c.beta[:3])
    assert bool((got["dz"][:, 2] == 0).all())
    assert r["dz"].e[:, :3].max() == 0 and r["dbeta"].e[:2].max() == 0 and r["dbeta"].e[2] > 0
    want = (c.dy[:, 2].double() * c.gate.double()).sum()
    assert abs(float(got["dbeta"][2]) - float(want)) <= float(r["dbeta"].e[2])


def test_bn_relu_autograd_gated_within_the_bound(observed):
    """conv_train.bn_relu as the training step calls it: gate * relu(bn(z)) + resid, differentiated."""
    from hvpr_amd import conv_train
    c = B.case("gated").to(DEV)
    bn = _module(c)
    z, gate, resid = (_nhwc(t).clone().requires_grad_(True) for t in (c.z, c.gate, c.resid))
    y = conv_train.bn_relu(z, bn, relu=True, gate=gate, resid=resid)
    y.backward(_nhwc(c.dy))
    got = {"y": y.detach().reshape(c.P, c.C), "dz": z.grad.reshape(c.P, c.C), "dgate": gate.grad.reshape(c.P), "dgamma": bn.weight.grad,
           "dbeta": bn.bias.grad, "running_mean": bn.running_mean, "running_var": bn.running_var}
    assert torch.equal(resid.grad, _nhwc(c.dy)) and int(bn.num_batches_tracked) == 1
    r = B.reference(c)
    r = {k: v for k, v in r.items() if k in got or k == "undecided"}
    _compare(c, got, r, observed, "bn train bn_relu")


def test_bn_relu_cat_within_the_bound(observed):
    """conv_train.bn_relu_cat with two branches: each normalises into its slice of the result and takes its gradient out of the
    result's gradient."""
    from hvpr_amd import conv_train
    ca, cb = B.Case(37, 32, seed=1, name="cat_0").to(DEV), B.Case(37, 24, seed=2, name="cat_1").to(DEV)
    bns = [_module(ca), _module(cb)]
    zs = [_nhwc(c.z).clone().requires_grad_(True) for c in (ca, cb)]
    y = conv_train.bn_relu_cat(zs, bns)
    assert y.shape == (1, 1, 37, 56)
    y.backward(_nhwc(torch.cat([ca.dy, cb.dy], 1)))
    lo = 0
    for c, bn, z in zip((ca, cb), bns, zs):
        got = {"y": y.detach()[0, 0, :, lo:lo + c.C], "dz": z.grad.reshape(c.P, c.C), "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
               "running_mean": bn.running_mean, "running_var": bn.running_var}
        r = B.reference(c)
        _compare(c, got, {k: v for k, v in r.items() if k in got or k == "undecided"}, observed, "bn train bn_relu_cat")
        lo += c.C


@pytest.mark.parametrize("C", B.FINALIZE_C)
@pytest.mark.parametrize("rows", B.FINALIZE_ROWS)
def test_finalize_partials_within_the_bound(rows, C, observed):
    """hvpr_bn_finalize_partials_f32 on synthetic workspace rows: k_bn_finalize4 (C % 4 == 0) over 1, 2 and 5 trips of its 256 threads,
    k_bn_finalize (one wave per channel) for C = 6, 7; the count is not the row count."""
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    p = B.Partials(rows, C)
    part = p.partials.to(DEV)
    out = torch.full((3, C + 8), SENTINEL, device=DEV)
    got = {}
    for _ in range(2):
        assert lib().hvpr_bn_finalize_partials_f32(part.data_ptr(), rows, C, p.count, p.eps, out[0].data_ptr(), out[1].data_ptr(),
                                                   out[2].data_ptr(), kernels._stream()) == OK
        now = {k: out[i, :C].cpu() for i, k in enumerate(("mean", "var", "invstd"))}
        assert not got or all(torch.equal(got[k], now[k]) for k in now)
        got = now
    assert bool((out[:, C:] == SENTINEL).all())
    fr = B.fractions(got, p.reference())
    observed(f"bn train finalize rows={rows} C={C}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()))
    assert len(fr) == 3 and max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("name", list(B.TWO_PART))
def test_two_part_batch_matches_the_joint_batch(name, observed):
    """The SyncBatchNorm path without a process group: per-part sums from hvpr_bn_relu_bwd_sums_nhwc_f32, added and divided by the
    joint count in float64 as conv_train.sync_backward_sums does, then hvpr_bn_relu_bwd_apply_nhwc_f32 per part with the pre-divided
    totals and inv_count = 1, against the float64 dz of the joint batch."""
    from hvpr_amd import conv_train, kernels
    from hvpr_amd._lib import lib
    c = B.case(name).to(DEV)
    P, C = c.P, c.C
    z = _nhwc(c.z)
    _, (scale, shift, mean, invstd), _ = conv_train._bn_forward(z, c.gamma, c.beta, c.eps, None, _module(c), c.relu, _nhwc(c.gate), _nhwc(c.resid))
    ws = torch.empty(B.workspace_bytes(P, C), dtype=torch.uint8, device=DEV)
    got = {"dz": torch.full((P, C), SENTINEL, device=DEV)}
    if c.gated:
        got["dgate"] = torch.full((P,), SENTINEL, device=DEV)
    sums, lo = [], 0

    def common(lo, Pj):
        return (c.dy[lo:lo + Pj].data_ptr(), C, 0, c.z[lo:lo + Pj].data_ptr(), Pj, C, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                invstd.data_ptr(), 1 if c.relu else 0, c.gate[lo:lo + Pj].data_ptr() if c.gated else None)
    for j, Pj in enumerate(c.parts):
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        assert lib().hvpr_bn_relu_bwd_sums_nhwc_f32(*common(lo, Pj), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()) == OK
        got[f"dgamma_{j}"], got[f"dbeta_{j}"] = dg, db
        sums.append((dg, db))
        lo += Pj
    packed = torch.cat([sum(s[0].double() for s in sums), sum(s[1].double() for s in sums)]) / float(P)
    dg_t, db_t = packed[:C].float().contiguous(), packed[C:].float().contiguous()
    lo = 0
    for Pj in c.parts:
        assert lib().hvpr_bn_relu_bwd_apply_nhwc_f32(*common(lo, Pj), got["dgate"][lo:lo + Pj].data_ptr() if c.gated else None,
                                                     got["dz"][lo:lo + Pj].data_ptr(), dg_t.data_ptr(), db_t.data_ptr(), 1.0, kernels._stream()) == OK
        lo += Pj
    r = B.reference(c)
    keep = set(got) | {"undecided"}
    _compare(c, got, {k: v for k, v in r.items() if k in keep}, observed, "bn train two-part")


# ------------------------------------------------------------------------------------------------ refusals
# Every buffer is far larger than any launch these small dimensions could address, so a missing refusal would show as a wrong status
# and a changed sentinel, not as a write outside a buffer.  Every output and the workspace are slices of one sentinel tensor.
class _Buffers:
    N = 1 << 14

    def __init__(self):
        self.src = torch.randn(4, self.N, device=DEV)                # z, dy, resid, gate
        self.par = torch.rand(8, 2048, device=DEV) + 0.5             # per-channel inputs
        self.tracked = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.out = torch.full((16, self.N), SENTINEL, device=DEV)

    def reset(self):
        self.out.fill_(SENTINEL)
        self.tracked.zero_()

    def untouched(self):
        return bool((self.out == SENTINEL).all()) and int(self.tracked) == 0


@pytest.fixture(scope="module")
def bufs():
    return _Buffers()


def _call(b, fn, **over):
    from hvpr_amd import kernels
    from hvpr_amd._lib import lib
    a = dict(P=4, C=8, pitch=8, off=0, gate=False, resid=False, dgate=False, short=0, inv_count=0.25, rm=True, rv=True, rows=3)
    a.update(over)
    L, s = lib(), kernels._stream()
    z, dy, resid, gate = (b.src[i].data_ptr() for i in range(4))
    par = [b.par[i].data_ptr() for i in range(8)]
    o = [b.out[i].data_ptr() for i in range(16)]
    need = L.hvpr_bn_workspace_bytes(max(a["P"], 1), max(a["C"], 4))
    assert 0 < need <= 4 * b.N
    if fn == "stats":
        return L.hvpr_bn_stats_nhwc_f32(z, a["P"], a["C"], B.EPS, o[0], o[1], o[2], o[3], need - a["short"], s)
    if fn == "finalize":
        return L.hvpr_bn_finalize_partials_f32(z, a["rows"], a["C"], 12, B.EPS, o[0], o[1], o[2], s)
    if fn == "affine":
        return L.hvpr_bn_train_affine_f32(par[0], par[1], par[2], a["C"], par[3], par[4], 0.1, 0.1, o[0] if a["rm"] else None,
                                          o[1] if a["rv"] else None, b.tracked.data_ptr(), o[2], o[3], s)
    if fn == "fwd":
        return L.hvpr_bn_relu_fwd_nhwc_f32(z, a["P"], a["C"], par[0], par[1], 1, gate if a["gate"] else None, resid if a["resid"] else None,
                                           o[0], a["pitch"], a["off"], s)
    common = (dy, a["pitch"], a["off"], z, a["P"], a["C"], par[0], par[1], par[2], par[3], 1, gate if a["gate"] else None)
    if fn == "sums":
        return L.hvpr_bn_relu_bwd_sums_nhwc_f32(*common, o[0], o[1], o[3], need - a["short"], s)
    assert fn == "apply"
    return L.hvpr_bn_relu_bwd_apply_nhwc_f32(*common, o[4] if a["dgate"] else None, o[5], par[4], par[5], ctypes.c_double(a["inv_count"]), s)


_SLICE = {
    "offset_not_multiple_of_4": dict(pitch=16, off=2),
    "pitch_not_multiple_of_4": dict(pitch=10),
    "slice_past_the_pitch": dict(pitch=12, off=8),
}
BN_ACCEPTS = [("stats", dict()), ("stats", dict(C=1024)), ("finalize", dict()), ("finalize", dict(C=6)), ("affine", dict()),
              ("affine", dict(rm=False, rv=False)), ("fwd", dict()), ("fwd", dict(gate=True, resid=True)), ("fwd", dict(pitch=16, off=4)),
              ("sums", dict()), ("sums", dict(pitch=16, off=4, gate=True)), ("apply", dict()), ("apply", dict(gate=True, dgate=True)),
              ("apply", dict(pitch=16, off=4))]
BN_REFUSALS = {
    "stats_C_6": ("stats", dict(C=6), UNSUPPORTED),
    "stats_C_1028": ("stats", dict(C=1028), UNSUPPORTED),
    "stats_short_workspace": ("stats", dict(short=1), WORKSPACE),
    "stats_no_pixels": ("stats", dict(P=0), INVALID),
    "finalize_C_2": ("finalize", dict(C=2), UNSUPPORTED),
    "finalize_C_1028": ("finalize", dict(C=1028), UNSUPPORTED),
    "finalize_no_rows": ("finalize", dict(rows=0), INVALID),
    "affine_running_mean_without_var": ("affine", dict(rv=False), INVALID),
    "affine_running_var_without_mean": ("affine", dict(rm=False), INVALID),
    "affine_no_channels": ("affine", dict(C=0), INVALID),
    "fwd_C_6": ("fwd", dict(C=6), UNSUPPORTED),
    "fwd_gate_without_resid": ("fwd", dict(gate=True), INVALID),
    "fwd_resid_without_gate": ("fwd", dict(resid=True), INVALID),
    **{f"fwd_{k}": ("fwd", v, UNSUPPORTED) for k, v in _SLICE.items()},
    "sums_C_6": ("sums", dict(C=6, pitch=6), UNSUPPORTED),
    "sums_C_1028": ("sums", dict(C=1028, pitch=1028), UNSUPPORTED),
    "sums_short_workspace": ("sums", dict(short=1), WORKSPACE),
    **{f"sums_{k}": ("sums", v, UNSUPPORTED) for k, v in _SLICE.items()},
    "apply_C_6": ("apply", dict(C=6, pitch=6), UNSUPPORTED),
    "apply_C_1028": ("apply", dict(C=1028, pitch=1028), UNSUPPORTED),
    "apply_gate_without_dgate": ("apply", dict(gate=True), INVALID),
    "apply_dgate_without_gate": ("apply", dict(dgate=True), INVALID),
    "apply_inv_count_0": ("apply", dict(inv_count=0.0), INVALID),
    "apply_inv_count_negative": ("apply", dict(inv_count=-0.25), INVALID),
    **{f"apply_{k}": ("apply", v, UNSUPPORTED) for k, v in _SLICE.items()},
}


def test_bn_accepts_the_base_calls(bufs):
    """The calls every refusal below is one step away from are accepted and write: a refusal cannot pass because the template is wrong."""
    for fn, over in BN_ACCEPTS:
        bufs.reset()
        assert _call(bufs, fn, **over) == OK, (fn, over)
        assert not bufs.untouched(), (fn, over)
    bufs.reset()


@pytest.mark.parametrize("name", list(BN_REFUSALS))
def test_bn_refuses(name, bufs):
    fn, over, status = BN_REFUSALS[name]
    bufs.reset()
    assert _call(bufs, fn, **over) == status
    assert bufs.untouched()
