"""GPU: hvpr_attend_rows_fwd_f32 / kernels.attend_rows / map_to_bev._AttendRows — the "attend over k rows" of get_score
(pointpillar_scatter.py:76-81) and of the memory's training branch (memory_module.py:53-57) as one HIP op.

Comparators are torch expressions written here: float64 for the true value, and the fp32 expression the op replaced in
map_to_bev.py (gather -> mul -> sum -> softmax -> mul -> sum) as the yardstick of what an fp32 evaluation achieves.  Value bar: the
op's largest absolute error <= 2 x the largest absolute error of that fp32 torch expression against the same float64 result, + 1e-7
(both are fp32 evaluations that differ in summation order and exp; the factor 2 is room for order).  Gradient bar: the same rule
norm-wise — ||g_op - g_64|| <= max(2 ||g_torch32 - g_64||, 1e-6 ||g_64||); 1e-6 of the norm is ~10 fp32 ulps, below which two
correct fp32 sums cannot be told apart."""
import copy

import numpy as np
import pytest
import torch

import torch_forms
from hvpr_amd import kernels, map_to_bev
from hvpr_amd.config import AttrDict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 64


def torch_attend(q, rows, idx):
    """The expression of map_to_bev.py before the op (any dtype).  Returns (out, w); out-of-range picks are not handled here."""
    pos = rows[idx]                                                                   # (M, k, C)
    w = torch.softmax((q.unsqueeze(1) * pos).sum(dim=2), dim=1)
    return (w.detach().unsqueeze(2) * pos).sum(dim=1), w


def _inputs(M, N, k, scale, seed, hot=False):
    g = torch.Generator().manual_seed(seed)
    rows = (torch.relu(torch.randn(N, C, generator=g)) * scale).to(DEV)
    q = torch.relu(torch.randn(M, C, generator=g)).to(DEV)
    if hot:         # all picks on N/10 points: every picked point serves many (pillar, k) pairs
        idx = (torch.randint(0, max(N // 10, 1), (M, k), generator=g) * 10).clamp(max=N - 1).to(DEV)
    else:
        idx = torch.randint(0, N, (M, k), generator=g).to(DEV)
    return q, rows, idx


CASES = [(1, 20, 20), (700, 5000, 20), (3900, 16384, 20), (257, 999, 1), (64, 4096, 32)]


@pytest.mark.parametrize("scale", [0.5, 4.0])
@pytest.mark.parametrize("M,N,k", CASES)
def test_values_against_float64_within_twice_the_fp32_torch_error(M, N, k, scale, observed):
    q, rows, idx = _inputs(M, N, k, scale, seed=M + k)
    out, w = kernels.attend_rows(q, rows, idx.to(torch.int32))
    assert out.shape == (M, C) and w.shape == (M, k)
    o64, w64 = torch_attend(q.double(), rows.double(), idx)
    o32, w32 = torch_attend(q, rows, idx)
    e_out, t_out = float((out.double() - o64).abs().max()), float((o32.double() - o64).abs().max())
    e_w, t_w = float((w.double() - w64).abs().max()), float((w32.double() - w64).abs().max())
    rowsum = float((w.double().sum(dim=1) - 1).abs().max())
    line = (f"attend_rows M={M} N={N} k={k} x{scale}: max |err| out {e_out:.3e} (torch fp32 {t_out:.3e}), w {e_w:.3e} (torch fp32 {t_w:.3e}), "
            f"|sum w - 1| {rowsum:.2e}")
    print(line)
    observed(line)
    assert e_out <= 2 * t_out + 1e-7, line
    assert e_w <= 2 * t_w + 1e-7, line
    assert rowsum <= k * 2.0 ** -23, line


@pytest.mark.parametrize("M,N,k", CASES)
def test_dense_form_equals_indexed_form_bit_for_bit(M, N, k):
    q, rows, idx = _inputs(M, N, k, 0.5, seed=3 * M + k)
    out_i, w_i = kernels.attend_rows(q, rows, idx.to(torch.int32))
    out_d, w_d = kernels.attend_rows(q, rows[idx].reshape(-1, C).contiguous(), None, k)
    assert torch.equal(out_i, out_d) and torch.equal(w_i, w_d)


def test_out_of_range_picks_read_a_row_of_zeros():
    M, N, k = 700, 5000, 20
    q, rows, idx = _inputs(M, N, k, 0.5, seed=11)
    g = torch.Generator().manual_seed(12)
    bad = (torch.rand(M, k, generator=g) < 0.03).to(DEV)
    low = (torch.rand(M, k, generator=g) < 0.5).to(DEV)
    idx_bad = torch.where(bad, torch.where(low, torch.full_like(idx, -1), torch.full_like(idx, N)), idx)
    idx_bad[0, :] = -1                                       # a pillar whose picks are all out of range: uniform weights, zero output
    bad[0, :] = True
    assert int(bad.sum()) > k
    out, w = kernels.attend_rows(q, rows, idx_bad.to(torch.int32))
    rows_z = torch.cat([rows, rows.new_zeros(1, C)], 0)
    out_z, w_z = kernels.attend_rows(q, rows_z, torch.where(bad, torch.full_like(idx, N), idx).to(torch.int32))
    assert torch.equal(out, out_z) and torch.equal(w, w_z)
    assert float(out[0].abs().max()) == 0.0 and torch.equal(w[0], torch.full_like(w[0], 1.0 / k))
    o64, _ = torch_attend(q.double(), rows_z.double(), torch.where(bad, torch.full_like(idx, N), idx))
    assert float((out.double() - o64).abs().max()) < 1e-5


def _grad_op(mode, q, rows, idx, cot):
    N = rows.shape[0]
    qq, rr = q.clone().requires_grad_(True), rows.clone().requires_grad_(True)
    if mode == "plan":
        out = map_to_bev._AttendRows.apply(qq, rr, idx, kernels.EdgePlan(idx, N))
    elif mode == "noplan":
        out = map_to_bev._AttendRows.apply(qq, rr, idx, None)
    else:               # dense over the materialised picks: autograd carries the gradient back through the torch index
        out = map_to_bev._AttendRows.apply(qq, rr[idx].reshape(-1, C), None, None)
    (out * cot).sum().backward()
    return out.detach(), rr.grad.clone(), qq.grad


def _grad_torch(q, rows, idx, cot, dtype):
    rr = rows.to(dtype).clone().requires_grad_(True)
    out, _ = torch_attend(q.to(dtype), rr, idx)
    (out * cot.to(dtype)).sum().backward()
    return rr.grad


@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("mode", ["plan", "noplan", "dense"])
def test_gradients_against_float64_autograd(mode, hot, observed):
    M, N, k = 700, 5000, 20
    q, rows, idx = _inputs(M, N, k, 0.5, seed=77, hot=hot)
    cot = torch.randn(M, C, generator=torch.Generator().manual_seed(78)).to(DEV)
    _, g_op, gq = _grad_op(mode, q, rows, idx, cot)
    assert gq is None                                        # q only enters through the detached weights
    g64 = _grad_torch(q, rows, idx, cot, torch.float64)
    g32 = _grad_torch(q, rows, idx, cot, torch.float32)
    n64 = float(g64.norm())
    e_op, e_t = float((g_op.double() - g64).norm()), float((g32.double() - g64).norm())
    line = (f"_AttendRows grad {mode}{' hot' if hot else ''}: ||err|| / ||g|| {e_op / n64:.3e} (torch fp32 {e_t / n64:.3e}); max |err| "
            f"{float((g_op.double() - g64).abs().max()):.3e} (torch fp32 {float((g32.double() - g64).abs().max()):.3e})")
    print(line)
    observed(line)
    assert n64 > 0
    assert e_op <= max(2 * e_t, 1e-6 * n64), line


def test_forward_and_backward_are_bit_reproducible():
    M, N, k = 3900, 16384, 20
    q, rows, idx = _inputs(M, N, k, 0.5, seed=5, hot=True)
    cot = torch.randn(M, C, generator=torch.Generator().manual_seed(6)).to(DEV)
    a = _grad_op("plan", q, rows, idx, cot)
    b = _grad_op("plan", q, rows, idx, cot)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = _grad_op("noplan", q, rows, idx, cot)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def _scatter_module(nx, ny):
    cfg = AttrDict(NUM_BEV_FEATURES=128, NUM_COORD_POINTS=3, NUM_PT_FEATURES=64, NUM_SCALE_FEATURES=32, NUM_K=20, NUM_M=2000, SHRINK_TH=0.0025)
    torch.manual_seed(31)
    m = map_to_bev.PointPillarScatter_Agg_Memory_1_scale(cfg, np.array([nx, ny, 1]))
    m.memory.weight.data.mul_(4.0)                           # supports of 10-80 items per row (G16's regime)
    return m.to(DEV).train()


def _scatter_batch(B, m_per_frame, n_per_frame, nx, ny, seed):
    g = torch.Generator().manual_seed(seed)
    coords, pcoords = [], []
    for b in range(B):
        cell = torch.randperm(nx * ny, generator=g)[:m_per_frame]
        coords.append(torch.stack([torch.full_like(cell, b), torch.zeros_like(cell), cell // nx, cell % nx], 1))
        pcoords.append(torch.cat([torch.full((n_per_frame, 1), float(b)), torch.rand(n_per_frame, 3, generator=g)], 1))
    M, N = B * m_per_frame, B * n_per_frame
    return {"pillar_features": torch.relu(torch.randn(M, 64, generator=g)).to(DEV),
            "pillar_scale_features": torch.relu(torch.randn(M, 32, generator=g)).to(DEV),
            "point_features": (torch.relu(torch.randn(N, 64, generator=g)) * 0.5).to(DEV),
            "voxel_coords": torch.cat(coords, 0).to(torch.int32).to(DEV), "point_coords": torch.cat(pcoords, 0).to(DEV), "batch_size": B}


CANVASES = ("spatial_features", "spatial_features_point", "spatial_scale_features")


def _run_scatter(mod, batch, cots, dtype):
    mod.memory.weight.grad = None
    ins = {k: batch[k].to(dtype).clone().requires_grad_(True) for k in ("pillar_features", "pillar_scale_features", "point_features")}
    d = mod({**ins, "voxel_coords": batch["voxel_coords"], "point_coords": batch["point_coords"].to(dtype), "batch_size": batch["batch_size"]})
    vals = {k: d[k].detach() for k in CANVASES + ("point_positive_features", "memory_positive_features")}
    sum((d[k] * cots[k].to(dtype)).sum() for k in CANVASES).backward()
    return vals, {"point_features": ins["point_features"].grad, "memory.weight": mod.memory.weight.grad.clone()}


def test_scatter_module_training_branch_against_the_torch_form(observed, monkeypatch):
    """PointPillarScatter_Agg_Memory_1_scale in training mode, two frames, against tests/torch_forms.scatter_train (with get_score and
    the memory's torch form) on the same weights.  The torch side takes its top-k picks from the product's kernel (exact on the fp32
    values) so that a tie at the k-th logit cannot swap a pick between the two sides: the picks are not what this test is about.
    Tolerances: those of fixture G16 on the GPU (train_fixture_cases.run_g16 as called by test_gpu_train_fixtures.py: values to 1e-4 of
    the tensor's maximum, the memory read-out norm-wise to 1e-3, gradients norm-wise to max(1e-4, 3 x the torch fp32 form's own
    distance from its float64 run))."""
    nx, ny, B = 48, 40, 2
    hip = _scatter_module(nx, ny)
    batch = _scatter_batch(B, 300, 2000, nx, ny, seed=41)
    g = torch.Generator().manual_seed(42)
    cots = {k: torch.randn(B, c, ny, nx, generator=g).to(DEV) for k, c in zip(CANVASES, (128, 128, 32))}
    refs = {}
    monkeypatch.setattr(torch_forms, "topk_points", lambda self, pillars, points: hip._topk_points(pillars.float(), points.float()))
    for dtype in (torch.float32, torch.float64):
        ref = copy.deepcopy(hip).to(dtype)
        torch_forms.patch(ref)
        refs[dtype] = _run_scatter(ref, batch, cots, dtype)
    vals, grads = _run_scatter(hip, batch, cots, torch.float32)
    (v32, g32), (v64, g64) = refs[torch.float32], refs[torch.float64]
    vt = 1e-4
    for k in CANVASES + ("point_positive_features",):
        ref = v32[k]
        assert vals[k].shape == ref.shape, k
        e = float((vals[k] - ref).abs().max()) / float(ref.abs().max())
        observed(f"scatter train branch vs torch form: {k} max |diff| / max |ref| {e:.2e} (bar {vt:.0e})")
        assert e <= vt, (k, e)
    e = float((vals["memory_positive_features"] - v32["memory_positive_features"]).norm() / v32["memory_positive_features"].norm())
    observed(f"scatter train branch vs torch form: memory_positive_features norm-wise {e:.2e} (bar {10 * vt:.0e})")
    assert float(v32["memory_positive_features"].norm()) > 0 and e < 10 * vt, e
    for k in grads:
        n = float(g64[k].norm())
        e = float((grads[k].double() - g64[k]).norm()) / n
        tol = max(1e-4, 3 * float((g32[k].double() - g64[k]).norm()) / n)
        observed(f"scatter train branch vs torch form (float64): grad {k} norm-wise {e:.2e} (bar {tol:.2e})")
        assert n > 0 and e < tol, (k, e, tol)


def test_grouped_training_path_holds_no_gathered_tensor(observed):
    """At batch-16 sizes (16 frames x 16 384 points, ~3 800 pillars each, k = 20, the 296 x 248 canvas): the rise of
    torch.cuda.max_memory_allocated over one forward + backward of the scatter module, less the outputs it returns and the gradients
    of its inputs, stays below the size of ONE gathered (M, k, 64) fp32 tensor — the expression this op replaced held four of them
    (two forward, their two gradients)."""
    nx, ny, B, mpf, npf = 296, 248, 16, 3812, 16384
    mod = _scatter_module(nx, ny)
    batch = _scatter_batch(B, mpf, npf, nx, ny, seed=51)
    M = B * mpf
    ins = {k: batch[k].clone().requires_grad_(True) for k in ("pillar_features", "pillar_scale_features", "point_features")}
    g = torch.Generator().manual_seed(52)
    cots = {k: torch.randn(B, c, ny, nx, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
            for k, c in zip(CANVASES, (128, 128, 32))}
    mod._workspace(B, torch.device(DEV))                    # the persistent cell map is no transient
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    d = mod({**ins, "voxel_coords": batch["voxel_coords"], "point_coords": batch["point_coords"], "batch_size": B})
    outs = [d[k] for k in CANVASES + ("point_positive_features", "memory_positive_features")]
    torch.autograd.backward([d[k] for k in CANVASES], [cots[k] for k in CANVASES])    # (no canvas-sized product of the test's own)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    # an output is counted with the storage it keeps alive (the 32-channel scale canvas is a slice of the 64-channel kernel's canvas)
    stores = {t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in outs}
    kept = sum(stores.values()) + sum(t.grad.numel() * 4 for t in ins.values()) + mod.memory.weight.grad.numel() * 4
    gathered = M * 20 * 64 * 4
    line = (f"scatter module fwd+bwd at batch 16 (M={M}): peak rise {rise / 2**20:.0f} MiB, outputs + input gradients {kept / 2**20:.0f} MiB, "
            f"transients {(rise - kept) / 2**20:.0f} MiB; one (M,k,64) tensor = {gathered / 2**20:.0f} MiB")
    print(line)
    observed(line)
    assert rise - kept < gathered, line
