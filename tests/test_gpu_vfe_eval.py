"""The eval pillar encoder (csrc/vfe.hip) against float64, element by element inside the derived rounding bound of vfe_eval_cases.py: no
tolerance added, no element excluded, pillar_mask bit-exact.  test_vfe_eval_host.py shows on the CPU what that bound admits and what
it catches.  The reference is computed on the device in float64 from the same fp32 words.

  rows form     hvpr_pillar_vfe_fwd_f32 (k_vfe_rows), one call of kernels.pillar_vfe_fwd per row of the table; m_device and the
                refusals through the C entry point on sentinel-filled buffers.
  packed form   hvpr_encode_fwd_f32 (k_vfe_gather) on point clouds whose arena holds a chosen sequence of point counts, with both
                forms of the index phase: (1) equal bit for bit to voxelize -> pillar_vfe_fwd -> memory_scatter_fwd, (2) inside the
                bound against float64 computed from the returned voxels, (3) the production form, want_voxels = want_mask = False
                (no sort: a pillar's points in arena arrival order), equal bit for bit to the form with both outputs on.

Every test reports max(err / bound) under "observed margins"."""
import numpy as np
import pytest
import torch

import vfe_eval_cases as V
from hvpr_amd import kernels, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OK, INVALID, UNSUPPORTED = 0, -1, -2                          # include/hvpr_amd.h hvpr_status
SENTINEL, GUARD = V.SENTINEL, 256
G = V.GRIDS["kitti"]
VS, GRID = list(G["vs"]), [G["nx"], G["ny"], 1]
RNG = list(G["lo"]) + [G["lo"][0] + G["vs"][0] * G["nx"], G["lo"][1] + G["vs"][1] * G["ny"], G["lo"][2] + G["vs"][2]]
OFF = V.offsets_of("kitti")


# ------------------------------------------------------------------------------------------------ rows form
@pytest.mark.parametrize("name", list(V.ROWS))
def test_row_within_the_bound(name, observed):
    c = V.case(name).to(DEV)
    r = V.reference(c)
    md = None if c.m_device is None else torch.tensor([c.m_device], dtype=torch.int32, device=DEV)
    g = V.GRIDS[c.grid]
    pf, sf, mask = kernels.pillar_vfe_fwd(c.voxels, c.num, c.coords, c.folded(), list(g["vs"]), V.offsets_of(c.grid), m_device=md)
    torch.cuda.synchronize()
    m = c.M if c.m_device is None else c.m_device
    fr = V.fractions(pf, sf, r, rows=m)
    observed(f"vfe eval [{name}] M={c.M} P={c.P}: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, (name, fr)
    assert torch.equal(mask.view(c.M, c.P)[:m].double(), r["mask"][:m]), name
    if name == "floor_decides":          # from the reference alone: the padded slot decides both maxes somewhere in every pillar
        assert bool(r["pad_wins_xmax"].any(1).all()) and bool(r["pad_wins_out"].any(1).all())
    if name == "floor_must_not_apply":
        assert not bool(r["pad_wins_xmax"].any()) and not bool(r["pad_wins_out"].any())


def _buffers(M, P):
    return {"pf": torch.full((M * 64 + GUARD,), SENTINEL, device=DEV), "sf": torch.full((M * 32 + GUARD,), SENTINEL, device=DEV),
            "mask": torch.full((M * P + GUARD,), SENTINEL, device=DEV)}


def _call(c, b, M=None, P=None, null=None, m_device=None):
    from hvpr_amd._lib import lib
    M, P = c.M if M is None else M, c.P if P is None else P
    ptr = lambda name, t: None if name == null else t.data_ptr()
    g = V.GRIDS[c.grid]
    return lib().hvpr_pillar_vfe_fwd_f32(ptr("voxels", c.voxels), ptr("num", c.num), ptr("coords", c.coords), M, P,
                                         None if m_device is None else m_device.data_ptr(), *[float(v) for v in g["vs"]],
                                         *[float(v) for v in V.offsets_of(c.grid)], *[ptr(k, getattr(c, k)) for k in V.WEIGHTS],
                                         ptr("pf", b["pf"]), ptr("sf", b["sf"]), ptr("mask", b["mask"]), kernels._stream())


def test_rows_at_or_past_m_device_keep_the_sentinel(observed):
    c = V.case("m_device_below_M").to(DEV)
    r = V.reference(c)
    m = c.m_device
    b = _buffers(c.M, c.P)
    assert _call(c, b, m_device=torch.tensor([m], dtype=torch.int32, device=DEV)) == OK
    torch.cuda.synchronize()
    for k, w in (("pf", 64), ("sf", 32), ("mask", c.P)):
        assert bool((b[k][m * w:] == SENTINEL).all()), k
    fr = V.fractions(b["pf"][:m * 64].view(m, 64), b["sf"][:m * 32].view(m, 32), r, rows=m)
    observed(f"vfe eval [m_device {m} of {c.M}, C entry point]: max err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, fr
    assert torch.equal(b["mask"][:m * c.P].view(m, c.P).double(), r["mask"][:m])
    full = _buffers(c.M, c.P)           # and without m_device every row is written, nothing past the end
    assert _call(c, full) == OK
    torch.cuda.synchronize()
    for k, w in (("pf", 64), ("sf", 32), ("mask", c.P)):
        assert bool((full[k][c.M * w:] == SENTINEL).all()) and not bool((full[k][:c.M * w] == SENTINEL).any()), k
        assert torch.equal(full[k][:m * w], b[k][:m * w]), k


REFUSALS = {
    "P_0": (dict(P=0), INVALID),
    "M_negative": (dict(M=-1), INVALID),
    "P_33": (dict(P=33), UNSUPPORTED),
    "null_w1": (dict(null="w1"), INVALID),
    "null_bs0": (dict(null="bs0"), INVALID),
    "null_pillar_features": (dict(null="pf"), INVALID),
    "M_0": (dict(M=0), OK),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_vfe_refuses_without_a_launch(name):
    over, status = REFUSALS[name]
    c = V.case("P5").to(DEV)
    b = _buffers(c.M, c.P)
    assert _call(c, b, **over) == status
    torch.cuda.synchronize()
    for k, v in b.items():
        assert bool((v == SENTINEL).all()), (name, k)


# ------------------------------------------------------------------------------------------------ packed form
_SHARED = {}


def _shared():
    if not _SHARED:
        _SHARED["folded"] = {k: v.to(DEV) for k, v in V.weights(5).items()}
        _SHARED["floor"] = {k: v.to(DEV) for k, v in V.weights(5, floor=True).items()}
        _SHARED["bank"] = torch.from_numpy(np.random.default_rng(40).uniform(-0.125, 0.125, (2000, 64)).astype(np.float32)).to(DEV)
    return _SHARED


PROD_KEYS = ("coords", "num_points", "pillar_features", "pillar_scale_features", "memory_features")


def _encode(tp, offs, B, P, max_voxels, cap_mode, ws, folded, index_mode, want):
    r = kernels.encode_fwd(tp, offs, B, RNG, VS, GRID, P, max_voxels, ws, folded, OFF, _shared()["bank"], 20, xyz_col=1, cap_mode=cap_mode,
                           want_voxels=want, want_mask=want, index_mode=index_mode)
    torch.cuda.synchronize()
    return r


def _production_equals_full(tp, offs, B, P, max_voxels, cap_mode, ws, folded, index_mode):
    """Item 3 -> the call with both optional outputs on, and the live pillar count."""
    full = _encode(tp, offs, B, P, max_voxels, cap_mode, ws, folded, index_mode, True)
    prod = _encode(tp, offs, B, P, max_voxels, cap_mode, ws, folded, index_mode, False)
    assert prod["voxels"] is None and prod["pillar_mask"] is None
    assert torch.equal(prod["voxel_offsets"], full["voxel_offsets"])
    m = int(full["voxel_offsets"][B])
    for k in PROD_KEYS:
        assert torch.equal(prod[k][:m], full[k][:m]), (k, "differs without the voxels / mask outputs")
    assert torch.equal(prod["spatial"], full["spatial"]) and torch.equal(prod["spatial_scale"], full["spatial_scale"])
    return full, m


def _packed(pts, offs, P, max_voxels, cap_mode, want_counts, index_mode, observed, tag, floor=False):
    S = _shared()
    folded = S["floor" if floor else "folded"]
    B = len(offs) - 1
    tp, to = torch.from_numpy(pts).to(DEV), torch.from_numpy(offs).to(DEV)
    ws = kernels.VoxelizeWorkspace(B, len(pts), GRID, DEV)
    v, c, n, vo = kernels.voxelize(tp, to, B, RNG, VS, GRID, P, max_voxels, ws, xyz_col=1, cap_mode=cap_mode)
    md = vo[B:B + 1]
    pf, sf, mask = kernels.pillar_vfe_fwd(v, n, c, folded, VS, OFF, m_device=md)
    mem, sp, sc = kernels.memory_scatter_fwd(pf, sf, c, S["bank"], 20, B, GRID[0], GRID[1], kernels.scatter_workspace(B, GRID[0], GRID[1], DEV),
                                             m_device=md)
    full, m = _production_equals_full(tp, to, B, P, max_voxels, cap_mode, ws, folded, index_mode)         # item 3
    assert m == len(want_counts) == int(vo[B]) and full["num_points"][:m].tolist() == list(want_counts), (tag, full["num_points"][:m].tolist())
    assert torch.equal(full["voxel_offsets"], vo)
    for key, ref in (("voxels", v), ("coords", c), ("num_points", n), ("pillar_features", pf), ("pillar_scale_features", sf),
                     ("pillar_mask", mask), ("memory_features", mem)):                                     # item 1
        assert torch.equal(full[key][:m], ref[:m]), (tag, key)
    assert torch.equal(full["spatial"], sp) and torch.equal(full["spatial_scale"], sc), tag
    raw = V.Raw(full["voxels"][:m], full["num_points"][:m], full["coords"][:m], folded, VS, OFF)          # item 2
    r = V.reference(raw)
    fr = V.fractions(full["pillar_features"][:m], full["pillar_scale_features"][:m], r)
    observed(f"vfe eval packed [{tag}, index_mode {index_mode}] {m} pillars: max err / bound " + ", ".join(f"{k} {x:.4f}" for k, x in fr.items()))
    assert max(fr.values()) <= 1.0, (tag, fr)
    assert torch.equal(full["pillar_mask"][:m].view(m, P).double(), r["mask"]), tag
    # the canvases hold the same rows at the pillars' cells
    cl = full["coords"][:m].long()
    assert torch.equal(full["spatial"][cl[:, 0], :64, cl[:, 2], cl[:, 3]], full["pillar_features"][:m])
    assert torch.equal(full["spatial_scale"][cl[:, 0], :, cl[:, 2], cl[:, 3]], full["pillar_scale_features"][:m])
    return r


@pytest.mark.parametrize("index_mode", [0, 1])
@pytest.mark.parametrize("interleave", [False, True], ids=["in_order", "interleaved"])
@pytest.mark.parametrize("name", list(V.SEQUENCES))
def test_packed_sequence(name, interleave, index_mode, observed):
    s = V.SEQUENCES[name]
    pts, offs = V.clouds(s["frames"], seed=3, interleave=interleave)
    want = [min(k, s["P"]) for f in s["frames"] for k in f]
    _packed(pts, offs, s["P"], 40000, 0, want, index_mode, observed, name + ("/interleaved" if interleave else ""))


@pytest.mark.parametrize("index_mode", [0, 1])
def test_packed_floor_inside_a_shared_pass(index_mode, observed):
    """The floor weights (b0 = 2 where every live point has y0 = 0) in the packed form: [3, 32, 1] a padded pillar, a full one in a pass
    of its own and a padded one in the next window; [16, 16] two full pillars in one pass; [5, 4, 3, 2, 1] five padded ones in one
    pass.  From the reference alone: the padded slot wins x_max in every short pillar and in no full one."""
    for counts in ([3, 32, 1], [16, 16], [5, 4, 3, 2, 1]):
        pts, offs = _far_cloud(counts)
        r = _packed(pts, offs, 32, 40000, 0, counts, index_mode, observed, f"floor {counts}", floor=True)
        short = torch.tensor(counts, device=DEV) < 32
        assert bool(r["pad_wins_xmax"][short].any(1).all()) and not bool(r["pad_wins_xmax"][~short].any())


def _far_cloud(counts):
    """clouds() with every voxel in a cell of x >= 100 (16 m out and more), distinct cells in a row of the grid."""
    rng = np.random.default_rng(len(counts))
    rows = []
    for j, k in enumerate(counts):
        u = 0.1 + 0.8 * rng.random((k, 3))
        p = np.zeros((k, 5))
        p[:, 1] = G["lo"][0] + (100 + 7 * j + u[:, 0]) * G["vs"][0]
        p[:, 2] = G["lo"][1] + (30 + u[:, 1]) * G["vs"][1]
        p[:, 3] = G["lo"][2] + u[:, 2] * G["vs"][2]
        p[:, 4] = rng.random(k)
        rows.append(p)
    pts = np.concatenate(rows).astype(np.float32)
    return pts, np.asarray([0, len(pts)], np.int32)


@pytest.mark.parametrize("index_mode", [0, 1])
def test_packed_v1_cap_drops_points_of_a_kept_voxel(index_mode, observed):
    """cap_mode = 1: the cap is reached while voxels 0 and 1 still receive points; their arena segments hold 7 and 3 columns of which 3
    and 2 are live (floor_here at the first live column, n < cn)."""
    pts, offs, cap, live = V.capped_cloud()
    _packed(pts, offs, 32, cap, 1, live, index_mode, observed, "v1 cap")


@pytest.mark.parametrize("index_mode", [0, 1])
def test_production_form_on_natural_frames(index_mode):
    """Item 3 on a shuffled KITTI-like frame (most segments out of index order) and on a ragged three-frame batch with an empty frame."""
    S = _shared()
    for frames in ([synthetic.hvpr_frame(1, shuffle=True)],
                   [synthetic.hvpr_frame(2)[:5000], np.zeros((0, 4), np.float32), synthetic.hvpr_frame(4, shuffle=True)[:3000]]):
        pts = np.concatenate([np.concatenate([np.full((len(f), 1), b, np.float32), f], 1) for b, f in enumerate(frames)], 0)
        offs = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
        B = len(frames)
        ws = kernels.VoxelizeWorkspace(B, len(pts), GRID, DEV)
        full, m = _production_equals_full(torch.from_numpy(pts).to(DEV), torch.from_numpy(offs).to(DEV), B, 32, 16000, 0, ws, S["folded"], index_mode)
        assert m > 1000
