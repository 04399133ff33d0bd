"""Plain PointPillars: what the host and GPU tests (test_pointpillar_host.py, test_gpu_pointpillar.py) and the G28 maker share.

pfn64 restates hvpr_pillar_vfe_plain_fwd_f32 (PillarVFE.forward, pillar_vfe.py:94-124, one folded PFN layer) in float64 on the SAME
float32 inputs the kernel gets (voxels, folded w / b, voxel size and offsets as float32 words) and returns, next to the output, the
bound |kernel - float64| may reach by rounding alone.  With u = 2^-24 and gamma(k) = k u / (1 - k u) (k roundings in a chain):

    mean     S_j = sum over the P slots of v[p, j], in any order: |S^ - S| <= gamma(P - 1) A_j, A_j = sum_p |v[p, j]|; one more
             rounding for the quotient by float(n) (exact for n <= 2^24):       E_mean_j = gamma(P) A_j / n
    cluster  fl(v - m^):   E_mean_j + u |v - m^| <= (1 + u) E_mean_j + u |v - m|
    centre   c^ = fl(fl(cell * vs) + off), the cell index exact: |c^ - c| <= gamma(2) (|cell vs| + |off|); then fl(v - c^):
                                                                                (1 + u) gamma(2) (|cell vs| + |off|) + u |v - c|
    mask     a product with 1.0 or 0.0: exact.  The four raw features are the inputs: exact.  A padded slot's ten features are zeros.
    layer    the bias and ten products summed in sequence, fused or not: a term passes through at most 11 roundings, so with
             E_k the error of feature k from above
                 E_y[p, c] = gamma(11) (|b_c| + sum_k |w_ck| (|f_k| + E_k)) + sum_k |w_ck| E_k   (+ 11 * 2^-126 for flushed products)
    relu and the maximum over the slots are 1-Lipschitz:                        bound[m, c] = max over ALL P slots of E_y[p, c]

No constant is fitted; test_pointpillar_host.py shows on the CPU that plain float32 arithmetic uses a small part of the bound."""
import os

import numpy as np

U = 2.0 ** -24
TINY_RANGE = [0, -5.12, -3, 10.24, 5.12, 1]            # 64 x 64 pillars of 0.16 m, head 32 x 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_pointpillar.npz")


def gamma(k):
    return k * U / (1.0 - k * U)


def f32_words(values):
    """The float32 words a list of Python floats becomes at the C boundary, as float64."""
    return np.asarray(values, np.float32).astype(np.float64)


def offsets_of(voxel_size, point_cloud_range):
    """PillarVFE's x / y / z offsets (pillar_vfe.py:79-81), in Python floats as the module computes them."""
    return [float(voxel_size[i]) / 2 + float(point_cloud_range[i]) for i in range(3)]


def pfn64(voxels, num_points, coords, w, b, voxel_size, offsets, rows=4096):
    """-> dict(out (M, C), mask (M, P), y (M, P, C) the per-slot outputs after ReLU, bound (M, C)), all float64.
    voxels (M, P, 4), num_points (M,), coords (M, 4) [b, z, y, x]; w (C, 10), b (C,): the folded layer.  More than `rows` pillars
    are taken in pieces, and y is then left out."""
    M = len(voxels)
    if M > rows:
        parts = [pfn64(voxels[i:i + rows], num_points[i:i + rows], coords[i:i + rows], w, b, voxel_size, offsets, rows)
                 for i in range(0, M, rows)]
        return {k: np.concatenate([p[k] for p in parts]) for k in ("out", "mask", "bound")}
    v = np.asarray(voxels, np.float32).astype(np.float64)
    n = np.asarray(num_points).astype(np.float64)
    cell = np.asarray(coords).astype(np.float64)[:, [3, 2, 1]]                      # x, y, z cell
    w, b = np.asarray(w, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    vs, off = f32_words(voxel_size), f32_words(offsets)
    M, P, _ = v.shape
    live = (np.arange(P)[None, :] < n[:, None]).astype(np.float64)                  # (M, P)
    xyz = v[..., :3]
    mean = xyz.sum(axis=1) / n[:, None]
    A = np.abs(xyz).sum(axis=1)
    cl = xyz - mean[:, None, :]
    ctr = cell * vs + off
    ce = xyz - ctr[:, None, :]
    f = np.concatenate([v, cl, ce], axis=-1) * live[..., None]                      # (M, P, 10)
    e_mean = gamma(P) * A / n[:, None]
    e_cl = ((1 + U) * e_mean[:, None, :] + U * np.abs(cl)) * live[..., None]
    e_ce = ((1 + U) * gamma(2) * (np.abs(cell * vs) + np.abs(off))[:, None, :] + U * np.abs(ce)) * live[..., None]
    E = np.concatenate([np.zeros_like(v), e_cl, e_ce], axis=-1)
    y = np.maximum(f @ w.T + b, 0.0)                                                # (M, P, C)
    aw = np.abs(w).T
    e_y = gamma(11) * (np.abs(b) + (np.abs(f) + E) @ aw) + E @ aw + 11 * 2.0 ** -126
    return {"out": y.max(axis=1), "mask": live, "y": y, "bound": e_y.max(axis=1)}


def pfn32(voxels, num_points, coords, w, b, voxel_size, offsets):
    """The same forward in plain float32 numpy, one rounding per operation, nothing fused -> out (M, C) float32."""
    f4 = np.float32
    v = np.asarray(voxels, f4)
    n = np.asarray(num_points).astype(f4)
    cell = np.asarray(coords).astype(f4)[:, [3, 2, 1]]
    w, b = np.asarray(w, f4), np.asarray(b, f4)
    vs, off = np.asarray(voxel_size, f4), np.asarray(offsets, f4)
    M, P, _ = v.shape
    live = (np.arange(P)[None, :] < n[:, None]).astype(f4)
    xyz = v[..., :3]
    s = np.zeros((M, 3), f4)
    for p in range(P):
        s = s + xyz[:, p]
    mean = s / n[:, None]
    cl = xyz - mean[:, None, :]
    ce = xyz - (cell * vs + off)[:, None, :]
    f = np.concatenate([v, cl, ce], axis=-1) * live[..., None]
    acc = np.broadcast_to(b, (M, P, len(b))).astype(f4)
    for k in range(10):
        acc = acc + f[..., k:k + 1] * w[None, None, :, k]
    assert acc.dtype == f4
    return np.maximum(acc, f4(0)).max(axis=1)


def used_fraction(got, r):
    """max |got - out| / bound over every element (bound > 0 everywhere: it holds the flush term)."""
    return float((np.abs(np.asarray(got, np.float64) - r["out"]) / r["bound"]).max())


def synth_pillars(seed, M, P, voxel_size, point_cloud_range, nx, ny, batch=1, force=True):
    """Random pillars in distinct cells of an nx x ny grid, points inside their cell, zero padded; n in [1, P] with n = 1 and n = P
    forced on the first two rows -> voxels (M, P, 4) f32, num_points (M,) i32, coords (M, 4) i32, rows grouped by frame."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, P + 1, M).astype(np.int32)
    if force and M >= 2:
        n[0], n[1] = 1, P
    bcol = np.sort(rng.integers(0, batch, M))
    counts = np.bincount(bcol, minlength=batch)
    assert counts.max() <= nx * ny, "more pillars in a frame than the grid has cells"
    cells = np.concatenate([rng.permutation(nx * ny)[:c] for c in counts])
    cx, cy = cells % nx, cells // nx
    u = rng.random((M, P, 4))
    vox = np.zeros((M, P, 4), np.float64)
    vox[..., 0] = point_cloud_range[0] + (cx[:, None] + u[..., 0]) * voxel_size[0]
    vox[..., 1] = point_cloud_range[1] + (cy[:, None] + u[..., 1]) * voxel_size[1]
    vox[..., 2] = point_cloud_range[2] + u[..., 2] * voxel_size[2]
    vox[..., 3] = u[..., 3]
    vox *= (np.arange(P)[None, :] < n[:, None])[..., None]
    coords = np.stack([bcol, np.zeros(M, np.int64), cy, cx], axis=1).astype(np.int32)
    return vox.astype(np.float32), n, coords


def folded_layer(seed, c_out):
    """A folded PFN layer by seed: w (c_out, 10) ~ N(0, sqrt(2 / 10)), b ~ N(0, 0.3) -> float32."""
    rng = np.random.default_rng([int(seed), c_out])
    return (rng.normal(0.0, np.sqrt(0.2), (c_out, 10)).astype(np.float32), rng.normal(0.0, 0.3, (c_out,)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ configs and models
def attr(**kw):
    from hvpr_amd.config import AttrDict
    return AttrDict(**kw)


def vfe_cfg(**kw):
    d = dict(NAME="PillarVFE", WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, USE_NORM=True, NUM_FILTERS=[64])
    d.update(kw)
    return attr(**d)


def backbone_cfg(**kw):
    d = dict(NAME="BaseBEVBackbone", LAYER_NUMS=[3, 5, 5], LAYER_STRIDES=[2, 2, 2], NUM_FILTERS=[64, 128, 256],
             UPSAMPLE_STRIDES=[1, 2, 4], NUM_UPSAMPLE_FILTERS=[128, 128, 128])
    d.update(kw)
    return attr(**d)


def grid_cfg(point_cloud_range, voxel_size=None):
    """pointpillar.yaml on another range (and voxel size)."""
    from hvpr_amd import config
    cfg = config.pointpillar_cfg()
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = [float(v) for v in point_cloud_range]
    if voxel_size is not None:
        for p in cfg.DATA_CONFIG.DATA_PROCESSOR:
            if p.NAME == "transform_points_to_voxels":
                p.VOXEL_SIZE = [float(v) for v in voxel_size]
    return cfg


def tiny_cfg():
    return grid_cfg(TINY_RANGE)


def build_model(cfg, seed=0, cls_bias=None, device=None):
    """The detector of `cfg` with synthetic_weights by seed, in eval mode."""
    from hvpr_amd import detector, synthetic_weights
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
    synthetic_weights.load_synthetic(model, seed=seed, cls_bias=cls_bias)
    if device is not None:
        model = model.to(device)
    return model.eval()


def load_det(module, shapes, seed, prefix=""):
    """detparams by name and seed into `module`; `shapes`: {name: shape} as a fixture records them (names carry `prefix`)."""
    import torch
    from detparams import det_state
    own = {k[len(prefix):]: s for k, s in shapes.items() if k.startswith(prefix)}
    state = {k: torch.from_numpy(t) for k, t in det_state({prefix + k: s for k, s in own.items()}, seed).items()}
    missing = module.load_state_dict({k[len(prefix):]: t for k, t in state.items()}, strict=False)
    assert not missing.unexpected_keys and all("num_batches_tracked" in k or k == "global_step" for k in missing.missing_keys), missing
    return module


def recorded_shapes(z, tag):
    return {str(n): tuple(int(v) for v in eval(str(s))) for n, s in zip(z[tag + ".param_names"], z[tag + ".param_shapes"])}


def frame_points(seed, point_cloud_range, batch_index=0):
    """synthetic.kitti_like_frame masked to the range -> (n, 5) float32 [b, x, y, z, r]."""
    from hvpr_amd import synthetic
    pts = synthetic.mask_points_by_range(synthetic.kitti_like_frame(seed), point_cloud_range)
    return np.concatenate([np.full((len(pts), 1), batch_index, np.float32), pts], axis=1).astype(np.float32)
