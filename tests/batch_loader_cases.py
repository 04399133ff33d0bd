"""The whole path of hvpr_amd.batch_loader in numpy, over augment_cases.augment_frame: FOV filter, augmentor, redraw, class
filter, trim, range mask, shuffle, collate.  test_batch_loader_host.py pins it to fixture G22 (the reference's own code, see
tests/golden/make_golden_batch.py) on the CPU; the GPU tests compare the device against the same fixture.

The keep decisions are restated with the kernels' operations (float32, left to right, no fused multiply-add), not with the
reference's BLAS products, whose order is unspecified: G22 keeps every point at least 1e-3 px / 1e-3 m off every border, far
more than either rounding, so all three decide alike.  The draws follow the loader's phases (hvpr_amd/batch_loader.py): the
augmentor draws of every frame of the batch, then each empty frame's redraw chain, then the permutations, each frame from its own
generator."""
import json
import os

import numpy as np

import augment_cases as AC

E24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ fixture access
def g22():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_train_batch.npz"), allow_pickle=False)


def g22_config(z):
    return json.loads(str(z["config"]))


def g22_bank(z, device="cuda:0"):
    return AC.g19_bank(z, json.loads(str(z["prepare"])), device=device)


def g22_frames(z, to_device=None):
    """The dataset's frames as a frame_source serves them."""
    calib = {m: z["calib." + m] for m in ("Tr_velo2cam", "R0", "P2")}
    out = []
    for i in range(int(z["num_frames"])):
        k = f"fr{i}."
        pts = z[k + "points"]
        out.append({"points": to_device(pts) if to_device else pts, "gt_boxes": z[k + "gt_boxes"],
                    "gt_names": [str(n) for n in z[k + "gt_names"]], "image_shape": z[k + "image_shape"],
                    "road_plane": z[k + "road_plane"], "calib": calib, "frame_id": str(i)})
    return out


def g22_generators(z):
    """One generator per batch slot, each in the state the reference's `np.random` had when it reached that frame."""
    B = len(z["train.indices"])
    gens = [np.random.RandomState(int(z["train.seed"]))]
    for b in range(1, B):
        k = f"train.b{b - 1}."
        g = np.random.RandomState(0)
        g.set_state(("MT19937", z[k + "rng_keys"], int(z[k + "rng_pos"][0]), int(z[k + "rng_pos"][1]), float(z[k + "rng_gauss"])))
        gens.append(g)
    return gens


def state_matches(gen, z, b):
    st, k = gen.get_state(), f"train.b{b}."
    return bool(np.array_equal(st[1], z[k + "rng_keys"]) and [st[2], st[3]] == z[k + "rng_pos"].tolist() and
                st[4] == float(z[k + "rng_gauss"]))


# ------------------------------------------------------------------------------------------------ the keep decisions
def _dot4(x, y, z, m, j):
    return ((x * m[0, j] + y * m[1, j]) + z * m[2, j]) + m[3, j]


def fov_flag(points, calib, image_shape):
    """csrc/point_pred.h in numpy float32."""
    V2C, R0, P2 = (np.asarray(calib[k], np.float32) for k in ("Tr_velo2cam", "R0", "P2"))
    a, p = np.dot(V2C.T, R0.T).astype(np.float32), np.ascontiguousarray(P2.T)
    x, y, z = (np.asarray(points[:, j], np.float32) for j in range(3))
    rx, ry, rz = (_dot4(x, y, z, a, j) for j in range(3))
    hx, hy, hz = (_dot4(rx, ry, rz, p, j) for j in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = hx / rz, hy / rz
    depth = hz - p[3, 2]
    assert u.dtype == np.float32 and depth.dtype == np.float32
    return (u >= 0) & (u < np.float32(image_shape[1])) & (v >= 0) & (v < np.float32(image_shape[0])) & (depth >= 0)


def range_flag(points, rng6):
    r = np.asarray(rng6, np.float32)
    return (points[:, 0] >= r[0]) & (points[:, 0] <= r[3]) & (points[:, 1] >= r[1]) & (points[:, 1] <= r[4])


# ------------------------------------------------------------------------------------------------ the path
def _augment(frame, planner, bank, gen, rng6, fov, remove_outside):
    pts = np.asarray(frame["points"], np.float32)
    if fov:
        pts = pts[fov_flag(pts, frame["calib"], frame["image_shape"])]
    names = np.asarray(frame["gt_names"]).astype(str)
    cls = np.array([bank.class_names.index(n) + 1 if n in bank.class_names else 0 for n in names], np.int32)
    plan = planner.plan_frame(frame["gt_names"], frame.get("calib"), frame.get("road_plane"), gen)
    arena, off = bank.host_points()
    r = AC.augment_frame(pts, frame["gt_boxes"], cls, plan, planner.ops, arena, off, bank.obj_box, planner.extra_width, rng6,
                         remove_outside=remove_outside)
    accepted = int(np.sum(r["valid"]))
    # len(data_dict['gt_boxes']) after DataAugmentor.forward: the sampler pops gt_boxes_mask, so with nothing pasted every
    # ground truth counts, trained class or not (database_sampler.py:189)
    r["after_augmentor"] = int((cls > 0).sum()) + accepted if accepted > 0 or planner.sampler_cfg is None else len(cls)
    r["plan"], r["fov_points"] = plan, len(pts)
    return r


def prepare_batch_host(frames, indices, planner, bank, gens, rng6, num_frames, fov=True, mask_range=True, shuffle=True,
                       remove_outside=True):
    """Training.  Returns the collated points (sum M, 1 + F), gt_boxes (B, max_gt, 8) and per slot the frames served, the
    permutation, the counts."""
    B = len(indices)
    slots = [{"items": [int(i)], "r": _augment(frames[i], planner, bank, gens[b], rng6, fov, remove_outside)}
             for b, i in enumerate(indices)]
    for b, s in enumerate(slots):
        while s["r"]["after_augmentor"] == 0:
            new_index = int(gens[b].randint(num_frames))
            s["items"].append(new_index)
            s["r"] = _augment(frames[new_index], planner, bank, gens[b], rng6, fov, remove_outside)
    parts = []
    for b, s in enumerate(slots):
        pts = s["r"]["points"]
        if mask_range:
            pts = pts[range_flag(pts, rng6)]
        s["perm"] = gens[b].permutation(len(pts)) if shuffle else np.arange(len(pts))
        pts = pts[s["perm"]]
        s["points"] = pts
        parts.append(np.concatenate([np.full((len(pts), 1), b, np.float32), pts], axis=1))
    max_gt = max(len(s["r"]["boxes"]) for s in slots)
    gt = np.zeros((B, max_gt, 8), np.float32)
    for b, s in enumerate(slots):
        gt[b, : len(s["r"]["boxes"])] = s["r"]["boxes"]
    return np.concatenate(parts, axis=0), gt, slots


def test_batch_host(frames, indices, class_names, rng6, fov=True, mask_range=True):
    parts, rows = [], []
    for b, i in enumerate(indices):
        fr = frames[i]
        pts = np.asarray(fr["points"], np.float32)
        keep = np.ones((len(pts),), bool)
        if fov:
            keep &= fov_flag(pts, fr["calib"], fr["image_shape"])
        if mask_range:
            keep &= range_flag(pts, rng6)
        pts = pts[keep]
        parts.append(np.concatenate([np.full((len(pts), 1), b, np.float32), pts], axis=1))
        names = np.asarray(fr["gt_names"]).astype(str)
        sel = [j for j, n in enumerate(names) if n in class_names]
        cls = np.asarray([class_names.index(names[j]) + 1 for j in sel], np.float32).reshape(-1, 1)
        rows.append(np.concatenate([np.asarray(fr["gt_boxes"], np.float32).reshape(-1, 7)[sel], cls], axis=1))
    gt = np.zeros((len(indices), max(len(r) for r in rows), 8), np.float32)
    for b, r in enumerate(rows):
        gt[b, : len(r)] = r
    return np.concatenate(parts, axis=0), gt


test_batch_host.__test__ = False


# ------------------------------------------------------------------------------------------------ the comparison with G22
def assert_train_batch_is_g22(z, points, gt_boxes, observed=None, who="restatement"):
    assert_same_batch(z["train.points"], z["train.gt_boxes"], points, gt_boxes, observed, "G22 " + who)


def assert_same_batch(ref_p, ref_b, points, gt_boxes, observed=None, who=""):
    """The assertions both the CPU and the GPU test make.  Bounds (derived in test_gpu_augment.py's docstring, doubled because
    here two roundings of the same exact value are compared, the reference's and ours): a rotated, scaled x or y is within
    3 * 2^-24 (|x| + |y|) scale of the exact value on either side, and |x| + |y| <= sqrt(2) (|x'| + |y'|) / scale', so
    |d| <= 6 * 2^-24 sqrt(2) (|x'| + |y'|); z takes one rounded product of the same float32 factors on both sides:
    |d| <= 2 * 2^-24 |z'|; a heading |d| <= 12 * 2^-24 (|h| + pi/4 + 3 pi); box sizes as z."""
    assert points.shape == ref_p.shape and points.dtype == np.float32, (points.shape, ref_p.shape)
    assert np.array_equal(points[:, 0], ref_p[:, 0]), "batch column"
    assert points[:, 4].tobytes() == ref_p[:, 4].tobytes(), "feature column: kept set and order"
    mag = np.sqrt(2.0) * (np.abs(ref_p[:, 1:2]) + np.abs(ref_p[:, 2:3])).astype(np.float64)
    dxy = np.abs(points[:, 1:3].astype(np.float64) - ref_p[:, 1:3])
    assert (dxy <= 6 * E24 * mag).all(), float((dxy / (E24 * mag)).max())
    dz = np.abs(points[:, 3].astype(np.float64) - ref_p[:, 3])
    assert (dz <= 2 * E24 * np.abs(ref_p[:, 3].astype(np.float64))).all()
    assert gt_boxes.shape == ref_b.shape, (gt_boxes.shape, ref_b.shape)
    assert np.array_equal(gt_boxes[:, :, 7], ref_b[:, :, 7]), "classes and padding"
    bmag = np.sqrt(2.0) * (np.abs(ref_b[:, :, 0:1]) + np.abs(ref_b[:, :, 1:2])).astype(np.float64)
    dbxy = np.abs(gt_boxes[:, :, 0:2].astype(np.float64) - ref_b[:, :, 0:2])
    assert (dbxy <= 6 * E24 * bmag).all()
    ds = np.abs(gt_boxes[:, :, 2:6].astype(np.float64) - ref_b[:, :, 2:6])
    assert (ds <= 2 * E24 * np.abs(ref_b[:, :, 2:6].astype(np.float64))).all()
    dh = np.abs(gt_boxes[:, :, 6].astype(np.float64) - ref_b[:, :, 6])
    assert (dh <= 12 * E24 * (np.abs(ref_b[:, :, 6].astype(np.float64)) + np.pi / 4 + 3 * np.pi) * (ref_b[:, :, 7] > 0)).all()
    if observed is not None:
        observed(f"{who}: x, y within {float((dxy / (E24 * mag + 1e-300)).max()):.2f} of 6 units of 2^-24 sqrt(2)(|x|+|y|); "
                 f"z within {float((dz / (E24 * np.abs(ref_p[:, 3].astype(np.float64)) + 1e-300)).max()):.2f} of 2 units")
