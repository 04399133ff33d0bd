"""The training augmentation restated in plain numpy, written from the reference's text (database_sampler.py:159-200 and
:118-157, augmentor_utils.py:6-78, data_augmentor.py:95-97, box_utils.py:27-71), plus the case generators of the GPU tests.
The GPU machine has no reference: this is the checker there, and tests/test_augment_host.py pins it to fixture G19 first.

Zero / non-zero overlap and inside / outside are decided in float64 by exact-arithmetic-free but margin-guarded tests: every case
made here satisfies `margins_ok` (box pairs separated by >= 0.1 m or overlapping by >= 0.01 m^2, no scene point within 1e-3 m of
a face), so float64 decides them as the fp32 kernels do."""
import numpy as np

PI32, TWO_PI32 = np.float32(np.pi), np.float32(2 * np.pi)
OP_FLIP_X, OP_FLIP_Y, OP_ROTATE, OP_SCALE = 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------ rectangles in float64
def corners_bev(b):
    b = np.asarray(b, np.float64)
    c, s = np.cos(b[6]), np.sin(b[6])
    l = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64) * (b[3:5] / 2)
    return np.stack([l[:, 0] * c - l[:, 1] * s + b[0], l[:, 0] * s + l[:, 1] * c + b[1]], axis=1)      # counter-clockwise


def _clip(poly, a, b):
    """The part of convex `poly` on the left of the line a -> b (Sutherland-Hodgman)."""
    out = []
    n = len(poly)
    for i in range(n):
        p, q = poly[i], poly[(i + 1) % n]
        sp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        sq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
        if sp >= 0:
            out.append(p)
        if (sp >= 0) != (sq >= 0):
            t = sp / (sp - sq)
            out.append(p + t * (q - p))
    return out


def overlap_area(b0, b1):
    poly, clip = list(corners_bev(b0)), corners_bev(b1)
    for i in range(4):
        if not poly:
            return 0.0
        poly = _clip(poly, clip[i], clip[(i + 1) % 4])
    if len(poly) < 3:
        return 0.0
    p = np.asarray(poly)
    return 0.5 * abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - p[:, 1] * np.roll(p[:, 0], -1)))


def _seg_dist(p, a, b):
    d = b - a
    t = np.clip(np.dot(p - a, d) / max(np.dot(d, d), 1e-300), 0.0, 1.0)
    return np.linalg.norm(p - (a + t * d))


def separation(b0, b1):
    """Distance between two rectangles that do not overlap."""
    c0, c1 = corners_bev(b0), corners_bev(b1)
    return min(min(_seg_dist(p, c1[i], c1[(i + 1) % 4]) for p in c0 for i in range(4)),
               min(_seg_dist(p, c0[i], c0[(i + 1) % 4]) for p in c1 for i in range(4)))


def pair_state(b0, b1):
    """(+1 overlapping by >= 0.01 m^2 | 0 separated by >= 0.1 m | None: inside the margin)."""
    a = overlap_area(b0, b1)
    if a >= 0.01:
        return 1
    if a == 0.0 and separation(b0, b1) >= 0.1:
        return 0
    return None


def iou_positive(boxes_a, boxes_b):
    """(n, m) bool: boxes overlap.  Decisive under the margin condition (asserted)."""
    out = np.zeros((len(boxes_a), len(boxes_b)), bool)
    for i, a in enumerate(boxes_a):
        for j, b in enumerate(boxes_b):
            st = pair_state(a, b)
            assert st is not None, ("box pair inside the margin", a, b)
            out[i, j] = st == 1
    return out


def point_face_distance(points, box):
    """Per point: how far it is from the surface of `box` (largest of the three signed face distances, as a magnitude: no more
    than the Euclidean distance), and the inside flag of
    csrc_cpu/gt_sampling.cpp:95-107 (|z - cz| <= dz/2, |x| < dx/2, |y| < dy/2 in the box frame)."""
    p, b = np.asarray(points, np.float64), np.asarray(box, np.float64)
    c, s = np.cos(-b[6]), np.sin(-b[6])
    sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
    lx, ly, lz = sx * c - sy * s, sx * s + sy * c, p[:, 2] - b[2]
    inside = (np.abs(lz) <= b[5] / 2) & (np.abs(lx) < b[3] / 2) & (np.abs(ly) < b[4] / 2)
    d = np.abs(np.maximum(np.maximum(np.abs(lx) - b[3] / 2, np.abs(ly) - b[4] / 2), np.abs(lz) - b[5] / 2))
    return d, inside


def points_inside(points, boxes):
    """(m, n) inside table in float64 (points (n, >=3), boxes (m, 7))."""
    out = np.zeros((len(boxes), len(points)), bool)
    for k, b in enumerate(boxes):
        out[k] = point_face_distance(points, b)[1]
    return out


# ------------------------------------------------------------------------------------------------ the pipeline
def collide(gt_boxes, cand_boxes, group_off, iou=None):
    """database_sampler.py:170-193 -> valid (C,) bool.  `iou(a, b)`: an (n, m) table whose zeros are exact (default: float64)."""
    iou = iou or (lambda a, b: iou_positive(a, b).astype(np.float32))
    existed = np.asarray(gt_boxes, np.float32).reshape(-1, 7)
    valid = np.zeros((len(cand_boxes),), bool)
    for g in range(len(group_off) - 1):
        s = np.asarray(cand_boxes[group_off[g]: group_off[g + 1]], np.float32)
        if len(s) == 0:
            continue
        iou1 = np.asarray(iou(s, existed), np.float32).reshape(len(s), len(existed))
        iou2 = np.array(iou(s, s), np.float32)
        iou2[range(len(s)), range(len(s))] = 0
        iou1 = iou1 if iou1.shape[1] > 0 else iou2
        ok = (iou1.max(axis=1) + iou2.max(axis=1)) == 0
        valid[group_off[g]: group_off[g + 1]] = ok
        existed = np.concatenate((existed, s[ok]), axis=0)
    return valid


def _fma32(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64; the sum is rounded to float64, then to float32
    (a double rounding could differ from a true fma in about one sum in 2^29: no check here asks for bits of x, y)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def transform_points(xyz, ops, xf, dtype, fused=False):
    """Flip / rotate / scale of augmentor_utils.py on (n, 3); c, s, scale are the plan's float32 values, carried in `dtype`.
    fused (float32 only): the second product of the rotation goes into the sum by a fused multiply-add, as the reference's gemm
    over a frame's points does (torch.matmul, 45 rows and more); a frame's few boxes take torch's unfused small-matrix sum."""
    x, y, z = (np.array(xyz[:, k], dtype) for k in range(3))
    c, s, sc = dtype(xf["cos"]), dtype(xf["sin"]), dtype(xf["scale"])
    for op in ops:
        if op == OP_FLIP_X and xf["flip_x"]:
            y = -y
        elif op == OP_FLIP_Y and xf["flip_y"]:
            x = -x
        elif op == OP_ROTATE and fused and dtype is np.float32:
            x, y = _fma32(y, -s, x * c), _fma32(y, c, x * s)
        elif op == OP_ROTATE:
            x, y = x * c + y * (-s), x * s + y * c
        elif op == OP_SCALE:
            x, y, z = x * sc, y * sc, z * sc
    return np.stack([x, y, z], axis=1)


def transform_boxes(boxes, ops, xf, dtype):
    b = np.array(boxes, dtype).reshape(-1, 7)
    b[:, 0:3] = transform_points(b[:, 0:3], ops, xf, dtype)
    h, dims = b[:, 6].copy(), b[:, 3:6].copy()
    for op in ops:
        if op == OP_FLIP_X and xf["flip_x"]:
            h = -h
        elif op == OP_FLIP_Y and xf["flip_y"]:
            h = -(h + dtype(PI32))
        elif op == OP_ROTATE:
            h = h + dtype(np.float32(xf["angle"]))
        elif op == OP_SCALE:
            dims = dims * dtype(xf["scale"])
    p = dtype(TWO_PI32)
    b[:, 6] = h - np.floor(h / p + dtype(0.5)) * p                                  # limit_period(h, 0.5, 2 pi)
    b[:, 3:6] = dims
    return b


def box_corners(boxes, dtype=np.float64):
    """box_utils.py:27-52 -> (n, 8, 3)."""
    b = np.asarray(boxes, dtype).reshape(-1, 7)
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], dtype) / 2
    l = b[:, None, 3:6] * t[None]
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    return np.stack([l[..., 0] * c + l[..., 1] * (-s) + b[:, None, 0], l[..., 0] * s + l[..., 1] * c + b[:, None, 1],
                     l[..., 2] + b[:, None, 2]], axis=2)


def boxes_in_range(boxes, rng6):
    """box_utils.py:55-71, min_num_corners = 1."""
    cn = box_corners(boxes)
    r = np.asarray(rng6, np.float64)
    return ((cn >= r[0:3]) & (cn <= r[3:6])).all(axis=2).sum(axis=1) >= 1


def augment_frame(points, gt_boxes, gt_cls, plan, ops, bank_arena, obj_off, obj_box, extra_width, rng6, remove_outside=True,
                  dtype=np.float32, iou=None, inside=None):
    """One frame through the whole pipeline.  plan: cand_obj, group_off, cand_box, cand_mv, cand_cls, flip_x, flip_y, cos, sin,
    angle, scale.  Returns valid (C,), kept (indices of the scene points that stay), points (M, F), boxes (K, 8), and
    src: per output point (candidate slot or -1, row in the arena or in the scene)."""
    inside = inside or points_inside
    points = np.asarray(points, np.float32)
    gt_boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 7)
    valid = collide(gt_boxes, plan["cand_box"], plan["group_off"], iou)
    vb = np.asarray(plan["cand_box"], np.float32).reshape(-1, 7)[valid]
    large = vb.copy()
    large[:, 3:6] += np.asarray(extra_width, np.float32)[None]
    kept = np.nonzero(inside(points[:, 0:3], large).sum(axis=0) == 0)[0] if len(points) else np.zeros((0,), np.int64)
    parts, src = [], []
    for k in np.nonzero(valid)[0]:
        o = int(plan["cand_obj"][k])
        op = np.array(bank_arena[obj_off[o]: obj_off[o + 1]], np.float32)
        op[:, :3] += np.asarray(obj_box[o], np.float32)[:3]
        op[:, 2] -= np.float32(plan["cand_mv"][k])
        parts.append(op)
        src.extend((int(k), int(r)) for r in range(obj_off[o], obj_off[o + 1]))
    parts.append(points[kept])
    src.extend((-1, int(i)) for i in kept)
    out = np.concatenate(parts, axis=0)
    xyz = transform_points(out[:, 0:3], ops, plan, dtype, fused=True)
    out_pts = np.concatenate([xyz, out[:, 3:].astype(dtype)], axis=1)
    rows = np.concatenate([gt_boxes[np.asarray(gt_cls) > 0], vb], axis=0)
    cls = np.concatenate([np.asarray(gt_cls)[np.asarray(gt_cls) > 0], np.asarray(plan["cand_cls"])[valid]])
    tb = transform_boxes(rows, ops, plan, dtype)
    keep = boxes_in_range(tb, rng6) if remove_outside and len(tb) else np.ones((len(tb),), bool)
    boxes = np.concatenate([tb, cls.astype(dtype)[:, None]], axis=1)[keep]
    return {"valid": valid, "kept": kept, "points": out_pts, "boxes": boxes, "src": src, "boxes_before_trim": tb}


def margins_ok(points, gt_boxes, plan, extra_width, out_boxes, rng6):
    """The condition every case satisfies (asserted where a case is made)."""
    allb = np.concatenate([np.asarray(gt_boxes, np.float64).reshape(-1, 7), np.asarray(plan["cand_box"], np.float64).reshape(-1, 7)])
    for i in range(len(allb)):
        for j in range(i + 1, len(allb)):
            if pair_state(allb[i], allb[j]) is None:
                return False, ("pair", i, j)
    for b in np.asarray(plan["cand_box"], np.float64).reshape(-1, 7):
        e = b.copy()
        e[3:6] += np.asarray(extra_width, np.float64)
        if len(points) and point_face_distance(points, e)[0].min() < 1e-3:
            return False, ("face", b)
    if len(out_boxes):
        cn = box_corners(np.asarray(out_boxes)[:, :7])
        r = np.asarray(rng6, np.float64)
        if min(np.abs(cn - r[0:3]).min(), np.abs(cn - r[3:6]).min()) < 1e-3:
            return False, ("corner",)
        if np.abs(np.abs(np.asarray(out_boxes, np.float64)[:, 6]) - np.pi).min() < 1e-3:
            return False, ("heading",)
    return True, None


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ fixture access
def g19():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_augmentor.npz"), allow_pickle=False)


def g19_config(z, run):
    import json
    return json.loads(str(z[f"run{run}.config"]))


def g19_bank(z, prepare, device="cuda:0"):
    from hvpr_amd.augment import ObjectBank
    off = z["db.point_off"]
    pts = [z["db.points"][off[i]: off[i + 1]] for i in range(len(off) - 1)]
    return ObjectBank.from_arrays([str(n) for n in z["db.names"]], z["db.boxes"], pts, [str(c) for c in z["class_names"]],
                                  num_points_in_gt=z["db.num_points_in_gt"], difficulty=z["db.difficulty"], prepare=prepare,
                                  device=device)


def g19_frames(z, run):
    """[(frame index, dict)] of a run, in the order the reference saw them."""
    out = []
    for f in [int(i) for i in z[f"run{run}.frames"]]:
        k = f"f{f}."
        fr = {"points": z[k + "points"], "gt_boxes": z[k + "gt_boxes"], "gt_names": [str(n) for n in z[k + "gt_names"]]}
        if k + "road_plane" in z.files:
            fr["road_plane"] = z[k + "road_plane"]
            fr["calib"] = {m: z["calib." + m] for m in ("Tr_velo2cam", "R0", "P2")}
        out.append((f, fr))
    return out


# ------------------------------------------------------------------------------------------------ case generators (GPU tests)
CAR = np.array([3.9, 1.6, 1.56], np.float32)


def grid_boxes(n, x0=4.0, y0=-36.0, pitch=6.0, per_row=10, heading=0.3, z=-1.0):
    """n car boxes on a grid, every pair separated by more than a metre."""
    b = np.zeros((n, 7), np.float32)
    for i in range(n):
        b[i] = [x0 + pitch * (i % per_row), y0 + pitch * (i // per_row), z, *CAR, heading + 0.1 * (i % 7)]
    return b


def synthetic_bank_arrays(n_obj, seed=5, max_pts=12, F=4):
    """n_obj objects (names cycle Car / Pedestrian / Cyclist), a few points each inside a 1 m cube around the origin; object 0
    is empty."""
    r = np.random.RandomState(seed)
    names = [["Car", "Pedestrian", "Cyclist"][i % 3] for i in range(n_obj)]
    pts = [np.zeros((0, F), np.float32) if i == 0 else r.uniform(-0.5, 0.5, (1 + r.randint(max_pts), F)).astype(np.float32)
           for i in range(n_obj)]
    return names, pts


def make_plan(cand_obj, cand_box, group_off, cand_cls=None, cand_mv=None, flip_x=False, flip_y=False, angle=0.0, scale=1.0):
    import torch
    a = torch.from_numpy(np.array([angle])).float()
    C = len(cand_obj)
    return {"cand_obj": np.asarray(cand_obj, np.int64), "cand_box": np.asarray(cand_box, np.float32).reshape(-1, 7),
            "group_off": np.asarray(group_off, np.int64),
            "cand_cls": np.ones((C,), np.int32) if cand_cls is None else np.asarray(cand_cls, np.int32),
            "cand_mv": np.zeros((C,), np.float32) if cand_mv is None else np.asarray(cand_mv, np.float32),
            "flip_x": flip_x, "flip_y": flip_y, "angle": angle, "cos": torch.cos(a).numpy()[0], "sin": torch.sin(a).numpy()[0],
            "scale": np.float32(scale)}
