"""get_infos' num_points_in_gt in numpy, the KITTI trees the tests read, and fixture G23.

The count (kitti_dataset.py:171-184) is restated over two pieces that are pinned elsewhere: the FOV decision with the kernels'
operations (batch_loader_cases.fov_flag: float32, left to right, no fused multiply-add) and the box decision of
hvpr_amd.gt_sampling.points_in_boxes_cpu on the float32 boxes (the reference builds its corners from `.float()` boxes, and the
hull of a cuboid's corners is the cuboid).  tests/test_kitti_infos_host.py pins the restatement to fixture G23, the reference's own
get_infos with scipy's Delaunay, on the CPU; the GPU machine has no reference, so this is the checker there.

Margin rule.  The reference's BLAS products, Qhull's tolerance and the device's cosf may all round otherwise than the checker, so
a decision is compared only where it is decisive.  Every generated cloud is cleaned BEFORE any side sees it: no point within
MARGIN (1e-3 m) of a face of any box of its frame (augment_cases.point_face_distance, float64), no projected pixel within 1e-3 px
of an image border, no rect depth within 1e-3 m of 0 (the rule of tests/golden/make_golden_batch.py).  The generators clean with
twice the margin against float64 boxes; the assertions use MARGIN against the boxes as the infos hold them.
"""
import os
import struct
import zlib
from pathlib import Path

import numpy as np

import augment_cases as AC
import batch_loader_cases as BC
import gt_database_cases as GC

MARGIN = 1e-3

P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float64)
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
               [0.007402527, 0.004351614, 0.9999631]], np.float64)
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]], np.float64)


def make_calib(k=0):
    """A KITTI-like calibration; k > 0 moves the focal length, the principal point and the lidar's mount a little."""
    p2, v2c = P2.copy(), V2C.copy()
    p2[0, 0] = p2[1, 1] = P2[0, 0] - 3.25 * k
    p2[0, 2] += 2.5 * k
    p2[1, 2] -= 1.75 * k
    v2c[:, 3] += [0.01 * k, -0.005 * k, 0.02 * k]
    return {"P2": p2.astype(np.float32), "P3": (p2 + [[0, 0, 0, -380.0], [0, 0, 0, 0], [0, 0, 0, 0]]).astype(np.float32),
            "R0": R0.astype(np.float32), "Tr_velo2cam": v2c.astype(np.float32)}


# ------------------------------------------------------------------------------------------------ the count, in numpy
def project64(xyz, calib):
    """(u, v, rect depth rz, depth) in float64 from the float32 calibration words."""
    v2c, r0, p2 = (np.asarray(calib[k], np.float64) for k in ("Tr_velo2cam", "R0", "P2"))
    hom = np.concatenate([np.asarray(xyz, np.float64)[:, :3], np.ones((len(xyz), 1))], axis=1)
    rect = hom @ (v2c.T @ r0.T)
    img = np.concatenate([rect, np.ones((len(xyz), 1))], axis=1) @ p2.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return img[:, 0] / rect[:, 2], img[:, 1] / rect[:, 2], rect[:, 2], img[:, 2] - p2[2, 3]


def fov_margin(points, calib, image_shape):
    """Per point the smallest distance (px or m) to a border of the FOV decision."""
    u, v, rz, depth = project64(points, calib)
    h, w = float(image_shape[0]), float(image_shape[1])
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.minimum.reduce([np.abs(rz), np.abs(depth), np.abs(u), np.abs(u - w), np.abs(v), np.abs(v - h)]), nan=0.0)


def box_margin(points, boxes):
    """Per point the smallest distance to a face of any of `boxes` (float64)."""
    d = np.full((len(points),), np.inf)
    for b in np.asarray(boxes, np.float64).reshape(-1, 7):
        d = np.minimum(d, AC.point_face_distance(points, b)[0])
    return d


def clean(points, boxes64, calib, image_shape, margin=2 * MARGIN):
    ok = (fov_margin(points, calib, image_shape) >= margin) & (box_margin(points, boxes64) >= margin)
    return np.ascontiguousarray(points[ok])


def margins_hold(points, boxes, calib, image_shape):
    """The assertion of the margin rule, against the boxes as the float32 test sees them."""
    if not len(points):
        return True
    b32 = np.asarray(boxes, np.float64).reshape(-1, 7).astype(np.float32)
    return bool(fov_margin(points, calib, image_shape).min() >= MARGIN and box_margin(points, b32).min() >= MARGIN)


def count_host(points, boxes, calib, image_shape):
    """(n,) int32: per box the points in the camera's view and inside it; -> also the number of points in view."""
    from hvpr_amd import gt_sampling
    pts = np.asarray(points, np.float32)
    fov = BC.fov_flag(pts, calib, image_shape) if len(pts) else np.zeros((0,), bool)
    b32 = np.asarray(boxes, np.float64).reshape(-1, 7).astype(np.float32)
    if not len(b32):
        return np.zeros((0,), np.int32), int(fov.sum())
    inside = gt_sampling.points_in_boxes_cpu(np.ascontiguousarray(pts[fov][:, 0:3]), b32)
    return np.asarray(inside).reshape(len(b32), -1).sum(axis=1).astype(np.int32), int(fov.sum())


def plain_count_host(points, boxes):
    """The database's count (count_points_in_boxes): the same box test over EVERY point of the frame."""
    from hvpr_amd import gt_sampling
    b32 = np.asarray(boxes, np.float64).reshape(-1, 7).astype(np.float32)
    if not len(b32):
        return np.zeros((0,), np.int32)
    inside = gt_sampling.points_in_boxes_cpu(np.ascontiguousarray(np.asarray(points, np.float32)[:, 0:3]), b32)
    return np.asarray(inside).reshape(len(b32), -1).sum(axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ kernel-level cases
def view_boxes(m, seed=0):
    """gt_database_cases.grid_boxes with the rows centred on the camera's axis (the grid starts at y = -40, out of view up to
    x = 47 m): some boxes in view, some across a border, some outside."""
    names, boxes = GC.grid_boxes(m, seed=seed)
    boxes[:, 1] += 40.0 - 3.0 * ((max(m, 1) - 1) // 16)
    return names, boxes


def make_case(point_counts, box_counts, seed=0, F=4, calib_of=lambda i: make_calib(i % 3), shape_of=lambda i: (375 - i % 3, 1242 - 9 * (i % 3))):
    """-> per frame a dict(points (n, F) float32 margin-clean, boxes (m, 7) float64, calib, image_shape): frame i has
    point_counts[i] points and box_counts[i] boxes on gt_database_cases' grid, which reaches out of the camera's view."""
    frames = []
    for i, (n, m) in enumerate(zip(point_counts, box_counts)):
        _, boxes = view_boxes(m, seed=seed * 1000 + i)
        calib, shape = calib_of(i), np.array(shape_of(i), np.int32)
        pts = clean(GC.frame_points(n + n // 8 + 64, boxes, seed * 1000 + 500 + i, F), boxes, calib, shape)
        assert len(pts) >= n, (len(pts), n)
        frames.append({"points": np.ascontiguousarray(pts[:n]), "boxes": boxes, "calib": calib, "image_shape": shape})
        assert margins_hold(frames[-1]["points"], boxes, calib, shape)
    return frames


def counts_of(frames):
    """-> (per frame the (m,) int32 counts, per frame the points in view)."""
    r = [count_host(f["points"], f["boxes"], f["calib"], f["image_shape"]) for f in frames]
    return [c for c, _ in r], [v for _, v in r]


# ------------------------------------------------------------------------------------------------ a KITTI tree
def png_bytes(h, w):
    """A valid 8-bit grey PNG of h x w zeros."""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(b"\x00" * ((w + 1) * h), 9)) + chunk(b"IEND", b""))


def calib_text(calib):
    def row(key, m):
        return key + ": " + " ".join("%.12e" % v for v in np.asarray(m, np.float64).reshape(-1))
    return "\n".join([row("P0", calib["P2"] * np.array([1, 1, 1, 0])), row("P1", calib["P3"]), row("P2", calib["P2"]), row("P3", calib["P3"]),
                      row("R0_rect", calib["R0"]), row("Tr_velo_to_cam", calib["Tr_velo2cam"]),
                      row("Tr_imu_to_velo", np.eye(3, 4))]) + "\n"


def label_line(name, box_lidar, calib, truncated=0.0, occluded=0, bbox=(100.0, 100.0, 200.0, 150.0), score=None):
    """A label_2 line for a lidar box (x, y, z, dx, dy, dz, heading): the camera fields with two decimals, as KITTI writes them."""
    b = np.asarray(box_lidar, np.float64)
    v2c, r0 = np.asarray(calib["Tr_velo2cam"], np.float64), np.asarray(calib["R0"], np.float64)
    loc = np.array([b[0], b[1], b[2] - b[5] / 2, 1.0]) @ (v2c.T @ r0.T)
    ry = -b[6] - np.pi / 2
    words = [name, "%.2f" % truncated, "%d" % occluded, "%.2f" % 0.25] + ["%.2f" % v for v in bbox]
    words += ["%.2f" % v for v in (b[5], b[4], b[3], loc[0], loc[1], loc[2], ry)]
    if score is not None:
        words.append("%.4f" % score)
    return " ".join(words)


DONTCARE_LINE = "DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10"


def label_boxes64(text, calib):
    """The lidar boxes of a label file's real objects, in float64 from the file's numbers (what the generators clean against; the
    infos' own boxes went through float32 and differ by about 1e-5 m)."""
    v2c, r0 = np.eye(4), np.eye(4)
    v2c[:3], r0[:3, :3] = np.asarray(calib["Tr_velo2cam"], np.float64), np.asarray(calib["R0"], np.float64)
    inv = np.linalg.inv((r0 @ v2c).T)
    out = []
    for line in text.splitlines():
        w = line.strip().split(" ")
        if w[0] == "DontCare":
            continue
        h, wd, l, x, y, z, ry = (float(v) for v in w[8:15])
        c = np.array([float(np.float32(x)), float(np.float32(y)), float(np.float32(z)), 1.0]) @ inv
        out.append([c[0], c[1], c[2] + h / 2, l, wd, h, -(np.pi / 2 + ry)])
    return np.asarray(out, np.float64).reshape(-1, 7)


def tree_files(frames, splits):
    """{relative path: bytes} of a KITTI directory.  frames: dicts with id, split ('train' / 'val' / 'test'), calib, image_shape,
    points, and for the labelled ones label (text), optionally plane (4 floats)."""
    files = {}
    for s, ids in splits.items():
        files["ImageSets/%s.txt" % s] = ("".join(i + "\n" for i in ids)).encode()
    for f in frames:
        d = "testing" if f["split"] == "test" else "training"
        files["%s/calib/%s.txt" % (d, f["id"])] = calib_text(f["calib"]).encode()
        files["%s/image_2/%s.png" % (d, f["id"])] = png_bytes(int(f["image_shape"][0]), int(f["image_shape"][1]))
        files["%s/velodyne/%s.bin" % (d, f["id"])] = np.ascontiguousarray(f["points"], np.float32).tobytes()
        if f.get("label") is not None:
            files["%s/label_2/%s.txt" % (d, f["id"])] = f["label"].encode()
        if f.get("plane") is not None:
            files["%s/planes/%s.txt" % (d, f["id"])] = ("# Plane\nWidth 4\nHeight 1\n" + " ".join("%.6e" % v for v in f["plane"]) + "\n").encode()
    return files


def write_tree(root, files):
    for rel, blob in files.items():
        p = Path(root) / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(blob)


def labelled_frames(point_counts, box_counts, seed=0, trailing_dontcare=1):
    """`make_case` as a tree of train frames with labels: -> (frames for tree_files, splits).  The clouds are cleaned against
    the boxes the label text gives, not the generator's."""
    frames = []
    for i, (n, m) in enumerate(zip(point_counts, box_counts)):
        names, boxes = view_boxes(m, seed=seed * 1000 + i)
        calib, shape = make_calib(i % 3), np.array((375 - i % 3, 1242 - 9 * (i % 3)), np.int32)
        lines = [label_line(nm, b, calib, bbox=(100.0 + k, 100.0, 180.0 + k, 160.0)) for k, (nm, b) in enumerate(zip(names, boxes))]
        lines += [DONTCARE_LINE % (10.0, 20.0, 30.0 + k, 40.0) for k in range(trailing_dontcare if i % 2 == 0 else 0)]
        if not lines:
            lines = [DONTCARE_LINE % (10.0, 20.0, 30.0, 40.0)]
        label = "\n".join(lines) + "\n"
        b64 = label_boxes64(label, calib)
        pts = clean(GC.frame_points(n + n // 8 + 64, boxes, seed * 1000 + 500 + i, 4, quantum=1.0 / 256), b64, calib, shape)
        assert len(pts) >= n
        frames.append({"id": "%06d" % (seed * 100 + i), "split": "train", "calib": calib, "image_shape": shape,
                       "points": np.ascontiguousarray(pts[:n]), "label": label, "plane": [0.01, -1.0, 0.02, 1.65] if i % 2 else None})
    return frames, {"train": [f["id"] for f in frames], "val": [], "test": []}


# ------------------------------------------------------------------------------------------------ infos, flat
def flatten_info(info, prefix=""):
    """[(path, value)] of a nested info dict, in key order."""
    out = []
    for k, v in info.items():
        out.extend(flatten_info(v, prefix + k + "/") if isinstance(v, dict) else [(prefix + k, v)])
    return out


def assert_same_infos(got, want, centre_tol=1e-4):
    """Keys and their order at every level, value types, dtypes, shapes, and the values bit for bit, except the three centre
    columns of gt_boxes_lidar: within `centre_tol` m (they pass through a float32 4 x 4 inverse and a 4-term float32 product of
    values <= 100 m: about 16 * 2^-24 * 100 = 1e-4, and LAPACK builds may round differently)."""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        fg, fw = flatten_info(g), flatten_info(w)
        assert [k for k, _ in fg] == [k for k, _ in fw], ([k for k, _ in fg], [k for k, _ in fw])
        for (k, a), (_, b) in zip(fg, fw):
            assert type(a).__name__ == type(b).__name__, (k, type(a), type(b))
            if not isinstance(b, np.ndarray):
                assert a == b, (k, a, b)
                continue
            assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
            if k == "annos/gt_boxes_lidar":
                assert a[:, 3:].tobytes() == b[:, 3:].tobytes(), k
                assert a.shape[0] == 0 or np.abs(a[:, :3] - b[:, :3]).max() <= centre_tol, (k, np.abs(a[:, :3] - b[:, :3]).max())
            elif a.dtype.kind == "U":
                assert a.tolist() == b.tolist(), k
            else:
                assert a.tobytes() == b.tobytes(), (k, a, b)


# ------------------------------------------------------------------------------------------------ fixture G23
SPLITS = ("train", "val", "test")


def g23():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_kitti_infos.npz"), allow_pickle=False)


def g23_tree(z):
    blob, off = z["tree.bytes"].tobytes(), z["tree.off"]
    return {str(p): blob[off[i]: off[i + 1]] for i, p in enumerate(z["tree.paths"])}


def g23_infos(z, split):
    """The reference's get_infos of a split ('trainval' = train + val), rebuilt with its value types."""
    if split == "trainval":
        return g23_infos(z, "train") + g23_infos(z, "val")
    infos = []
    for i in range(int(z["infos.%s.n" % split])):
        p, info = "infos.%s.%d." % (split, i), {}
        for path, tname in zip(z[p + "keys"], z[p + "types"]):
            v = z[p + str(path)]
            v = {"int": int, "str": str}[str(tname)](v) if str(tname) in ("int", "str") else v
            assert type(v).__name__ == str(tname), (path, tname)
            node, parts = info, str(path).split("/")
            for part in parts[:-1]:
                node = node.setdefault(part, {})
            node[parts[-1]] = v
        infos.append(info)
    return infos


def g23_store(out, split, infos):
    out["infos.%s.n" % split] = np.array(len(infos), np.int64)
    for i, info in enumerate(infos):
        p, flat = "infos.%s.%d." % (split, i), flatten_info(info)
        out[p + "keys"] = np.array([k for k, _ in flat])
        out[p + "types"] = np.array([type(v).__name__ for _, v in flat])
        for k, v in flat:
            assert isinstance(v, (int, str, np.ndarray)) and not isinstance(v, bool), (k, type(v))
            out[p + k] = np.asarray(v)


def g23_frame_inputs(z, split):
    """Per info of a labelled split: (points, calib as the reader gives it, image_shape) from the tree's own bytes."""
    tree, out = g23_tree(z), []
    for info in g23_infos(z, split):
        idx = info["point_cloud"]["lidar_idx"]
        pts = np.frombuffer(tree["training/velodyne/%s.bin" % idx], np.float32).reshape(-1, 4)
        rows = [np.array(line.split(" ")[1:], np.float32) for line in tree["training/calib/%s.txt" % idx].decode().splitlines()]
        calib = {"P2": rows[2].reshape(3, 4), "R0": rows[4].reshape(3, 3), "Tr_velo2cam": rows[5].reshape(3, 4)}
        out.append((pts, calib, info["image"]["image_shape"]))
    return out
