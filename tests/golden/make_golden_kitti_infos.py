"""Generate tests/golden/g23_kitti_infos.npz by running the reference's own KittiDataset.get_infos
(pcdet/datasets/kitti/kitti_dataset.py:119-191) on a throw-away KITTI tree in a temporary directory.

Runs only where the reference is (see make_golden.py, whose loader this script imports and does not edit; the dataset module is
loaded as make_golden_gt_database.py loads it).  What G23 pins is the reference's PYTHON and its numpy / scipy: the label and
calibration parsing, the difficulty rule, every field of an info with its key order, shape and dtype, the float32 inverse behind
gt_boxes_lidar, lidar_to_rect / get_fov_flag, boxes_to_corners_3d and in_hull with scipy's Delaunay as shipped.  Stood in for, in
memory: DatasetTemplate and skimage (as G20 and G21 do).  `io.imread` returns zeros of the PNG's true shape, so the reference's
get_image_shape (an image decode through skimage) stays UNPINNED; the unbound methods are called on a stand-in object that
holds the paths.

Scene: 5 frames, 000000 / 000001 in train, 000002 / 000003 in val, 000004 in test (no label), three calibrations and image
shapes.  000000: four classes, one line with a 16th field, two trailing DontCare rows, a road plane.  000001: a van that
straddles the left image border (its count is strictly smaller than the plain box count: the case that tells get_infos' count
from count_points_in_boxes), a pedestrian inside the van's box with a point both contain, a car behind the camera (count 0 over
points that are inside it).  000002: DontCare rows only, zero real objects.  000003: every level of the difficulty rule, -1
included.  No degenerate box.  Clouds of at most 2 500 points, coordinates multiples of 1/256 m.

Margins, asserted in float64 against the boxes the reference computed: every point at least 1e-3 m from every face of every box
of its frame, at least 1e-3 px from the image borders and 1e-3 m of depth from 0.  They are a property of the generated scene:
nothing the reference counted is left out.

Stored: every file of the tree as bytes; every field of every info with its dtype and type name.  The archive is written with
fixed time stamps: a second run gives the same bytes.
"""
import io
import os
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402
import make_golden_gt_database as MGD  # noqa: E402
import gt_database_cases as GC  # noqa: E402
import kitti_infos_cases as KC  # noqa: E402

SPLITS = {"train": ["000000", "000001"], "val": ["000002", "000003"], "test": ["000004"]}
SHAPES = {"000000": (375, 1242), "000001": (370, 1224), "000002": (376, 1241), "000003": (375, 1242), "000004": (374, 1238)}
CALIB = {"000000": 0, "000001": 1, "000002": 2, "000003": 0, "000004": 1}
N_POINTS = {"000000": 2500, "000001": 2400, "000002": 600, "000003": 2000, "000004": 500}
PLANE = [-7.051e-03, -9.997e-01, -2.292e-02, 1.681e+00]


def labels():
    c0, c1 = KC.make_calib(0), KC.make_calib(1)
    dc = KC.DONTCARE_LINE
    out = {}
    out["000000"] = "\n".join([
        KC.label_line("Car", [12.3, 2.1, -0.92, 3.9, 1.6, 1.56, 0.37], c0, 0.0, 0, (580.0, 170.0, 660.0, 230.0), score=0.8765),
        KC.label_line("Pedestrian", [9.2, -3.1, -0.81, 0.8, 0.6, 1.73, -1.2], c0, 0.1, 1, (800.0, 150.0, 830.0, 240.0)),
        KC.label_line("Cyclist", [18.4, 5.2, -0.85, 1.76, 0.6, 1.73, 2.5], c0, 0.4, 2, (400.0, 160.0, 430.0, 200.0)),
        KC.label_line("Van", [25.1, -6.3, -0.72, 5.0, 2.0, 2.0, -2.9], c0, 0.0, 0, (760.0, 150.0, 840.0, 190.0)),
        dc % (500.0, 160.0, 520.0, 175.0), dc % (100.0, 100.0, 180.0, 180.0)]) + "\n"
    van = np.array([6.5, 5.4, -0.8, 5.0, 2.0, 2.0, 0.3])
    ped = np.concatenate([van[:3] + [0.3, -0.5, 0.05], [0.8, 0.6, 1.73, 0.9]])
    out["000001"] = "\n".join([
        KC.label_line("Van", van, c1, 0.6, 0, (0.0, 150.0, 250.0, 369.0)),
        KC.label_line("Pedestrian", ped, c1, 0.0, 2, (150.0, 140.0, 200.0, 300.0)),
        KC.label_line("Car", [-8.2, 1.1, -0.9, 3.9, 1.6, 1.56, 1.1], c1, 0.0, 3, (300.0, 170.0, 380.0, 200.0))]) + "\n"
    out["000002"] = "\n".join([dc % (10.0, 20.0, 90.0, 60.0), dc % (700.0, 150.0, 720.0, 170.0)]) + "\n"
    out["000003"] = "\n".join([
        KC.label_line("Car", [15.2, -1.3, -0.95, 4.1, 1.7, 1.5, -0.4], c0, 0.0, 0, (600.0, 170.0, 700.0, 215.0)),       # easy
        KC.label_line("Car", [22.6, 4.4, -0.9, 3.7, 1.55, 1.6, 1.9], c0, 0.2, 1, (450.0, 170.0, 520.0, 199.5)),         # moderate
        KC.label_line("Cyclist", [11.1, 3.3, -0.8, 1.7, 0.6, 1.7, 0.05], c0, 0.45, 2, (350.0, 160.0, 400.0, 230.0)),    # hard
        KC.label_line("Pedestrian", [30.7, -8.2, -0.7, 0.7, 0.65, 1.8, -2.2], c0, 0.0, 0, (900.0, 165.0, 910.0, 188.0)),  # height 24
        dc % (1.0, 2.0, 3.0, 4.0)]) + "\n"
    return out, van, ped


def scene():
    lab, van, ped = labels()
    frames = []
    for split, ids in SPLITS.items():
        for k, idx in enumerate(ids):
            calib, shape = KC.make_calib(CALIB[idx]), np.array(SHAPES[idx], np.int32)
            b64 = KC.label_boxes64(lab[idx], calib) if idx in lab else np.zeros((0, 7))
            n = N_POINTS[idx]
            pts = GC.frame_points(n + n // 8 + 64, b64, 2300 + int(idx), quantum=1.0 / 256)
            pts = KC.clean(pts, b64, calib, shape)[:n]
            if idx == "000001":                                                  # a point at a place the van and the pedestrian contain
                pts[7, :3] = np.round(ped[:3] * 256) / 256
            assert len(KC.clean(pts, b64, calib, shape)) == len(pts) == n and np.array_equal(pts[:, :3] * 256, np.round(pts[:, :3] * 256))
            frames.append({"id": idx, "split": split, "calib": calib, "image_shape": shape, "points": pts, "label": lab.get(idx),
                           "plane": PLANE if idx in ("000000", "000003") else None})
    return frames


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def main():
    R = MGD.load_kitti_dataset(MG.load_reference())
    KD = R.kitti_dataset.KittiDataset
    R.kitti_dataset.io.imread = lambda p: np.zeros(SHAPES[Path(p).stem] + (3,), np.uint8)       # the PNG's true shape
    frames = scene()
    files = KC.tree_files(frames, SPLITS)
    tmp = Path(tempfile.mkdtemp(prefix="g23_infos_"))
    KC.write_tree(tmp, files)
    Stand = type("Stand", (), {n: KD.__dict__[n] for n in ("get_lidar", "get_image_shape", "get_label", "get_calib", "get_fov_flag",
                                                            "get_infos")})
    out = {}
    infos = {}
    for split, ids in SPLITS.items():
        ds = Stand()
        ds.split, ds.root_split_path, ds.sample_id_list = split, tmp / ("testing" if split == "test" else "training"), ids
        infos[split] = ds.get_infos(num_workers=1, has_label=split != "test", count_inside_pts=split != "test")
        KC.g23_store(out, split, infos[split])
    paths = sorted(files)
    off = np.zeros((len(paths) + 1,), np.int64)
    off[1:] = np.cumsum([len(files[p]) for p in paths])
    out.update({"tree.paths": np.array(paths), "tree.off": off, "tree.bytes": np.frombuffer(b"".join(files[p] for p in paths), np.uint8)})

    # the coverage the scene is there for, and the margins
    by_id = {f["id"]: f for f in frames}
    levels = set()
    for split in ("train", "val"):
        for info in infos[split]:
            f, a = by_id[info["point_cloud"]["lidar_idx"]], info["annos"]
            assert KC.margins_hold(f["points"], a["gt_boxes_lidar"], f["calib"], f["image_shape"]), f["id"]
            assert tuple(info["image"]["image_shape"]) == SHAPES[f["id"]]
            n_real = a["gt_boxes_lidar"].shape[0]
            assert (a["num_points_in_gt"][n_real:] == -1).all() and (a["name"][n_real:] == "DontCare").all()
            assert n_real == 0 or (np.minimum.reduce(a["gt_boxes_lidar"][:, 3:6], axis=1) > 0.5).all(), "a degenerate box"
            levels |= set(a["difficulty"][:n_real].tolist())
            want, _ = KC.count_host(f["points"], a["gt_boxes_lidar"], f["calib"], f["image_shape"])
            assert np.array_equal(a["num_points_in_gt"][:n_real], want), (f["id"], a["num_points_in_gt"], want)
    assert levels == {0, 1, 2, -1}, levels
    a0, a1, a2 = infos["train"][0]["annos"], infos["train"][1]["annos"], infos["val"][0]["annos"]
    assert a0["name"].tolist()[-2:] == ["DontCare", "DontCare"] and a0["score"][0] == 0.8765 and a0["score"][1] == -1.0
    assert a2["gt_boxes_lidar"].shape == (0, 7) and a2["num_points_in_gt"].tolist() == [-1, -1]
    plain = KC.plain_count_host(by_id["000001"]["points"], a1["gt_boxes_lidar"])
    hull = a1["num_points_in_gt"]
    assert 0 < hull[0] < plain[0], ("the van does not straddle the border", hull, plain)
    assert hull[2] == 0 < plain[2], ("the car behind the camera", hull, plain)
    p7 = by_id["000001"]["points"][7:8]
    assert KC.count_host(p7, a1["gt_boxes_lidar"], by_id["000001"]["calib"], SHAPES["000001"])[0].tolist() == [1, 1, 0], "two boxes"
    path = os.path.join(MG.OUT, "g23_kitti_infos.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes;", len(paths), "files,", int(off[-1]), "bytes of tree; counts",
          [i["annos"]["num_points_in_gt"].tolist() for s in ("train", "val") for i in infos[s]], "plain 000001", plain.tolist())


if __name__ == "__main__":
    main()
