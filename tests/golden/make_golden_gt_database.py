"""Generate tests/golden/g21_gt_database.npz by running the reference's own KittiDataset.create_groundtruth_database
(pcdet/datasets/kitti/kitti_dataset.py:193-243) on a canned scene in a temporary directory.

Runs only where the reference is (see make_golden.py, whose loader this script imports and does not edit).  What G21 pins is
the reference's PYTHON: the loop over frames and boxes, the file names, the float32-minus-float64 move into the box frame, the
record keys, their order and value types, what `used_classes` filters.  Stood in for, in memory: the absent native
points_in_boxes_cpu by hvpr_amd.gt_sampling (as G19 does; it stays UNPINNED), skimage and DatasetTemplate (as G20 does),
`get_lidar` and `root_path` by a stand-in object the unbound method is called on, and the module-level name `Path`, which the
reference's file defines only when it is run as a script (:430).

Scene: 3 frames of 1 500 to 2 500 points with 4, 2 and 6 boxes; float64 centres that are no float32 numbers; two trailing
DontCare names on frame 0; an empty object (frame 2, off the field); a point inside two boxes (frame 1); used_classes without
Van.  Coordinates are multiples of 1/256 m so that the clouds compress.  The margin rule of tests/gt_database_cases.py holds and
is asserted: no point within 1e-3 m of a box face.

Stored: the scene, every record of the pickle with its value types, every file's bytes.
"""
import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402
import augment_cases as AC  # noqa: E402
import gt_database_cases as GC  # noqa: E402
from hvpr_amd import gt_sampling  # noqa: E402

USED_CLASSES = ["Car", "Pedestrian", "Cyclist"]
SPLIT = "train"
N_POINTS = [1500, 2500, 1600]


def load_kitti_dataset(R):
    MG._stub("pcdet.datasets", os.path.join(MG.REF, "pcdet/datasets"))
    MG._stub("pcdet.datasets.kitti", os.path.join(MG.REF, "pcdet/datasets/kitti"))
    sk = MG._stub("skimage")
    sk.io = MG._stub("skimage.io")
    MG._stub("pcdet.datasets.dataset").DatasetTemplate = type("DatasetTemplate", (), {})
    roi = sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    roi.points_in_boxes_cpu = lambda p, b: torch.from_numpy(gt_sampling.points_in_boxes_cpu(p, b))      # :217-219 calls .numpy()
    utils = sys.modules["pcdet.utils"]
    utils.calibration_kitti = MG._load("pcdet.utils.calibration_kitti", "pcdet/utils/calibration_kitti.py")
    utils.object3d_kitti = MG._load("pcdet.utils.object3d_kitti", "pcdet/utils/object3d_kitti.py")
    R.kitti_dataset = MG._load("pcdet.datasets.kitti.kitti_dataset", "pcdet/datasets/kitti/kitti_dataset.py")
    R.kitti_dataset.Path = Path
    return R


def scene():
    infos, clouds = [], {}
    # frame 0: four classes, two trailing DontCare rows
    names, boxes = GC.grid_boxes(4, seed=2100)
    infos.append(GC.make_info("000021", names, boxes, trailing_dontcare=2, seed=2100))
    # frame 1: a pedestrian standing inside a van's box, and a point at a place both contain
    _, b = GC.grid_boxes(2, seed=2101)
    b[0, 3:6], b[1, 0:3], b[1, 3:6] = GC.SIZES["Van"], b[0, 0:3] + [0.3, 0.1, 0.05], GC.PED
    infos.append(GC.make_info("000022", ["Van", "Pedestrian"], b, seed=2101))
    # frame 2: six boxes, the last one off the field: no point
    names, boxes = GC.grid_boxes(6, seed=2102)
    boxes[5, 0:2] += [300.0, 200.0]
    infos.append(GC.make_info("000023", names, boxes, trailing_dontcare=1, seed=2102))
    for k, info in enumerate(infos):
        boxes = info["annos"]["gt_boxes_lidar"]
        pts = GC.frame_points(N_POINTS[k], boxes[:5] if k == 2 else boxes, 2150 + k, quantum=1.0 / 256)   # none near the empty one
        if k == 1:
            shared = np.round(boxes[1, :3] * 256) / 256
            pts[7, :3] = shared
            assert len(GC.clean_points(pts, boxes)) == len(pts)
        clouds[info["point_cloud"]["lidar_idx"]] = pts
        # the scene the issue asks for
        assert not np.array_equal(boxes[:, :3].astype(np.float32).astype(np.float64), boxes[:, :3])
        for b in boxes.astype(np.float32):
            assert AC.point_face_distance(pts, b)[0].min() >= GC.MARGIN
    return infos, clouds


def main():
    R = load_kitti_dataset(MG.load_reference())
    infos, clouds = scene()
    tmp = Path(tempfile.mkdtemp(prefix="g21_db_"))
    info_path = tmp / "kitti_infos_train.pkl"
    with open(info_path, "wb") as f:
        pickle.dump(infos, f)

    class Dataset:
        root_path = tmp

        @staticmethod
        def get_lidar(idx):
            return clouds[idx].copy()

    R.kitti_dataset.KittiDataset.create_groundtruth_database(Dataset(), info_path=info_path, used_classes=USED_CLASSES, split=SPLIT)
    with open(tmp / ("kitti_dbinfos_%s.pkl" % SPLIT), "rb") as f:
        db = pickle.load(f)

    out = {"n_frames": np.array(len(infos), np.int64), "used_classes": np.array(USED_CLASSES), "split": np.array(SPLIT)}
    for k, info in enumerate(infos):
        a, p = info["annos"], f"f{k}."
        out.update({p + "lidar_idx": np.array(info["point_cloud"]["lidar_idx"]), p + "points": clouds[info["point_cloud"]["lidar_idx"]],
                    p + "name": a["name"], p + "difficulty": a["difficulty"], p + "bbox": a["bbox"], p + "score": a["score"],
                    p + "gt_boxes_lidar": a["gt_boxes_lidar"]})
    out["db.classes"] = np.array(list(db))
    out["db.class_sizes"] = np.array([len(v) for v in db.values()], np.int64)
    for c, recs in enumerate(db.values()):                                       # a class's records, stacked key by key
        assert all(list(r) == GC.RECORD_KEYS for r in recs)
        types = [[type(r[k]).__name__ for k in GC.RECORD_KEYS] for r in recs]
        assert all(t == types[0] for t in types)
        out[f"db.{c}.types"] = np.array(types[0])
        for k in GC.RECORD_KEYS:
            out[f"db.{c}.{k}"] = np.array([r[k] for r in recs])
            assert out[f"db.{c}.{k}"].dtype == np.asarray(recs[0][k]).dtype or k in ("name", "path", "image_idx"), k
    paths = sorted(str(q.relative_to(tmp)) for q in (tmp / "gt_database").iterdir())
    blobs = [open(tmp / q, "rb").read() for q in paths]
    off = np.zeros((len(paths) + 1,), np.int64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    out.update({"files.paths": np.array(paths), "files.off": off, "files.bytes": np.frombuffer(b"".join(blobs), np.uint8)})

    # the coverage the scene is there for
    sizes = dict(zip(paths, np.diff(off)))
    n_obj = sum(i["annos"]["gt_boxes_lidar"].shape[0] for i in infos)
    assert len(paths) == n_obj == 12 and "Van" not in db and any("Van" in q for q in paths)
    assert sizes["gt_database/000023_%s_5.bin" % infos[2]["annos"]["name"][5]] == 0, "the empty object has points"
    assert sum(v == 0 for v in sizes.values()) == 1
    hit = gt_sampling.points_in_boxes_cpu(clouds["000022"][:, :3], infos[1]["annos"]["gt_boxes_lidar"])
    assert hit[:, 7].tolist() == [1, 1] and (hit.sum(axis=0) == 2).sum() >= 1, "no point in two boxes"
    assert not any("DontCare" in q for q in paths)
    path = os.path.join(MG.OUT, "g21_gt_database.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(paths), "files,", int(off[-1]), "bytes of points")


if __name__ == "__main__":
    main()
