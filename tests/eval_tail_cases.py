"""Shared by the G20 generator (tests/golden/make_golden_eval_tail.py) and the eval-tail tests: the annotation formulas of
box_utils.py:152-235 / kitti_dataset.py:281-293 evaluated in float64, and the loader of the fixture."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_eval_tail.npz")
FIELDS = ("alpha", "bbox", "dimensions", "location", "rotation_y", "score", "boxes_lidar")
SX = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64) / 2
SZ = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64) / 2


def annos_f64(boxes, calib, image_shape):
    """boxes (n, 7) lidar, centre z -> dict of float64 arrays: the annotation fields, plus `edges` (the image box before the
    clip) and `depth` (n, 8), the rect depth of every corner."""
    b = np.asarray(boxes, np.float64).reshape(-1, 7)
    V2C, R0, P2 = (np.asarray(calib[k], np.float64) for k in ("Tr_velo2cam", "R0", "P2"))
    xyz = b[:, 0:3].copy()
    xyz[:, 2] -= b[:, 5] / 2
    loc = np.hstack([xyz, np.ones((len(b), 1))]) @ (V2C.T @ R0.T)
    l, w, h = b[:, 3], b[:, 4], b[:, 5]
    ry = -b[:, 6] - np.pi / 2
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    xc, zc = l[:, None] * SX, w[:, None] * SZ
    yc = np.zeros((len(b), 8))
    yc[:, 4:] = -h[:, None]
    cx, cy, cz = loc[:, 0:1] + (xc * c + zc * s), loc[:, 1:2] + yc, loc[:, 2:3] + (-xc * s + zc * c)
    u = (cx * P2[0, 0] + cy * P2[0, 1] + cz * P2[0, 2] + P2[0, 3]) / cz
    v = (cx * P2[1, 0] + cy * P2[1, 1] + cz * P2[1, 2] + P2[1, 3]) / cz
    edges = np.stack([u.min(1), v.min(1), u.max(1), v.max(1)], axis=1) if len(b) else np.zeros((0, 4))
    bbox = edges.copy()
    bbox[:, [0, 2]] = np.clip(bbox[:, [0, 2]], 0, image_shape[1] - 1)
    bbox[:, [1, 3]] = np.clip(bbox[:, [1, 3]], 0, image_shape[0] - 1)
    lidar = b.copy()
    lidar[:, 2] = xyz[:, 2]
    return {"alpha": -np.arctan2(-b[:, 1], b[:, 0]) + ry, "bbox": bbox, "dimensions": np.stack([l, h, w], axis=1), "location": loc,
            "rotation_y": ry, "boxes_lidar": lidar, "edges": edges, "depth": cz}


class G20:
    """The fixture, read once."""

    def __init__(self):
        z = np.load(GOLDEN, allow_pickle=False)
        self.z = z
        self.class_names = [str(s) for s in z["class_names"]]
        self.thresholds = [float(t) for t in z["thresholds"]]
        self.n_frames, self.batch = int(z["n_frames"]), int(z["batch"])
        self.calibs = [{k: z[f"calib{c}.{k}"] for k in ("P2", "R0", "Tr_velo2cam")} for c in range(int(z["n_calibs"]))]
        self.calib_of, self.image_shape = z["calib_of"], z["image_shape"]
        self.frame_id = [str(s) for s in z["frame_id"]]

    def pred(self, f):
        return self.z[f"f{f}.pred_boxes"], self.z[f"f{f}.pred_scores"], self.z[f"f{f}.pred_labels"]

    def anno(self, f):
        return {k: self.z[f"f{f}.anno.{k}"] for k in FIELDS + ("name", "truncated", "occluded")}

    def gt_anno(self, f):
        return {k: self.z[f"f{f}.gt.{k}"] for k in ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y")}

    def gt_boxes(self, batch):
        return self.z[f"b{batch}.gt_boxes"]

    def batch_dict(self, batch):
        fs = range(batch * self.batch, (batch + 1) * self.batch)
        return {"batch_size": self.batch, "frame_id": [self.frame_id[f] for f in fs], "calib": [self.calibs[self.calib_of[f]] for f in fs],
                "image_shape": np.stack([self.image_shape[f] for f in fs]), "gt_boxes": self.gt_boxes(batch)}

    def recall(self, batch=None):
        tag = "recall" if batch is None else f"b{batch}.recall"
        return dict(zip((str(k) for k in self.z[tag + "_keys"]), (int(v) for v in self.z[tag + "_values"])))
