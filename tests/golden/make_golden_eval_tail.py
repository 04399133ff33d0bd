"""Generate tests/golden/g20_eval_tail.npz: the reference's evaluation epilogue on a canned scene — KittiDataset.
generate_prediction_dicts (kitti_dataset.py:246-320), Detector3DTemplate.generate_recall_record (detector3d_template.py:276-318)
and the loop of eval_one_epoch (tools/eval_utils/eval_utils.py:22-127), each imported and run as it is.

Runs only where the reference is (see make_golden.py, whose loader this script imports and does not edit).  Stood in for, in
memory: the absent native boxes_iou3d_gpu by the CPU oracle (as G15 does), the absent rotate_iou.py by the oracle's rotated
intersection and numba.jit by the identity (as G12 does), skimage (imported by kitti_dataset.py, unused here), DatasetTemplate
(the base class, which neither method touches), load_data_to_gpu.  Those stay UNPINNED; what G20 pins is the reference's Python.

Scene: 6 frames as 3 batches of 2 with 0, 1, 5, 12, 3, 7 detections, three classes, two calibrations (one with R0 = identity),
two image shapes.  generate_prediction_dicts is fed COPIES of the boxes: it lowers z of the array it is given in place
(box_utils.py:159-162), so the `boxes_lidar` it returns carries the bottom-centre z, and that is what is stored.

Margins, asserted below in float64: every box centre has x >= 5 m, every projected corner a depth >= 2 m, every image-box edge lies
inside the image by >= 1 px or outside it by >= 1 px (the clip is then active), with at least one edge of each kind on each of
the four sides; no best IoU of the recall record lies within 1e-3 of a threshold.
"""
import os
import re
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
import eval_tail_cases as EC  # noqa: E402

CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]
THRESHOLDS = [0.3, 0.5, 0.7]
SIZES = {1: [3.9, 1.6, 1.56], 2: [0.8, 0.6, 1.73], 3: [1.76, 0.6, 1.73]}
N_PRED = [0, 1, 5, 12, 3, 7]
CALIBS = [
    {"P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
     "R0": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
                     [0.007402527, 0.004351614, 0.9999631]], np.float32),
     "Tr_velo2cam": np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                              [0.9998621, 0.007523790, 0.01480755, -0.2717806]], np.float32)},
    {"P2": np.array([[707.0493, 0, 604.0814, 45.75831], [0, 707.0493, 180.5066, -0.3454157], [0, 0, 1, 0.004981016]], np.float32),
     "R0": np.eye(3, dtype=np.float32),
     "Tr_velo2cam": np.array([[0.0, -1.0, 0.0, 0.003], [0.0, 0.0, -1.0, -0.06], [1.0, 0.0, 0.0, -0.29]], np.float32)},
]
CALIB_OF = [0, 1, 0, 1, 1, 0]
IMAGE_SHAPE = [[375, 1242], [370, 1224], [375, 1242], [370, 1224], [370, 1224], [375, 1242]]

# label, x, y, z (centre), heading, size scale — the boxes that cross an image side; the rest are drawn far enough to lie inside
CROSSING = {
    2: [(1, 6.0, 5.6, -0.9, 0.3, 1.0), (2, 5.2, -4.4, -0.7, 1.1, 1.0)],                      # left | right
    3: [(1, 5.4, 0.4, 0.7, 1.5, 1.3), (1, 5.3, -0.6, -1.05, 1.62, 1.0), (3, 5.6, 5.1, -0.6, -0.4, 1.0),
        (2, 5.1, -4.7, -0.8, 2.9, 1.0)],                                                     # top | bottom | left | right
    5: [(1, 5.5, 1.0, 0.9, 0.2, 1.2), (1, 5.2, -4.0, -1.0, 1.4, 1.0)],                        # top (and left) | bottom, right
}


def scene(seed):
    gen = np.random.RandomState(seed)
    frames = []
    for f, n in enumerate(N_PRED):
        rows = list(CROSSING.get(f, []))[:n]
        while len(rows) < n:
            x = gen.uniform(12.0, 60.0)
            rows.append((int(gen.randint(1, 4)), x, gen.uniform(-0.55, 0.55) * x, gen.uniform(-1.2, -0.4), gen.uniform(-np.pi, np.pi),
                         gen.uniform(0.85, 1.15)))
        boxes = np.array([[x, y, z, *(np.array(SIZES[l]) * s), h] for l, x, y, z, h, s in rows], np.float32).reshape(-1, 7)
        labels = np.array([r[0] for r in rows], np.int64)
        scores = np.round(gen.permutation(np.linspace(0.12, 0.97, 40))[:n], 4).astype(np.float32)
        order = gen.permutation(n)
        frames.append((boxes[order], scores[order], labels[order]))
    return frames, gen


def ground_truth(frames, gen):
    """Per batch a padded (2, G, 8) table: copies of detections moved along x, misses, and the zero-row cases."""
    G = 6

    def rows_of(f, picks, shifts):
        t = np.zeros((G, 8), np.float32)
        b, _, l = frames[f]
        for r, (i, dx) in enumerate(zip(picks, shifts)):
            t[r, :7], t[r, 7] = b[i], l[i]
            t[r, 0] += dx
        return t
    g0 = np.zeros((G, 8), np.float32)                           # frame 0: no detection, two ground truths (missed)
    g0[0] = [20.0, 3.0, -0.9, 3.9, 1.6, 1.56, 0.4, 1]
    g0[1] = [30.0, -6.0, -0.7, 0.8, 0.6, 1.73, 1.0, 2]
    g1 = rows_of(1, [0], [0.25])
    g2 = rows_of(2, [0, 1, 2, 3], [0.0, 0.1, 0.45, 9.0])
    g2[5] = g2[3]; g2[3] = 0                                    # a zero row in the middle stays a ground truth
    g3 = rows_of(3, [0, 2, 4, 6, 8, 10], [0.05, 0.2, 0.12, 0.6, 0.3, 0.02])
    g4 = np.zeros((G, 8), np.float32)                           # all rows zero: the reference counts ONE box
    g5 = rows_of(5, [1, 3, 5], [0.15, 0.33, 0.08])
    return [np.stack([g0, g1]), np.stack([g2, g3]), np.stack([g4, g5])]


def check_margins(frames):
    sides = {(k, kind): 0 for k in range(4) for kind in ("in", "out")}
    for f, (boxes, _, _) in enumerate(frames):
        if not len(boxes):
            continue
        assert (boxes[:, 0] >= 5.0).all(), f
        h, w = IMAGE_SHAPE[f]
        r = EC.annos_f64(boxes, CALIBS[CALIB_OF[f]], (h, w))
        assert (r["depth"] >= 2.0).all(), (f, r["depth"].min())
        for k, (lo, hi) in enumerate(((0, w - 1), (0, h - 1), (0, w - 1), (0, h - 1))):
            e = r["edges"][:, k]
            bound = lo if k < 2 else hi                         # the side this edge can cross
            other = hi if k < 2 else lo
            inside = (e >= lo + 1) & (e <= hi - 1)
            outside = (e <= bound - 1) if k < 2 else (e >= bound + 1)
            assert (inside | outside).all(), (f, k, e)
            assert not (((e <= other + 1) if k >= 2 else (e >= other - 1)) & ~inside).any(), (f, k, e)   # never across the far side
            sides[k, "in"] += int(inside.sum())
            sides[k, "out"] += int(outside.sum())
    assert all(v > 0 for v in sides.values()), sides
    return sides


def load_eval_side(R):
    """kitti_dataset.py, eval.py (as in make_golden.g12_kitti_eval) and eval_utils.py with their absent imports stood in."""
    O = MG._import_oracle()
    R = MG.load_post_processing(R)

    def jit(*a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else (lambda f: f)
    nb = MG._stub("numba"); nb.jit = jit; nb.prange = range

    def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
        def as7(b):
            t = np.zeros((len(b), 7), np.float32)
            t[:, 0:2], t[:, 3:5], t[:, 5], t[:, 6] = b[:, 0:2], b[:, 2:4], 1.0, -b[:, 4]
            return t
        inter = O.boxes_overlap_bev(as7(boxes), as7(query_boxes)).astype(np.float64) if len(boxes) and len(query_boxes) else \
            np.zeros((len(boxes), len(query_boxes)))
        a1, a2 = (boxes[:, 2] * boxes[:, 3])[:, None], (query_boxes[:, 2] * query_boxes[:, 3])[None, :]
        ua = {-1: a1 + a2 - inter, 0: a1 + 0 * a2, 1: a2 + 0 * a1}.get(criterion)
        return inter.astype(np.float32) if ua is None else np.where(inter > 0, inter / ua, 0.0).astype(np.float32)
    MG._stub("pcdet.datasets", os.path.join(MG.REF, "pcdet/datasets"))
    kitti = MG._stub("pcdet.datasets.kitti", os.path.join(MG.REF, "pcdet/datasets/kitti"))
    pkg = MG._stub("pcdet.datasets.kitti.kitti_object_eval_python", os.path.join(MG.REF, "pcdet/datasets/kitti/kitti_object_eval_python"))
    MG._stub("pcdet.datasets.kitti.kitti_object_eval_python.rotate_iou").rotate_iou_gpu_eval = rotate_iou_gpu_eval
    pkg.eval = MG._load("pcdet.datasets.kitti.kitti_object_eval_python.eval", "pcdet/datasets/kitti/kitti_object_eval_python/eval.py")
    kitti.kitti_object_eval_python = pkg
    sk = MG._stub("skimage"); sk.io = MG._stub("skimage.io")
    MG._stub("pcdet.datasets.dataset").DatasetTemplate = type("DatasetTemplate", (), {})
    utils = sys.modules["pcdet.utils"]
    utils.calibration_kitti = R.calibration = MG._load("pcdet.utils.calibration_kitti", "pcdet/utils/calibration_kitti.py")
    utils.object3d_kitti = MG._load("pcdet.utils.object3d_kitti", "pcdet/utils/object3d_kitti.py")
    R.kitti_dataset = MG._load("pcdet.datasets.kitti.kitti_dataset", "pcdet/datasets/kitti/kitti_dataset.py")
    sys.modules["pcdet.models"].load_data_to_gpu = lambda batch_dict: R.protocol.append("load_data_to_gpu")
    sys.modules["pcdet"].models = sys.modules["pcdet.models"]
    sys.modules["pcdet"].utils = utils
    MG._stub("eval_utils", os.path.join(MG.REF, "tools/eval_utils"))
    R.eval_utils = MG._load("eval_utils.eval_utils", "tools/eval_utils/eval_utils.py")
    R.protocol = []
    return R


def gt_annos_of(R, gts):
    """The split's ground-truth annotation dicts (camera frame), formed from the non-zero lidar rows by the reference's own
    box_utils, as kitti_dataset.py forms the detections'."""
    annos = []
    for f in range(len(N_PRED)):
        g = gts[f // 2][f % 2]
        g = g[np.abs(g).sum(1) > 0]
        calib = R.calibration.Calibration(dict(CALIBS[CALIB_OF[f]]))
        n = len(g)
        a = {"name": np.array([CLASS_NAMES[int(c) - 1] for c in g[:, 7]], dtype="<U16"), "truncated": np.zeros(n), "occluded": np.zeros(n, np.int64),
             "alpha": np.zeros(n), "bbox": np.zeros((n, 4)), "dimensions": np.zeros((n, 3)), "location": np.zeros((n, 3)), "rotation_y": np.zeros(n)}
        if n:
            b = g[:, :7].copy()
            cam = R.box_utils.boxes3d_lidar_to_kitti_camera(b.copy(), calib)
            a.update(alpha=(-np.arctan2(-b[:, 1], b[:, 0]) + cam[:, 6]).astype(np.float64),
                     bbox=R.box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=IMAGE_SHAPE[f]).astype(np.float64),
                     dimensions=cam[:, 3:6].astype(np.float64), location=cam[:, 0:3].astype(np.float64), rotation_y=cam[:, 6].astype(np.float64))
        annos.append(a)
    return annos


def main():
    R = load_eval_side(MG.load_reference())
    frames, gen = scene(2020)
    sides = check_margins(frames)
    gts = ground_truth(frames, gen)
    F, B = len(N_PRED), 2
    out = {"class_names": np.array(CLASS_NAMES), "thresholds": np.array(THRESHOLDS, np.float64), "n_frames": np.int64(F), "batch": np.int64(B),
           "n_calibs": np.int64(len(CALIBS)), "calib_of": np.array(CALIB_OF, np.int64), "image_shape": np.array(IMAGE_SHAPE, np.int64),
           "frame_id": np.array(["%06d" % (7 * f + 3) for f in range(F)])}
    for c, cal in enumerate(CALIBS):
        for k, v in cal.items():
            out[f"calib{c}.{k}"] = v
    for f, (b, s, l) in enumerate(frames):
        out[f"f{f}.pred_boxes"], out[f"f{f}.pred_scores"], out[f"f{f}.pred_labels"] = b, s, l
    for k, g in enumerate(gts):
        out[f"b{k}.gt_boxes"] = g

    KD = R.kitti_dataset.KittiDataset
    iou3d = R.det_template.iou3d_nms_utils.boxes_iou3d_gpu
    recall_fn = R.det_template.Detector3DTemplate.generate_recall_record

    def batch_dict(k):
        fs = range(k * B, (k + 1) * B)
        return {"batch_size": B, "frame_id": [str(out["frame_id"][f]) for f in fs], "image_shape": np.array([IMAGE_SHAPE[f] for f in fs]),
                "calib": [R.calibration.Calibration(dict(CALIBS[CALIB_OF[f]])) for f in fs], "gt_boxes": torch.from_numpy(gts[k].copy())}

    def pred_dicts(k):
        return [{"pred_boxes": torch.from_numpy(frames[f][0].copy()), "pred_scores": torch.from_numpy(frames[f][1].copy()),
                 "pred_labels": torch.from_numpy(frames[f][2].copy())} for f in range(k * B, (k + 1) * B)]

    # --- prediction dicts and recall counters, the two functions called directly
    total = {}
    for k in range(F // B):
        bd, pd = batch_dict(k), pred_dicts(k)
        annos = KD.generate_prediction_dicts(bd, pd, CLASS_NAMES)
        rec = {}
        for i, p in enumerate(pd):
            f = k * B + i
            rec = recall_fn(torch.from_numpy(frames[f][0].copy()), rec, i, bd, THRESHOLDS)
            a = annos[i]
            assert a["frame_id"] == str(out["frame_id"][f]) and len(a["name"]) == N_PRED[f]
            for key in EC.FIELDS + ("name", "truncated", "occluded"):
                v = np.asarray(a[key])
                out[f"f{f}.anno.{key}"] = v.astype("<U16") if v.dtype.kind in "US" else v
            if N_PRED[f]:
                assert a["bbox"].dtype == np.float32 and a["alpha"].dtype == np.float32
                assert np.array_equal(a["boxes_lidar"][:, 2], frames[f][0][:, 2] - frames[f][0][:, 5] / 2)      # z lowered in place
                g = gts[k][i]
                last = len(g) - 1
                while last > 0 and g[last].sum() == 0:
                    last -= 1
                best = iou3d(torch.from_numpy(frames[f][0][:, :7].copy()), torch.from_numpy(g[:last + 1, :7].copy())).max(0)[0].numpy()
                assert all(np.abs(best - t).min() > 1e-3 for t in THRESHOLDS), (f, best)
                out[f"f{f}.best_iou"] = best
        keys = sorted(rec)
        out[f"b{k}.recall_keys"], out[f"b{k}.recall_values"] = np.array(keys), np.array([rec[x] for x in keys], np.int64)
        for x in keys:
            total[x] = total.get(x, 0) + rec[x]
    out["recall_keys"], out["recall_values"] = np.array(sorted(total)), np.array([total[x] for x in sorted(total)], np.int64)
    assert total["gt"] == 2 + 1 + 6 + 6 + 1 + 3 and 0 < total["rcnn_0.7"] < total["rcnn_0.5"] < total["rcnn_0.3"] < total["gt"], total

    # --- the loop protocol: eval_one_epoch over stand-ins
    gt_annos = gt_annos_of(R, gts)
    for f, a in enumerate(gt_annos):
        for key, v in a.items():
            out[f"f{f}.gt.{key}"] = v
    log = R.protocol
    del log[:]

    class Dataset:
        class_names = CLASS_NAMES
        kitti_infos = [{"annos": a} for a in gt_annos]

        def __len__(self):
            return F

        @staticmethod
        def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
            log.append("dataset.generate_prediction_dicts")
            return KD.generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=output_path)

        def evaluation(self, det_annos, class_names, **kwargs):
            log.append("dataset.evaluation(%s)" % ",".join(sorted(kwargs)))
            return KD.evaluation(self, det_annos, class_names, **kwargs)

    class Loader:
        dataset = Dataset()

        def __len__(self):
            return F // B

        def __iter__(self):
            return (batch_dict(k) for k in range(F // B))

    class Model:
        def __init__(self):
            self.k = 0

        def eval(self):
            log.append("model.eval")

        def __call__(self, bd):
            log.append("model(batch)")
            pd, rec = pred_dicts(self.k), {}
            for i in range(B):
                rec = recall_fn(pd[i]["pred_boxes"], rec, i, bd, THRESHOLDS)
            self.k += 1
            return pd, rec, None

    class Logger:
        def info(self, s):
            log.append("logger.info:" + re.sub(r"[0-9.]+ second", "<t> second", str(s).split("\n")[0][:60]))

    cfg = MG.EasyDict(LOCAL_RANK=0, MODEL=dict(POST_PROCESSING=dict(RECALL_THRESH_LIST=THRESHOLDS, EVAL_METRIC="kitti")))
    with tempfile.TemporaryDirectory(prefix="g20_eval_") as tmp:
        ret = R.eval_utils.eval_one_epoch(cfg, Model(), Loader(), 7, Logger(), dist_test=False, save_to_file=False, result_dir=Path(tmp))
        assert (Path(tmp) / "result.pkl").exists()
    keys = sorted(ret)
    out["loop.calls"] = np.array([s.replace(tmp, "<result_dir>") for s in log])
    out["loop.keys"], out["loop.values"] = np.array(keys), np.array([float(ret[k]) for k in keys], np.float64)
    assert ret["recall/rcnn_0.3"] == total["rcnn_0.3"] / total["gt"] and max(ret[k] for k in keys if "3d" in k) > 0, ret
    path = os.path.join(MG.OUT, "g20_eval_tail.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; edges per side (in / out):", sides)
    print({k: round(float(ret[k]), 4) for k in keys if "moderate_R40" in k or "recall" in k}, dict(total))


if __name__ == "__main__":
    main()
