"""KITTI object AP on the device (row f3 of SURVEY.md §8f): the result of kitti_eval.get_official_eval_result from a fixed number
of launches and two host reads per eval_class, whatever the number of frames.

kitti_eval.py (interpreted loops per frame x class x difficulty x overlap set x threshold) stays untouched as the yardstick.  Here
the annotations of all frames are laid end to end once (AnnoTables), the overlaps of every frame come from two launches
(hvpr_boxes_pairwise_ragged_f32, hvpr_kitti_overlaps_f64) and the greedy matching from hvpr_kitti_match_f64 (csrc/kitti_ap.hip):

    overlaps -> threshold pass -> ONE read (true-positive scores, n_valid) -> kitti_eval.get_thresholds per combo on the host
             -> counting pass  -> ONE read (tp / fp / fn and the orientation similarity per combo and threshold)

Precision, recall, AOS and the monotone envelope are then formed by the expressions of kitti_eval.eval_class from the same
integers, so precision and recall are equal to the host's; the similarity sums differ from the host's by the device's cos and
the order of a double sum only.
"""
import numpy as np

from . import kitti_eval
from .kitti_eval import CLASS_TO_NAME, _N_SAMPLE

MAX_DT_PER_FRAME, MAX_GT_PER_FRAME = 4096, 1024      # the matching kernel keeps one `assigned` bit per detection in 64 lanes x 64 bits
ROW = 16                                             # doubles per annotation row
_COLS = {"bbox": slice(0, 4), "alpha": 4, "location": slice(5, 8), "dimensions": slice(8, 11), "rotation_y": 11, "occluded": 12,
         "truncated": 13, "score": 14}
_NAME_TO_CLASS = {v.lower(): k for k, v in CLASS_TO_NAME.items()}


def _rows(annos, with_score):
    n = sum(len(a["name"]) for a in annos)
    rows = np.zeros((n, ROW), np.float64)
    for key, col in _COLS.items():
        if key == "score" and not with_score:
            continue
        width = {"bbox": 4, "location": 3, "dimensions": 3}.get(key)
        parts = [np.asarray(a[key]).astype(np.float64).reshape((-1, width) if width else (-1,)) for a in annos if len(a["name"])]
        if parts:
            rows[:, col] = np.concatenate(parts)
    names = [str(s) for a in annos for s in a["name"]]
    cls = np.array([_NAME_TO_CLASS.get(s.lower(), -1) for s in names], np.int32).reshape(-1)
    return rows, cls, names


def _as7(rows):
    """The float32 (x, z, 0, l, w, 1, -rotation_y) rows kitti_eval.hip_rotated_intersection hands to the geometry kernel."""
    t = np.zeros((len(rows), 7), np.float32)
    t[:, 0], t[:, 1], t[:, 3], t[:, 4], t[:, 5] = rows[:, 5], rows[:, 7], rows[:, 8], rows[:, 10], 1.0
    t[:, 6] = -rows[:, 11].astype(np.float32)
    return t


class AnnoTables:
    """All frames of (gt_annos, dt_annos) as flat arrays, built once on the host and uploaded once (on first use of `.dev`).

    Per box a row of 16 float64: bbox[4], alpha, location[3], dimensions[3], rotation_y, occluded, truncated, score (detections),
    pad; `gt_cls` / `dt_cls` the int32 class id of the LOWER-CASED name through CLASS_TO_NAME (0..5, else -1); `gt_dontcare` one
    byte per ground truth from the EXACT string "DontCare" (clean_data mixes the two comparisons in just this way); `gt_off`,
    `dt_off`, `pair_off` int64 [F + 1] with pair_off[f + 1] - pair_off[f] = nd_f * ng_f; `gt_box7` / `dt_box7` the float32 rows
    of the rotated-rectangle kernel.

    Arrays arriving as float32 are widened to float64 first.  The host evaluator forms its area and volume products in the
    incoming dtype, so equality with it is claimed for float64 annotations; for float32 annotations it is claimed against the
    host evaluator run on the widened copies.

    Raises ValueError for a frame with more than 4096 detections or 1024 ground truths, or totals past what the kernels index.
    """

    def __init__(self, gt_annos, dt_annos):
        if len(gt_annos) != len(dt_annos):
            raise ValueError("gt_annos and dt_annos must hold the same frames")
        self.n_frames = F = len(gt_annos)
        ng = np.array([len(a["name"]) for a in gt_annos], np.int64)
        nd = np.array([len(a["name"]) for a in dt_annos], np.int64)
        if F and (nd.max() > MAX_DT_PER_FRAME or ng.max() > MAX_GT_PER_FRAME):
            raise ValueError(f"at most {MAX_DT_PER_FRAME} detections and {MAX_GT_PER_FRAME} ground truths per frame "
                             f"(got {int(nd.max())} and {int(ng.max())})")
        self.gt_off, self.dt_off, self.pair_off = (np.concatenate([[0], np.cumsum(v)]).astype(np.int64) for v in (ng, nd, nd * ng))
        if self.gt_off[-1] >= 2 ** 31 or self.dt_off[-1] >= 2 ** 31 or self.pair_off[-1] > 2 ** 36:
            raise ValueError("too many boxes or pairs for one evaluation")
        self.gt_rows, self.gt_cls, gnames = _rows(gt_annos, False)
        self.dt_rows, self.dt_cls, _ = _rows(dt_annos, True)
        self.gt_dontcare = np.array([s == "DontCare" for s in gnames], np.uint8).reshape(-1)
        self.gt_box7, self.dt_box7 = _as7(self.gt_rows), _as7(self.dt_rows)
        self.n_gt, self.n_dt, self.n_pairs = int(self.gt_off[-1]), int(self.dt_off[-1]), int(self.pair_off[-1])
        self._dev = None

    @classmethod
    def from_device(cls, gt_annos, dt_rows, dt_cls, dt_box7, dt_off, n_dt, n_pairs, pair_off=None):
        """Tables whose detection side is ALREADY on the device (eval_loop.DeviceEvalEpilogue fills it batch by batch): dt_rows
        [>= n_dt, 16] f64, dt_cls i32, dt_box7 [.., 7] f32, dt_off [F + 1] int64, all cuda.  The ground truths are laid out from the
        host dicts as in the constructor and uploaded with them.  n_dt and n_pairs are the two HOST totals the launches are sized
        with (the caller reads them; nothing is read here); pair_off, when the caller formed it for that read, is taken as it is.
        The detection side has no host copy: `dt_rows`, `dt_cls`, `dt_box7` and the host `dt_off` / `pair_off` stay None."""
        import torch
        self = cls.__new__(cls)
        self.n_frames = F = len(gt_annos)
        if dt_off.numel() != F + 1:
            raise ValueError("gt_annos and dt_off must hold the same frames")
        ng = np.array([len(a["name"]) for a in gt_annos], np.int64)
        if F and ng.max() > MAX_GT_PER_FRAME:
            raise ValueError(f"at most {MAX_GT_PER_FRAME} ground truths per frame (got {int(ng.max())})")
        self.gt_off = np.concatenate([[0], np.cumsum(ng)]).astype(np.int64)
        self.n_gt, self.n_dt, self.n_pairs = int(self.gt_off[-1]), int(n_dt), int(n_pairs)
        if self.n_gt >= 2 ** 31 or self.n_dt >= 2 ** 31 or self.n_pairs > 2 ** 36:
            raise ValueError("too many boxes or pairs for one evaluation")
        self.gt_rows, self.gt_cls, gnames = _rows(gt_annos, False)
        self.gt_dontcare = np.array([s == "DontCare" for s in gnames], np.uint8).reshape(-1)
        self.gt_box7 = _as7(self.gt_rows)
        self.dt_rows = self.dt_cls = self.dt_box7 = self.dt_off = self.pair_off = None
        dev = dt_off.device
        up = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(dev) for k in ("gt_rows", "gt_cls", "gt_dontcare", "gt_box7", "gt_off")}
        if pair_off is None:
            pair_off = device_pair_off(dt_off, up["gt_off"])
        self._dev = dict(up, dt_rows=dt_rows, dt_cls=dt_cls, dt_box7=dt_box7, dt_off=dt_off, pair_off=pair_off)
        return self

    _FIELDS = ("gt_rows", "gt_cls", "gt_dontcare", "gt_box7", "dt_rows", "dt_cls", "dt_box7", "gt_off", "dt_off", "pair_off")

    @property
    def dev(self):
        """The arrays as CUDA tensors (uploaded on first use)."""
        if self._dev is None:
            import torch
            self._dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).cuda() for k in self._FIELDS}
        return self._dev


def device_pair_off(dt_off, gt_off):
    """pair_off [F + 1] int64 on the device from the two device offset arrays: pair_off[f + 1] - pair_off[f] = nd_f * ng_f."""
    import torch
    pairs = (dt_off[1:] - dt_off[:-1]) * (gt_off[1:] - gt_off[:-1])
    return torch.cat([torch.zeros((1,), dtype=torch.int64, device=dt_off.device), torch.cumsum(pairs, 0)])


def _read(t):
    """The module's ONE way from device to host (a synchronising copy): eval_class makes two of these."""
    return t.cpu().numpy()


def rotated_intersections(tables):
    """(n_pairs,) float32 BEV intersection areas of every frame's detections x ground truths, one launch."""
    from . import kernels
    d = tables.dev
    return kernels.boxes_pairwise_ragged(d["dt_box7"], d["gt_box7"], d["dt_off"], d["gt_off"], d["pair_off"], tables.n_pairs)


def overlaps(tables, metric):
    """(n_pairs,) float64 on the device: kitti_eval.frame_overlap of every frame, frame f at pair_off[f] as [nd_f, ng_f]."""
    from . import kernels
    d = tables.dev
    inter = rotated_intersections(tables) if metric != 0 else None
    return kernels.kitti_overlaps(d["gt_rows"], d["dt_rows"], inter, d["gt_off"], d["dt_off"], d["pair_off"], tables.n_pairs, metric)


def _match(tables, ov, metric, classes, mo, thresholds=None, thresh_count=None, compute_aos=False, out=None):
    from . import kernels
    d = tables.dev
    return kernels.kitti_match(d["gt_rows"], d["gt_cls"], d["gt_dontcare"], d["dt_rows"], d["dt_cls"], d["gt_off"], d["dt_off"],
                               d["pair_off"], ov, metric, classes, mo, thresholds, thresh_count, compute_aos, out)


def match_statistics(tables, classes, metric, min_overlaps, compute_aos=False):
    """The integers behind eval_class.  -> dict(tp_score [combos, NG] (NaN: no true positive), n_valid [C, 3], thresholds
    [combos, 41], thresh_count [combos], counts [combos, 41, 3] (tp, fp, fn), sim [combos, 41]); combo = (m * 3 + l) * K + k."""
    import torch
    mo = np.ascontiguousarray(np.asarray(min_overlaps, np.float64)[:, metric, :])          # [K, C]
    K, C = mo.shape
    combos, NG, T = C * 3 * K, tables.n_gt, _N_SAMPLE
    dev = tables.dev["pair_off"].device
    ov = overlaps(tables, metric)
    # threshold pass: scores and n_valid share one buffer, so that one copy brings both
    buf = torch.empty((combos * NG * 8 + C * 3 * 4,), dtype=torch.uint8, device=dev)
    _match(tables, ov, metric, classes, mo, out=(buf[:combos * NG * 8].view(torch.float64).view(combos, NG),
                                                 buf[combos * NG * 8:].view(torch.int32).view(C, 3)))
    host = _read(buf)
    tp_score = host[:combos * NG * 8].view(np.float64).reshape(combos, NG)
    n_valid = host[combos * NG * 8:].view(np.int32).reshape(C, 3)
    thresholds, thresh_count = np.zeros((combos, T)), np.zeros(combos, np.int32)
    for combo in range(combos):
        s = tp_score[combo]
        th = kitti_eval.get_thresholds(s[~np.isnan(s)], int(n_valid[combo // K // 3, combo // K % 3]))
        thresholds[combo, :len(th)], thresh_count[combo] = th, len(th)
    # counting pass: similarity sums and counts share one buffer likewise
    buf = torch.empty((combos * T * (8 + 3 * 4),), dtype=torch.uint8, device=dev)
    _match(tables, ov, metric, classes, mo, torch.from_numpy(thresholds).to(dev), torch.from_numpy(thresh_count).to(dev), compute_aos,
           out=(buf[combos * T * 8:].view(torch.int32).view(combos, T, 3), buf[:combos * T * 8].view(torch.float64).view(combos, T)))
    host = _read(buf)
    return {"tp_score": tp_score, "n_valid": n_valid, "thresholds": thresholds, "thresh_count": thresh_count,
            "counts": host[combos * T * 8:].view(np.int32).reshape(combos, T, 3),
            "sim": host[:combos * T * 8].view(np.float64).reshape(combos, T)}


def eval_class(tables, classes, metric, min_overlaps, compute_aos=False):
    """kitti_eval.eval_class on the device -> dict(precision, recall, orientation), each [class, difficulty, overlap set, 41]."""
    st = match_statistics(tables, classes, metric, min_overlaps, compute_aos)
    K = len(min_overlaps)
    shape = (len(classes), 3, K, _N_SAMPLE)
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for m in range(len(classes)):
        for l in range(3):
            for k in range(K):
                combo = (m * 3 + l) * K + k
                n = int(st["thresh_count"][combo])
                pr = np.zeros((n, 4))
                pr[:, :3], pr[:, 3] = st["counts"][combo, :n], st["sim"][combo, :n]
                with np.errstate(divide="ignore", invalid="ignore"):
                    recall[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
                    precision[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
                    if compute_aos:
                        aos[m, l, k, :n] = pr[:, 3] / (pr[:, 0] + pr[:, 1])
                for arr in (precision, recall, aos):       # monotone envelope over the sampled thresholds
                    for i in range(n):
                        arr[m, l, k, i] = np.max(arr[m, l, k, i:])
    return {"precision": precision, "recall": recall, "orientation": aos}


def get_official_eval_result(gt_annos, dt_annos, current_classes):
    """kitti_eval.get_official_eval_result with the per-frame work on the device -> (text, ret_dict), same text and keys."""
    tables = AnnoTables(gt_annos, dt_annos)
    return kitti_eval.get_official_eval_result(
        gt_annos, dt_annos, current_classes,
        eval_class_fn=lambda gts, dts, classes, metric, mo, compute_aos: eval_class(tables, classes, metric, mo, compute_aos))
