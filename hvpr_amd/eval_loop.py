"""The evaluation epilogue on the device (row f5): from the `sync=False` records of post_processing to KITTI annotation rows and
recall counters with NO host read per batch, and a whole split from points to the AP table with a constant number of reads.

The host path — post_processing(sync=True), Detector3DTemplate.generate_recall_record, kitti_eval.generate_prediction_dicts, then
kitti_eval_device.AnnoTables — stays as the yardstick and is not touched.  Here a batch costs one pinned upload of its calibration
table and two library calls (csrc/eval_tail.hip): hvpr_recall_record_f32 and hvpr_prediction_annos_f32, the latter writing straight
into the split-wide tables kitti_eval_device reads.  What comes back, and when:

    recall_dict()   ONE read: the running counters
    tables(gt)      ONE read: the two totals the evaluator's launches are sized with (detections, detection x ground-truth pairs)
    det_annos()     ONE read: the rows, for result.pkl and the txt files

Every device-to-host copy of this module goes through _read.
"""
import pickle

import numpy as np
import torch

from . import kernels, kitti_eval, kitti_eval_device as KD
from .calibration import CALIB_WORDS, pack_calib

N_READS = 0                                            # calls of _read so far (tests and tools/bench_eval_tail.py watch it)


def _read(t):
    """The module's ONE way from device to host (a synchronising copy)."""
    global N_READS
    N_READS += 1
    return t.cpu().numpy()


def class_of_label(class_names):
    """Evaluator class id (kitti_eval.CLASS_TO_NAME, compared in lower case as AnnoTables does) of label 1, 2, ...; -1 for a name
    outside the evaluator's six."""
    return [KD._NAME_TO_CLASS.get(str(n).lower(), -1) for n in class_names]


def _batched(recs, key, tail):
    """The per-frame tensors of a batch as one contiguous (B, ...) tensor (a small device copy, no read)."""
    return torch.stack([r[key].reshape(tail) for r in recs])


class DeviceEvalEpilogue:
    """Owns the split-wide detection tables (the layout of kitti_eval_device.AnnoTables) and the running recall counters.

    class_names: the detector's, label l names class_names[l - 1]; recall_thresh_list: POST_PROCESSING.RECALL_THRESH_LIST (at most
    8); max_frames: frames of the split; post_max: the rows a frame can have (<= 4096, the evaluator's limit): NMS_POST_MAXSIZE,
    times the number of classes on the MULTI_CLASSES_NMS branch (`post_max_of`).
    The tables hold max_frames * post_max rows unless `capacity` says otherwise; a split that outgrows them raises at the next
    read (nothing is written past them)."""

    def __init__(self, class_names, recall_thresh_list, max_frames, post_max, capacity=None, device="cuda"):
        if len(recall_thresh_list) > 8:
            raise ValueError("at most 8 recall thresholds")
        if not 0 < int(post_max) <= KD.MAX_DT_PER_FRAME:
            raise ValueError(f"post_max must be in 1..{KD.MAX_DT_PER_FRAME}")
        self.class_names, self.thresholds = list(class_names), list(recall_thresh_list)
        self.class_of_label = class_of_label(self.class_names)
        self.max_frames, self.post_max = int(max_frames), int(post_max)
        self.capacity = cap = int(capacity) if capacity is not None else self.max_frames * self.post_max
        dev = self.device = torch.device(device)
        self.dt_rows = torch.empty((cap, KD.ROW), dtype=torch.float64, device=dev)
        self.dt_cls = torch.empty((cap,), dtype=torch.int32, device=dev)
        self.dt_label = torch.empty((cap,), dtype=torch.int32, device=dev)
        self.dt_box7 = torch.empty((cap, 7), dtype=torch.float32, device=dev)
        self.boxes_lidar = torch.empty((cap, 7), dtype=torch.float32, device=dev)
        self.dt_off = torch.zeros((self.max_frames + 1,), dtype=torch.int64, device=dev)
        self.row_base = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.recall = torch.zeros((1 + len(self.thresholds),), dtype=torch.int64, device=dev)
        self.n_frames, self.rows_bound, self.frame_ids = 0, 0, []
        self._n_dt = None                                  # the host total, once tables() has read it

    # ---------------------------------------------------------------------------------------------------------- per batch
    def add_batch(self, batch_dict, pred_dicts):
        """The `sync=False` records of one batch -> rows and counters on the device.  No synchronising call."""
        B = len(pred_dicts)
        if B == 0:
            return
        if any("pred_count" not in r for r in pred_dicts):
            raise ValueError("add_batch takes the sync=False records of post_processing (class-agnostic or MULTI_CLASSES_NMS branch): "
                             "padded tensors with a device pred_count; sync=True records belong to the host path")
        if self.n_frames + B > self.max_frames:
            raise ValueError(f"more than max_frames = {self.max_frames} frames")
        P = int(pred_dicts[0]["pred_boxes"].shape[0])
        if P > self.post_max:
            raise ValueError(f"records padded to {P} rows, post_max is {self.post_max}")
        boxes = _batched(pred_dicts, "pred_boxes", (P, 7))
        scores = _batched(pred_dicts, "pred_scores", (P,))
        labels = _batched(pred_dicts, "pred_labels", (P,))
        counts = _batched(pred_dicts, "pred_count", (1,)).reshape(B)
        host = torch.empty((B, CALIB_WORDS), dtype=torch.float32, pin_memory=True)
        host.numpy()[:] = pack_calib(batch_dict["calib"], batch_dict["image_shape"])
        calib = host.to(self.device, non_blocking=True)
        if "gt_boxes" in batch_dict:
            gt = batch_dict["gt_boxes"]
            c = kernels.recall_record(boxes, counts, gt if gt.is_contiguous() else gt.contiguous(), self.thresholds)
            self.recall += c.sum(dim=0)
        kernels.prediction_annos(boxes, scores, labels, counts, calib, self.class_of_label, self.row_base, self.n_frames, self.dt_rows,
                                 self.dt_cls, self.dt_label, self.dt_box7, self.boxes_lidar, self.dt_off, self.overflow)
        self.n_frames += B
        self.rows_bound = min(self.rows_bound + B * P, self.capacity)
        self.frame_ids += list(batch_dict["frame_id"]) if "frame_id" in batch_dict else [None] * B
        self._n_dt = None

    # ---------------------------------------------------------------------------------------------------------- at the end
    @property
    def n_detections(self):
        """Rows written so far, as tables() read it (None before that read and after a later add_batch)."""
        return self._n_dt

    def _check(self, overflow):
        if int(overflow):
            raise RuntimeError(f"the split has more detections than the tables' {self.capacity} rows")

    def recall_dict(self):
        """The reference's recall_dict summed over the batches so far: gt, roi_<t> (no ROI head here: 0) and rcnn_<t>.  ONE read."""
        r = _read(self.recall)
        out = {"gt": int(r[0])}
        for i, t in enumerate(self.thresholds):
            out["roi_%s" % str(t)] = 0
            out["rcnn_%s" % str(t)] = int(r[1 + i])
        return out

    def det_annos(self, frame_ids=None):
        """The host list of annotation dicts (kitti_dataset.py:261-303), frame by frame, for result.pkl and the txt files.  ONE read
        (of the rows written so far when tables() has told how many they are, else of as many as the batches could hold)."""
        F = self.n_frames
        n = self._n_dt if self._n_dt is not None else self.rows_bound
        parts = [self.dt_rows[:n], self.boxes_lidar[:n], self.dt_label[:n], self.dt_off[:F + 1], self.overflow]
        sizes = [p.numel() * p.element_size() for p in parts]
        buf = _read(torch.cat([p.reshape(-1).view(torch.uint8) for p in parts]))
        cut = np.cumsum([0] + sizes)
        rows, lidar, label, off, over = (buf[cut[i]:cut[i + 1]].view(dt) for i, dt in
                                         enumerate((np.float64, np.float32, np.int32, np.int64, np.int32)))
        self._check(over[0])
        rows, lidar = rows.reshape(-1, KD.ROW), lidar.reshape(-1, 7)
        names = np.array(self.class_names)
        ids = list(frame_ids) if frame_ids is not None else self.frame_ids
        annos = []
        for f in range(F):
            a, b = int(off[f]), int(off[f + 1])
            k = b - a
            d = {"name": np.zeros(k), "truncated": np.zeros(k), "occluded": np.zeros(k), "alpha": np.zeros(k), "bbox": np.zeros((k, 4)),
                 "dimensions": np.zeros((k, 3)), "location": np.zeros((k, 3)), "rotation_y": np.zeros(k), "score": np.zeros(k),
                 "boxes_lidar": np.zeros((k, 7))}
            if k:
                r = rows[a:b].astype(np.float32)           # the rows are float32 values widened at the store: exact
                d.update(name=names[label[a:b] - 1], alpha=r[:, 4], bbox=r[:, 0:4], dimensions=r[:, 8:11], location=r[:, 5:8],
                         rotation_y=r[:, 11], score=r[:, 14], boxes_lidar=lidar[a:b].copy())
            d["frame_id"] = ids[f] if f < len(ids) else None
            annos.append(d)
        return annos

    def tables(self, gt_annos):
        """kitti_eval_device.AnnoTables over the frames added so far, the detection side as it lies on the device.  ONE read: the
        number of detections, the number of detection x ground-truth pairs, the overflow flag."""
        F = self.n_frames
        if len(gt_annos) != F:
            raise ValueError(f"{len(gt_annos)} ground-truth frames for {F} frames of detections")
        ng = np.array([len(a["name"]) for a in gt_annos], np.int64)
        gt_off = torch.from_numpy(np.concatenate([[0], np.cumsum(ng)]).astype(np.int64)).to(self.device, non_blocking=True)
        dt_off = self.dt_off[:F + 1]
        pair_off = KD.device_pair_off(dt_off, gt_off)
        n_dt, n_pairs, over = (int(v) for v in _read(torch.cat([dt_off[-1:], pair_off[-1:], self.overflow.to(torch.int64)])))
        self._check(over)
        self._n_dt = n_dt
        return KD.AnnoTables.from_device(gt_annos, self.dt_rows, self.dt_cls, self.dt_box7, dt_off, n_dt, n_pairs, pair_off=pair_off)

    def evaluate(self, gt_annos):
        """(text, dict) of kitti_eval.get_official_eval_result, the per-frame work by kitti_eval_device.eval_class on the device
        tables.  The host evaluator decides on AOS from the first detection's alpha (-10 means none); alpha is always formed here,
        so AOS is reported whenever there is a detection."""
        t = self.tables(gt_annos)
        first = [{"alpha": np.zeros(1 if t.n_dt else 0)}]
        return kitti_eval.get_official_eval_result(
            gt_annos, first, self.class_names,
            eval_class_fn=lambda gts, dts, classes, metric, mo, compute_aos: KD.eval_class(t, classes, metric, mo, compute_aos))


def write_kitti_txt(annos, output_dir):
    """The per-frame result files of kitti_dataset.py:305-318."""
    for a in annos:
        with open(output_dir / ("%s.txt" % a["frame_id"]), "w") as f:
            bbox, loc, dims = a["bbox"], a["location"], a["dimensions"]
            for i in range(len(bbox)):
                print("%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f"
                      % (a["name"][i], a["alpha"][i], bbox[i][0], bbox[i][1], bbox[i][2], bbox[i][3], dims[i][1], dims[i][2], dims[i][0],
                         loc[i][0], loc[i][1], loc[i][2], a["rotation_y"][i], a["score"][i]), file=f)


def post_max_of(cfg, class_names=None):
    """Rows per frame of the sync=False records of cfg's post-processing: NMS_POST_MAXSIZE, per class with MULTI_CLASSES_NMS."""
    ncfg = cfg.MODEL.POST_PROCESSING.NMS_CONFIG
    post = int(ncfg.NMS_POST_MAXSIZE)
    if ncfg.get("MULTI_CLASSES_NMS", False):
        post *= len(class_names if class_names is not None else cfg.CLASS_NAMES)
    return post


def eval_one_epoch_device(cfg, model, batches, gt_annos, epoch_id=None, logger=None, save_to_file=False, result_dir=None,
                          log_every=0, class_names=None, epilogue=None):
    """The reference's eval_one_epoch (tools/eval_utils/eval_utils.py:22-127) over DeviceEvalEpilogue: the model is called with
    sync=False, nothing is read back per batch, and the returned dict is the reference's — recall/roi_<t>, recall/rcnn_<t> and the
    AP keys.  batches: the collated batch dicts (load_data_to_gpu is applied); gt_annos: the split's ground-truth annotation dicts
    in frame order.  Every `log_every` batches (0: never) the running recall is read and offered as statistics_info's progress text
    to logger.info.  With result_dir, result.pkl is written (and the txt files with save_to_file).  Single rank only."""
    from .detector import load_data_to_gpu
    pp = cfg.MODEL.POST_PROCESSING
    thresholds = list(pp.RECALL_THRESH_LIST)
    class_names = list(class_names if class_names is not None else cfg.CLASS_NAMES)
    # sized on the host before anything is launched: more than the evaluator's rows per frame raises here
    ep = epilogue if epilogue is not None else DeviceEvalEpilogue(class_names, thresholds, len(gt_annos), post_max_of(cfg, class_names))
    info = logger.info if logger is not None else (lambda s: None)
    info("*************** EPOCH %s EVALUATION *****************" % epoch_id)
    model.eval()
    for i, batch_dict in enumerate(batches):
        load_data_to_gpu(batch_dict)
        with torch.no_grad():
            pred_dicts, _, _ = model(batch_dict, sync=False)
        ep.add_batch(batch_dict, pred_dicts)
        if log_every and (i + 1) % log_every == 0:
            r, t0 = ep.recall_dict(), str(thresholds[0])
            info("recall_%s: (%d, %d) / %d" % (t0, r["roi_" + t0], r["rcnn_" + t0], r["gt"]))
    info("*************** Performance of EPOCH %s *****************" % epoch_id)
    recall = ep.recall_dict()
    ret = {}
    gt_num = recall["gt"]
    for t in thresholds:
        ret["recall/roi_%s" % str(t)] = recall["roi_%s" % str(t)] / max(gt_num, 1)
        ret["recall/rcnn_%s" % str(t)] = recall["rcnn_%s" % str(t)] / max(gt_num, 1)
        info("recall_roi_%s: %f" % (t, ret["recall/roi_%s" % str(t)]))
        info("recall_rcnn_%s: %f" % (t, ret["recall/rcnn_%s" % str(t)]))
    text, ap = ep.evaluate(gt_annos)                        # reads the totals: the number of detections is known from here on
    info("Average predicted number of objects(%d samples): %.3f" % (ep.n_frames, ep.n_detections / max(1, ep.n_frames)))
    if result_dir is not None:
        result_dir.mkdir(parents=True, exist_ok=True)
        annos = ep.det_annos()
        with open(result_dir / "result.pkl", "wb") as f:
            pickle.dump(annos, f)
        if save_to_file:
            out = result_dir / "final_result" / "data"
            out.mkdir(parents=True, exist_ok=True)
            write_kitti_txt(annos, out)
        info("Result is save to %s" % result_dir)
    info(text)
    ret.update(ap)
    info("****************Evaluation done.*****************")
    return ret
