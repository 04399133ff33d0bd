"""GPU: the evaluation epilogue on the device (hvpr_amd/eval_loop.py, csrc/eval_tail.hip).

Recall: hvpr_recall_record_f32 against Detector3DTemplate.generate_recall_record looped over the frames — equal integers, best IoU
bit-equal to boxes_iou3d_gpu(...).max(0).  Annotations: hvpr_prediction_annos_f32 against fixture G20 (the reference's own
generate_prediction_dicts), per field |device - f64| <= 4 * max|reference fp32 - f64| + 2^-23 * max|field|, f64 being
eval_tail_cases.annos_f64; clipped edges, names, scores and dimensions exact.  Whole path: the real 3-class detector, batch 2,
sync=False, no synchronising call in add_batch, a bounded number of reads, and eval_one_epoch_device against G20's loop record."""
import numpy as np
import pytest
import torch

from eval_tail_cases import FIELDS, G20, annos_f64
from hvpr_amd import eval_loop, iou3d_nms_utils, kernels, kitti_eval, kitti_eval_device as KD
from hvpr_amd.detector import Detector3DTemplate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = {1: [3.9, 1.6, 1.56], 2: [0.8, 0.6, 1.73], 3: [1.76, 0.6, 1.73]}
_CACHE = {}


def g20():
    if "g20" not in _CACHE:
        _CACHE["g20"] = G20()
    return _CACHE["g20"]


# ------------------------------------------------------------------------------------------------ recall
def recall_scene(sizes, seed, P=70, G=70):
    """Padded (B, P, 7) predictions with counts and a (B, G, 8) ground-truth table for frames of (n_pred, n_gt) live rows: the
    ground truths are predictions moved a little (every IoU range occurs), the rows past a frame's count hold boxes that WOULD
    match a ground truth (they must be ignored), the rows past the ground truths are zero."""
    rng = np.random.default_rng(seed)
    B = len(sizes)
    pred, gt, count = np.zeros((B, P, 7), np.float32), np.zeros((B, G, 8), np.float32), np.zeros((B,), np.int32)
    for b, (n, m) in enumerate(sizes):
        k = max(n, m, 1)
        lab = rng.integers(1, 4, k)
        base = np.stack([rng.uniform(5, 60, k), rng.uniform(-30, 30, k), rng.uniform(-1.2, -0.6, k)], 1)
        boxes = np.concatenate([base, np.array([SIZES[int(l)] for l in lab]) * rng.uniform(0.9, 1.1, (k, 3)), rng.uniform(-3.1, 3.1, (k, 1))], 1)
        pred[b, :n] = boxes[:n]
        moved = boxes[:m].copy()
        moved[:, 0] += rng.choice([0.0, 0.05, 0.2, 0.5, 1.0, 8.0], m)
        moved[:, 6] += rng.choice([0.0, 0.05, 0.4], m)
        gt[b, :m, :7], gt[b, :m, 7] = moved, lab[:m]
        pred[b, n:] = moved[0] if m else boxes[0]
        count[b] = n
    return pred, count, gt


def host_recall(pred, count, gt, thresholds):
    """The yardstick, frame by frame -> (B, 1 + T) integers and the list of best-IoU rows."""
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    rows, best = [], []
    for b in range(len(pred)):
        r = Detector3DTemplate.generate_recall_record(p[b, :count[b]], {}, b, {"gt_boxes": g}, thresholds)
        rows.append([r["gt"]] + [r["rcnn_%s" % str(t)] for t in thresholds])
        best.append(iou3d_nms_utils.boxes_iou3d_gpu(p[b, :count[b]], g[b, :r["gt"], :7]).max(dim=0)[0].cpu().numpy()
                    if count[b] and r["gt"] else None)
    return np.array(rows, np.int64), best


def device_recall(pred, count, gt, thresholds):
    p, c, g = (torch.from_numpy(a).to(DEV) for a in (pred, count, gt))
    best = torch.full((gt.shape[0], gt.shape[1]), -7.0, dtype=torch.float32, device=DEV)
    counts = kernels.recall_record(p, c, g, thresholds, best_iou=best)
    return counts.cpu().numpy(), best.cpu().numpy()


ALL_SIZES = [(n, m) for n in (0, 1, 63, 64, 65) for m in (0, 1, 64, 65)]
CASES = {(1, 1): [(65, 65)], (3, 3): [(0, 1), (64, 64), (1, 0)], (17, 3): ALL_SIZES[:16] + [(65, 65)], (3, 1): [(63, 65), (65, 1), (0, 0)]}


@pytest.mark.parametrize("B,T", sorted(CASES))
def test_recall_counters_equal_the_host_loop(B, T):
    thresholds = [0.3, 0.5, 0.7][:T] if T == 3 else [0.5]
    sizes = CASES[B, T]
    assert len(sizes) == B
    pred, count, gt = recall_scene(sizes, 100 + B)
    want, want_best = host_recall(pred, count, gt, thresholds)
    got, best = device_recall(pred, count, gt, thresholds)
    assert np.array_equal(got, want), (got, want)
    assert [int(w[0]) for w in want] == [max(m, 1) for _, m in sizes]            # no live row still counts row 0
    for b, (n, m) in enumerate(sizes):
        k = int(want[b, 0])
        if want_best[b] is not None:
            assert np.array_equal(best[b, :k], want_best[b]), b
        else:
            assert (best[b, :k] == 0).all()
        assert (best[b, k:] == 0).all()
    if B > 1:
        assert want[:, 1:].sum() > 0 and (want[:, -1] < want[:, 0]).any()
    again, best2 = device_recall(pred, count, gt, thresholds)
    assert again.tobytes() == got.tobytes() and best2.tobytes() == best.tobytes()


def test_recall_trim_and_identical_boxes():
    car = [20.0, 3.0, -0.9, 3.9, 1.6, 1.56, 0.4]
    pred = np.zeros((4, 3, 7), np.float32)
    pred[:, 0], pred[:, 1] = car, [40.0, -8.0, -0.8, 0.8, 0.6, 1.73, 1.0]
    count = np.array([2, 2, 2, 2], np.int32)
    gt = np.zeros((4, 6, 8), np.float32)
    # frame 0: all rows zero -> one box.  frame 1: a zero row and a cancelling row in the middle stay, the identical box is recalled
    gt[1, 0, :7], gt[1, 2, :2], gt[1, 4, :7] = car, [2.0, -2.0], pred[0, 1]
    # frame 2: a non-zero row whose sum cancels to exactly 0 at the tail is cut, with the zero row behind it
    gt[2, 0, :7], gt[2, 1, :7], gt[2, 2, :3] = car, [21.0, 3.0, -0.9, 3.9, 1.6, 1.56, 0.4], [4.0, -1.0, -3.0]
    # frame 3: only a cancelling row, at row 0: never cut
    gt[3, 0, :2] = [1.5, -1.5]
    thresholds = [0.3, 0.5, 0.7]
    want, want_best = host_recall(pred, count, gt, thresholds)
    got, best = device_recall(pred, count, gt, thresholds)
    assert want[:, 0].tolist() == [1, 5, 2, 1]
    assert np.array_equal(got, want), (got, want)
    assert got[1].tolist() == [5, 2, 2, 2] and got[2, 1] == 2 and got[2, 3] == 1
    assert best[1, 0] > 0.99 and best[1, 4] > 0.99 and best[1, 0] == want_best[1][0]
    for b in range(4):
        assert np.array_equal(best[b, :want[b, 0]], want_best[b])


def test_recall_empty_shapes_and_refusals():
    pred, count, gt = recall_scene([(5, 4), (0, 2)], 7, P=8, G=6)
    p, c, g = (torch.from_numpy(a).to(DEV) for a in (pred, count, gt))
    thr = [0.3, 0.5, 0.7]
    # no ground-truth rows at all: nothing is counted, as the host loop finds
    assert (kernels.recall_record(p, c, g[:, :0].contiguous(), thr).cpu().numpy() == 0).all()
    assert host_recall(pred, count, gt[:, :0], thr)[0].sum() == 0
    # no prediction rows: the ground truths are counted, none recalled
    got = kernels.recall_record(p[:, :0].contiguous(), c, g, thr).cpu().numpy()
    assert got.tolist() == [[4, 0, 0, 0], [2, 0, 0, 0]]
    assert kernels.recall_record(p, c, g, []).cpu().numpy().tolist() == [[4], [2]]          # T = 0
    # refusals touch nothing
    counts = torch.full((2, 10), -7, dtype=torch.int32, device=DEV)
    best = torch.full((2, 6), -7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="hvpr_recall_record_f32"):
        kernels.recall_record(p, c, g, [0.1 * i for i in range(1, 10)], counts=counts, best_iou=best)
    with pytest.raises(RuntimeError, match="hvpr_recall_record_f32"):
        kernels.recall_record(p, c, g[:, :, :6].contiguous(), thr, counts=counts[:, :4].contiguous(), best_iou=best)
    torch.cuda.synchronize()
    assert (counts == -7).all() and (best == -7).all()


def padded_records(frames, P, device=DEV, adjacent=True):
    """sync=False records of a batch from per-frame (boxes, scores, labels): padded to P rows with copies of row 0 of the batch's
    first non-empty frame (a live-looking box that must be ignored), as views of one batched tensor or as tensors of their own."""
    B = len(frames)
    fill = next((f for f in frames if len(f[0])), (np.array([[9.0, 1.0, -1.0, 3.9, 1.6, 1.56, 0.2]], np.float32), np.array([0.5], np.float32), np.array([1])))
    boxes, scores, labels = np.zeros((B, P, 7), np.float32), np.zeros((B, P), np.float32), np.zeros((B, P), np.int64)
    boxes[:], scores[:], labels[:] = fill[0][0], fill[1][0], fill[2][0]
    for b, (bx, sc, lb) in enumerate(frames):
        boxes[b, :len(bx)], scores[b, :len(bx)], labels[b, :len(bx)] = bx, sc, lb
    count = torch.tensor([len(f[0]) for f in frames], dtype=torch.int32, device=device)
    tb, ts, tl = (torch.from_numpy(a).to(device) for a in (boxes, scores, labels))
    own = (lambda t: t) if adjacent else (lambda t: t.clone())
    return [{"pred_boxes": own(tb[b]), "pred_scores": own(ts[b]), "pred_labels": own(tl[b]), "pred_count": own(count[b:b + 1])} for b in range(B)]


def g20_batch(k, with_gt=True):
    g = g20()
    bd = g.batch_dict(k)
    if with_gt:
        bd["gt_boxes"] = torch.from_numpy(bd["gt_boxes"]).to(DEV)
    else:
        del bd["gt_boxes"]
    return bd, [g.pred(f) for f in range(k * g.batch, (k + 1) * g.batch)]


def g20_epilogue(adjacent=True, with_gt=True, **kw):
    g = g20()
    ep = eval_loop.DeviceEvalEpilogue(g.class_names, g.thresholds, g.n_frames, 12, **kw)
    for k in range(g.n_frames // g.batch):
        bd, frames = g20_batch(k, with_gt)
        ep.add_batch(bd, padded_records(frames, 12, adjacent=adjacent))
    return ep


def test_recall_counters_of_the_fixture():
    g = g20()
    for k in range(3):
        bd, frames = g20_batch(k)
        recs = padded_records(frames, 12)
        c = kernels.recall_record(torch.stack([r["pred_boxes"] for r in recs]), torch.cat([r["pred_count"] for r in recs]), bd["gt_boxes"],
                                  g.thresholds).sum(dim=0).cpu().numpy()
        want = g.recall(k)
        assert c.tolist() == [want["gt"]] + [want["rcnn_%s" % str(t)] for t in g.thresholds], k
    ep = g20_epilogue()
    assert ep.recall_dict() == g.recall()
    none = g20_epilogue(with_gt=False)                      # gt_boxes absent from the dict: the counters stay untouched
    assert none.recall_dict() == {k: 0 for k in g.recall()}


# ------------------------------------------------------------------------------------------------ annotations
@pytest.mark.parametrize("adjacent", [True, False])
def test_annotations_against_the_fixture(adjacent, observed):
    g = g20()
    ep = g20_epilogue(adjacent=adjacent)
    annos = ep.det_annos()
    assert len(annos) == 6 and [a["frame_id"] for a in annos] == g.frame_id
    worst = {}
    n_clipped = 0
    for f, a in enumerate(annos):
        boxes, scores, labels = g.pred(f)
        ref = g.anno(f)
        assert sorted(a) == sorted(list(ref) + ["frame_id"])
        assert a["name"].shape == ref["name"].shape and a["bbox"].shape == ref["bbox"].shape and a["boxes_lidar"].shape == ref["boxes_lidar"].shape
        if not len(boxes):
            continue
        f64 = annos_f64(boxes, g.calibs[g.calib_of[f]], g.image_shape[f])
        f64["score"] = scores.astype(np.float64)
        assert list(a["name"]) == list(ref["name"])
        assert a["score"].tobytes() == ref["score"].tobytes() and a["dimensions"].tobytes() == ref["dimensions"].tobytes()
        assert (a["truncated"] == 0).all() and (a["occluded"] == 0).all()
        for k in FIELDS:
            assert a[k].dtype == ref[k].dtype == np.float32, k
            ref_err = float(np.abs(ref[k].astype(np.float64) - f64[k]).max())
            dev_err = float(np.abs(a[k].astype(np.float64) - f64[k]).max())
            bar = 4 * ref_err + 2.0 ** -23 * float(np.abs(f64[k]).max())
            w = worst.setdefault(k, [0.0, 0.0])
            w[0], w[1] = max(w[0], dev_err), max(w[1], ref_err)
            assert dev_err <= bar, (f, k, dev_err, ref_err, bar)
        h, w_ = g.image_shape[f]
        lo, hi = np.zeros(4), np.array([w_ - 1, h - 1, w_ - 1, h - 1], np.float64)
        out = (f64["edges"] < lo) | (f64["edges"] > hi)                             # the fixture keeps these >= 1 px outside
        assert np.array_equal(a["bbox"][out], np.where(f64["edges"] < lo, lo, hi)[out].astype(np.float32))
        assert np.array_equal(a["bbox"][out], ref["bbox"][out])
        n_clipped += int(out.sum())
    assert n_clipped >= 8
    observed("eval tail G20 |device - f64| (|reference - f64|): " + ", ".join(f"{k} {v[0]:.2e} ({v[1]:.2e})" for k, v in worst.items()))


def test_tables_are_in_the_evaluators_layout():
    g = g20()
    ep = g20_epilogue()
    annos = ep.det_annos()
    want = KD.AnnoTables([g.gt_anno(f) for f in range(6)], annos)
    got = ep.tables([g.gt_anno(f) for f in range(6)])
    assert (got.n_dt, got.n_pairs, got.n_gt, got.n_frames) == (28, want.n_pairs, want.n_gt, 6)
    d = got.dev
    assert np.array_equal(d["dt_off"].cpu().numpy(), want.dt_off) and np.array_equal(d["pair_off"].cpu().numpy(), want.pair_off)
    assert np.array_equal(d["dt_rows"][:28].cpu().numpy(), want.dt_rows) and (want.dt_rows[:, 12:14] == 0).all()
    assert np.array_equal(d["dt_cls"][:28].cpu().numpy(), want.dt_cls) and np.array_equal(d["dt_box7"][:28].cpu().numpy(), want.dt_box7)
    for k in ("gt_rows", "gt_cls", "gt_dontcare", "gt_box7", "gt_off"):
        assert np.array_equal(d[k].cpu().numpy(), getattr(want, k)), k


def _tables(cap, guard, max_frames, dev=DEV):
    t = {"dt_rows": torch.full((cap + guard, 16), -7.0, dtype=torch.float64, device=dev), "dt_cls": torch.full((cap + guard,), -7, dtype=torch.int32, device=dev),
         "dt_label": torch.full((cap + guard,), -7, dtype=torch.int32, device=dev), "dt_box7": torch.full((cap + guard, 7), -7.0, device=dev),
         "boxes_lidar": torch.full((cap + guard, 7), -7.0, device=dev), "dt_off": torch.zeros((max_frames + 1,), dtype=torch.int64, device=dev),
         "row_base": torch.zeros((1,), dtype=torch.int64, device=dev), "overflow": torch.zeros((1,), dtype=torch.int32, device=dev)}
    return t


def _annos_call(t, cap, recs, calib, frame_base):
    B = len(recs)
    kernels.prediction_annos(torch.stack([r["pred_boxes"] for r in recs]), torch.stack([r["pred_scores"] for r in recs]),
                             torch.stack([r["pred_labels"] for r in recs]), torch.cat([r["pred_count"] for r in recs]), calib, [0, 1, 2],
                             t["row_base"], frame_base, t["dt_rows"][:cap], t["dt_cls"][:cap], t["dt_label"][:cap], t["dt_box7"][:cap],
                             t["boxes_lidar"][:cap], t["dt_off"], t["overflow"])
    assert B == calib.shape[0]


def test_compaction_counts_offsets_and_overflow():
    g = g20()
    P = 5
    b5, s5, l5 = g.pred(2)                                    # five boxes: a frame filled to P
    frames = [(b5[:0], s5[:0], l5[:0]), (b5[:1], s5[:1], l5[:1]), (b5, s5, l5)]
    calib = torch.from_numpy(eval_loop.pack_calib([g.calibs[0]] * 3, [g.image_shape[2]] * 3)).to(DEV)
    t = _tables(12, 4, 6)
    _annos_call(t, 12, padded_records(frames, P), calib, 0)
    _annos_call(t, 12, padded_records(frames[::-1], P), calib, 3)              # continues where the first call ended
    assert t["dt_off"].cpu().tolist() == [0, 0, 1, 6, 11, 12, 12] and int(t["row_base"]) == 12 and int(t["overflow"]) == 0
    rows = t["dt_rows"].cpu().numpy()
    assert (rows[:12, 14] == np.concatenate([s5[:1], s5, s5, s5[:1]])).all() and (rows[12:] == -7).all()      # no gap, nothing after
    assert np.array_equal(rows[1:6], rows[6:11]) and np.array_equal(rows[0], rows[11])
    assert t["dt_label"].cpu().tolist() == np.concatenate([l5[:1], l5, l5, l5[:1], [-7] * 4]).tolist()
    assert (t["boxes_lidar"][12:] == -7).all() and (t["dt_box7"][12:] == -7).all() and (t["dt_cls"][12:] == -7).all()
    # one row short: the flag is set, offsets stop at cap, nothing is written past it
    t = _tables(11, 5, 6)
    _annos_call(t, 11, padded_records(frames, P), calib, 0)
    _annos_call(t, 11, padded_records(frames[::-1], P), calib, 3)
    assert int(t["overflow"]) == 1 and t["dt_off"].cpu().tolist() == [0, 0, 1, 6, 11, 11, 11] and int(t["row_base"]) == 11
    short = t["dt_rows"].cpu().numpy()
    assert np.array_equal(short[:11], rows[:11]) and (short[11:] == -7).all() and (t["dt_label"][11:] == -7).all()
    assert (t["boxes_lidar"][11:] == -7).all() and (t["dt_box7"][11:] == -7).all() and (t["dt_cls"][11:] == -7).all()
    # a refusal (more frames than dt_off holds) touches nothing
    t = _tables(12, 4, 2)
    with pytest.raises(RuntimeError, match="hvpr_prediction_annos_f32"):
        _annos_call(t, 12, padded_records(frames, P), calib, 0)
    torch.cuda.synchronize()
    assert (t["dt_rows"] == -7).all() and (t["dt_off"] == 0).all() and int(t["row_base"]) == 0
    # through the epilogue, the overflow surfaces at the read
    ep = g20_epilogue(capacity=27)
    with pytest.raises(RuntimeError, match="more detections"):
        ep.det_annos()
    with pytest.raises(ValueError, match="MULTI_CLASSES_NMS"):
        ep2 = eval_loop.DeviceEvalEpilogue(g.class_names, g.thresholds, 6, 12)
        bd, fr = g20_batch(0)
        ep2.add_batch(bd, [{k: v for k, v in r.items() if k != "pred_count"} for r in padded_records(fr, 12)])


# ------------------------------------------------------------------------------------------------ the whole path
def _detector_scene():
    """Six synthetic frames through the real 3-class detector in batches of two: per batch the dict after the forward pass (with a
    ground-truth table made from its own detections) and the host yardstick's sync=True records and recall."""
    if "scene" in _CACHE:
        return _CACHE["scene"]
    from hvpr_amd import detector, synthetic, synthetic_weights
    from hvpr_amd.config import hvpr_3class_cfg
    g = g20()
    cfg = hvpr_3class_cfg()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
    synthetic_weights.load_synthetic(model, seed=5, cls_bias=-2.0)
    with torch.no_grad():
        model.dense_head.conv_cls.bias += torch.tensor([0.0, -0.2, 0.1] * 6)
    model = model.to(DEV).eval()
    batches = []
    for k in range(3):
        frames = [synthetic.hvpr_frame(70 + 2 * k), synthetic.hvpr_frame(71 + 2 * k)[:12000 + 1000 * k]]
        pts = np.concatenate([np.concatenate([np.full((len(f), 1), b, np.float32), f], 1) for b, f in enumerate(frames)])
        host_keys = {"frame_id": ["%06d" % (2 * k + b) for b in range(2)], "calib": [g.calibs[(k + b) % 2] for b in range(2)],
                     "image_shape": np.stack([g.image_shape[(k + b) % 2 + 2] for b in range(2)])}
        with torch.no_grad():
            preds, _, bd = model({"points": torch.from_numpy(pts).to(DEV), "batch_size": 2, **host_keys})
        bd.update(host_keys)
        gt = np.zeros((2, 7, 8), np.float32)
        for b in range(2):
            pb, pl = preds[b]["pred_boxes"].cpu().numpy(), preds[b]["pred_labels"].cpu().numpy()
            far = np.nonzero(pb[:, 0] > 8.0)[0][:5]
            gt[b, :len(far), :7], gt[b, :len(far), 7] = pb[far], pl[far]
            gt[b, :len(far), 0] += np.array([0.0, 0.1, 0.3, 0.6, 5.0])[:len(far)]
        bd["gt_boxes"] = torch.from_numpy(gt).to(DEV)
        with torch.no_grad():
            preds_s, recall_s, _ = model.post_processing(bd, sync=True)
        batches.append((bd, preds_s, recall_s, gt))
    cls = list(cfg.CLASS_NAMES)
    host_annos, gt_annos = [], []
    for bd, preds_s, _, gt in batches:
        host_annos += kitti_eval.generate_prediction_dicts(bd, preds_s, cls)
        for b in range(2):
            rows = gt[b][np.abs(gt[b]).sum(1) > 0]
            cam = kitti_eval.boxes3d_lidar_to_kitti_camera(rows[:, :7], bd["calib"][b])
            n = len(rows)
            gt_annos.append({"name": np.array([cls[int(c) - 1] for c in rows[:, 7]], dtype="<U16"), "truncated": np.zeros(n), "occluded": np.zeros(n, np.int64),
                             "alpha": (-np.arctan2(-rows[:, 1], rows[:, 0]) + cam[:, 6]).astype(np.float64),
                             "bbox": kitti_eval.boxes3d_kitti_camera_to_imageboxes(cam, bd["calib"][b], bd["image_shape"][b]).astype(np.float64).reshape(-1, 4),
                             "dimensions": cam[:, 3:6].astype(np.float64), "location": cam[:, 0:3].astype(np.float64), "rotation_y": cam[:, 6].astype(np.float64)})
    _CACHE["scene"] = (model, cfg, batches, host_annos, gt_annos)
    return _CACHE["scene"]


def test_whole_path_without_a_host_read_per_batch(observed):
    model, cfg, batches, host_annos, gt_annos = _detector_scene()
    cls = list(cfg.CLASS_NAMES)
    thr = list(cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST)
    post = int(cfg.MODEL.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE)
    ep = eval_loop.DeviceEvalEpilogue(cls, thr, 6, post)
    records = []
    with torch.no_grad():
        for bd, _, _, _ in batches:
            records.append(model.post_processing(bd, sync=False)[0])
    torch.cuda.synchronize()
    reads0 = eval_loop.N_READS
    torch.cuda.set_sync_debug_mode("error")
    try:
        for (bd, _, _, _), recs in zip(batches, records):
            ep.add_batch(bd, recs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert eval_loop.N_READS == reads0
    # recall: the sum of the host loop's per-batch records
    want = {}
    for _, _, r, _ in batches:
        for k, v in r.items():
            want[k] = want.get(k, 0) + v
    assert ep.recall_dict() == want and want["gt"] > 0 and want["rcnn_%s" % str(thr[0])] > 0
    text, ap = ep.evaluate(gt_annos)
    assert eval_loop.N_READS - reads0 <= 3
    # annotations: the host formatter on the sync=True records of the same batches
    annos = ep.det_annos()
    assert [len(a["name"]) for a in annos] == [len(a["name"]) for a in host_annos] and sum(len(a["name"]) for a in annos) > 20
    worst = {}
    for f, (a, h) in enumerate(zip(annos, host_annos)):
        bd, preds_s = batches[f // 2][0], batches[f // 2][1]
        boxes = preds_s[f % 2]["pred_boxes"].cpu().numpy()
        f64 = annos_f64(boxes, bd["calib"][f % 2], bd["image_shape"][f % 2])
        f64["score"] = preds_s[f % 2]["pred_scores"].cpu().numpy().astype(np.float64)
        assert a["frame_id"] == h["frame_id"] and list(a["name"]) == list(h["name"])
        assert a["score"].tobytes() == h["score"].tobytes() and a["dimensions"].tobytes() == np.asarray(h["dimensions"], np.float32).tobytes()
        near = int((f64["depth"] < 2.0).any(axis=1).sum())                 # nearer to the image plane than the fixture's boxes
        for k in FIELDS:
            ref = np.asarray(h[k], np.float64)
            if k == "boxes_lidar":                                     # the fixture decides: the bottom-centre z
                assert np.array_equal(ref[:, 2], boxes[:, 2]) and np.array_equal(a[k][:, 2], boxes[:, 2] - boxes[:, 5] / 2)
                ref = ref.copy()
                ref[:, 2] = boxes[:, 2] - boxes[:, 5] / 2
            ref_err = float(np.abs(ref - f64[k]).max())
            dev_err = float(np.abs(a[k].astype(np.float64) - f64[k]).max())
            w = worst.setdefault(k, [0.0, 0.0, 0, 0])
            w[0], w[1] = max(w[0], dev_err), max(w[1], ref_err)
            w[2] += int((a[k].astype(np.float64) != ref).sum())
            assert dev_err <= 4 * ref_err + 2.0 ** -23 * float(np.abs(f64[k]).max()), (f, k, dev_err, ref_err)
        worst["bbox"][3] += near
    observed("eval tail detector scene |device - f64| (|host - f64|) [elements unequal to the host's]: "
             + ", ".join(f"{k} {v[0]:.2e} ({v[1]:.2e}) [{v[2]}]" for k, v in worst.items())
             + f"; {worst['bbox'][3]} of {sum(len(a['name']) for a in annos)} boxes have a corner nearer than 2 m")
    # AP: the device tables against the device evaluator run on the host formatter's annotations
    text_h, ap_h = KD.get_official_eval_result(gt_annos, host_annos, cls)
    assert sorted(ap) == sorted(ap_h) and len(ap) == 36
    for k, v in ap_h.items():
        assert abs(ap[k] - v) < 1e-9, (k, ap[k], v)
    assert text.splitlines() == text_h.splitlines() and max(ap.values()) > 0
    # and the tables built on the device against the constructor's on the host copy of the same rows
    text_c, ap_c = KD.get_official_eval_result(gt_annos, annos, cls)
    assert ap_c == ap and text_c.splitlines() == text.splitlines()


class _CannedModel:
    """The model of G20's loop record: returns the canned detections as sync=False records."""

    def __init__(self, log):
        self.k, self.log = 0, log

    def eval(self):
        self.log.append("model.eval")

    def __call__(self, batch_dict, sync=True):
        assert sync is False
        self.log.append("model(batch)")
        g = g20()
        recs = padded_records([g.pred(f) for f in range(self.k * g.batch, (self.k + 1) * g.batch)], 12)
        self.k += 1
        return recs, {}, batch_dict


class _LoggedEpilogue(eval_loop.DeviceEvalEpilogue):
    """Writes the device loop's steps under the names of the reference's they stand for."""
    log = None

    def add_batch(self, batch_dict, pred_dicts):
        self.log.append("dataset.generate_prediction_dicts")
        return super().add_batch(batch_dict, pred_dicts)

    def evaluate(self, gt_annos):
        self.log.append("dataset.evaluation")
        return super().evaluate(gt_annos)


def test_eval_one_epoch_device_against_the_loop_record(tmp_path, monkeypatch):
    from hvpr_amd import detector
    g = g20()
    cfg = types_cfg(g)
    log = []

    class Logger:
        def info(self, s):
            log.append("logger.info:" + str(s).split("\n")[0][:60])
    real_load = detector.load_data_to_gpu
    monkeypatch.setattr(detector, "load_data_to_gpu", lambda bd: (log.append("load_data_to_gpu"), real_load(bd))[1])
    ep = _LoggedEpilogue(g.class_names, g.thresholds, 6, 12)
    ep.log = log
    batches = [g.batch_dict(k) for k in range(3)]
    ret = eval_loop.eval_one_epoch_device(cfg, _CannedModel(log), batches, [g.gt_anno(f) for f in range(6)], epoch_id=7, logger=Logger(),
                                          result_dir=tmp_path, log_every=2, epilogue=ep)
    want = dict(zip((str(k) for k in g.z["loop.keys"]), g.z["loop.values"]))
    assert sorted(ret) == sorted(want)
    total = g.recall()
    for k, v in want.items():
        if k.startswith("recall/"):
            assert ret[k] == total[k.split("/")[1]] / total["gt"] == v, k            # equal integers behind the ratios
        else:
            assert abs(ret[k] - v) < 1e-3, (k, ret[k], v)
    assert max(v for k, v in want.items() if "3d" in k) > 0
    # the steps in the reference's order: load, model, annotations per batch, then the evaluation
    calls = [str(s) for s in g.z["loop.calls"]]
    steps = lambda seq: [s.split("(")[0] if s.startswith("dataset.evaluation") else s for s in seq if not s.startswith("logger")]
    assert steps(log) == steps(calls) and steps(log)[-1] == "dataset.evaluation" and steps(log).count("load_data_to_gpu") == 3
    assert "logger.info:recall_0.3: (0, 8) / 15" in log                              # statistics_info's text after two batches
    for line in ("logger.info:recall_rcnn_0.3: 0.578947", "logger.info:*************** EPOCH 7 EVALUATION *****************",
                 "logger.info:Average predicted number of objects(6 samples): 4.667", "logger.info:****************Evaluation done.*****************"):
        assert line in log and line in calls, line
    import pickle
    with open(tmp_path / "result.pkl", "rb") as f:
        saved = pickle.load(f)
    assert [a["frame_id"] for a in saved] == g.frame_id and [len(a["name"]) for a in saved] == [0, 1, 5, 12, 3, 7]


def types_cfg(g):
    from hvpr_amd.config import AttrDict
    return AttrDict({"CLASS_NAMES": g.class_names, "MODEL": {"POST_PROCESSING": {"RECALL_THRESH_LIST": g.thresholds, "EVAL_METRIC": "kitti",
                                                                                  "NMS_CONFIG": {"NMS_POST_MAXSIZE": 12}}}})
