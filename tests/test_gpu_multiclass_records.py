"""GPU: hvpr_gather_predictions_multiclass_f32 against numpy, the detector's sync=False MULTI_CLASSES_NMS records against its
sync=True ones, and the device evaluation epilogue on those records against the host route.

The kernel is a gather: integers are compared for equality and floats bit for bit."""
import numpy as np
import pytest
import torch

from hvpr_amd import eval_loop, kernels, kitti_eval, kitti_eval_device as KD

DEV = "cuda:0"
gpu = pytest.mark.gpu


def _ref(boxes, scores, keep, counts, nc):
    """The records in numpy.  boxes (B, A, W), scores (B * nc, A), keep (B * nc, K), counts (B * nc,)."""
    B, K = boxes.shape[0], keep.shape[1]
    P = nc * K
    ob = np.repeat(boxes[:, :1, :7], P, axis=1).copy() if P else np.zeros((B, 0, 7), np.float32)
    os_ = np.repeat(scores.reshape(B, nc, -1)[:, 0, :1], P, axis=1).copy() if P else np.zeros((B, 0), np.float32)
    ol, osel, oc = np.ones((B, P), np.int64), np.zeros((B, P), np.int64), np.zeros((B,), np.int32)
    for b in range(B):
        r = 0
        for k in range(nc):
            s = b * nc + k
            for i in range(min(max(int(counts[s]), 0), K)):
                a = int(keep[s, i])
                ob[b, r], os_[b, r], ol[b, r], osel[b, r] = boxes[b, a, :7], scores[s, a], k + 1, a
                r += 1
        oc[b] = r
    return ob, os_, ol, osel, oc


def _case(B, nc, K, A, counts=None, width=7, gap=0, seed=0):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((B, A + gap, width)).astype(np.float32)       # gap rows: table_stride != A * width
    scores = rng.random((B * nc, A)).astype(np.float32)
    keep = rng.integers(0, max(A, 1), (B * nc, K)).astype(np.int32)
    counts = rng.integers(0, K + 1, (B * nc,)) if counts is None else np.asarray(counts).reshape(-1)
    return table, scores, keep, counts.astype(np.int32)


def _run(table, scores, keep, counts, nc, A):
    t = torch.from_numpy(table).to(DEV)
    boxes = t[:, :A]                                                          # a view when the table has gap rows
    B, K = table.shape[0], keep.shape[1]
    dev = lambda a: torch.from_numpy(a).to(DEV)
    if boxes.is_contiguous():
        out = kernels.gather_predictions_multiclass(boxes, dev(scores), dev(keep), dev(counts), nc)
    else:                                                                     # the C entry point, with the table's own stride
        ob = torch.empty((B, nc * K, 7), device=DEV)
        os_ = torch.empty((B, nc * K), device=DEV)
        ol, osel = torch.empty((B, nc * K), dtype=torch.int64, device=DEV), torch.empty((B, nc * K), dtype=torch.int64, device=DEV)
        oc = torch.empty((B,), dtype=torch.int32, device=DEV)
        s, k, c = dev(scores), dev(keep), dev(counts)
        kernels.check(kernels.lib().hvpr_gather_predictions_multiclass_f32(
            t.data_ptr(), table.shape[2], table.shape[1] * table.shape[2], s.data_ptr(), A, k.data_ptr(), c.data_ptr(), B, nc, K,
            ob.data_ptr(), os_.data_ptr(), ol.data_ptr(), osel.data_ptr(), oc.data_ptr(), kernels._stream()), "multiclass gather")
        out = (ob, os_, ol, osel, oc)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _same(got, want):
    for g, w, name in zip(got, want, ("boxes", "scores", "labels", "selected", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), name


CASES = {
    "smallest": dict(B=1, nc=1, K=1, A=1, counts=[1]),
    "smallest_empty": dict(B=1, nc=1, K=1, A=1, counts=[0]),
    "mixed_counts": dict(B=2, nc=3, K=4, A=8, counts=[[0, 4, 2], [0, 0, 0]]),
    "all_full": dict(B=2, nc=3, K=4, A=8, counts=[[4, 4, 4], [4, 4, 4]]),
    "clamp": dict(B=2, nc=3, K=4, A=8, counts=[[9, 4, 100], [5, -3, 4]]),
    "prefix": dict(B=3, nc=5, K=7, A=33, seed=3),
    "more_than_one_block": dict(B=2, nc=3, K=40, A=300, seed=4),              # 3 * 40 * 8 = 960 threads: four blocks per frame
    "width_and_stride": dict(B=2, nc=3, K=4, A=8, width=9, gap=5, seed=5),
}


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_against_numpy(name):
    c = dict(CASES[name])
    table, scores, keep, counts = _case(**c)
    A, nc = c["A"], c["nc"]
    want = _ref(table[:, :A], scores, keep, counts, nc)
    if name == "mixed_counts":
        assert want[4].tolist() == [6, 0]
    if name == "clamp":
        assert want[4].tolist() == [12, 8]
    _same(_run(table, scores, keep, counts, nc, A), want)


@gpu
def test_kernel_early_returns():
    # K == 0: the counts are zeroed and nothing else is written
    boxes = torch.zeros((2, 4, 7), device=DEV)
    scores = torch.zeros((6, 4), device=DEV)
    keep = torch.zeros((6, 0), dtype=torch.int32, device=DEV)
    kc = torch.full((6,), 3, dtype=torch.int32, device=DEV)
    ob, os_, ol, osel, oc = kernels.gather_predictions_multiclass(boxes, scores, keep, kc, 3)
    assert ob.shape == (2, 0, 7) and os_.shape == ol.shape == osel.shape == (2, 0) and oc.cpu().tolist() == [0, 0]
    # B == 0: nothing is done
    out = kernels.gather_predictions_multiclass(boxes[:0], scores[:0], torch.zeros((0, 5), dtype=torch.int32, device=DEV), kc[:0], 3)
    assert out[0].shape == (0, 15, 7) and out[4].shape == (0,)
    L = kernels.lib()
    assert L.hvpr_gather_predictions_multiclass_f32(None, 7, 0, None, 0, None, None, 0, 3, 5, None, None, None, None, None, None) == 0
    assert L.hvpr_gather_predictions_multiclass_f32(None, 6, 0, None, 0, None, None, 1, 3, 5, None, None, None, None, None, None) != 0
    with pytest.raises(ValueError, match="shapes"):
        kernels.gather_predictions_multiclass(boxes, scores[:5], keep[:5], kc[:5], 3)


# ------------------------------------------------------------------------------------------------ detector
_CACHE = {}


def _model():
    """hvpr_3class with synthetic weights and MULTI_CLASSES_NMS; the class biases leave class 2 (Pedestrian) with nothing above the
    score threshold and the others with something."""
    if "model" not in _CACHE:
        from hvpr_amd import detector, synthetic_weights
        from hvpr_amd.config import hvpr_3class_cfg
        cfg = hvpr_3class_cfg()
        cfg.MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS = True
        model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg))
        synthetic_weights.load_synthetic(model, seed=5, cls_bias=-2.0)
        with torch.no_grad():
            model.dense_head.conv_cls.bias += torch.tensor([0.0, -1.0e6, 0.1] * 6)       # sigmoid(x - 1e6) is 0 for any logit
        _CACHE["model"] = (model.to(DEV).eval(), cfg)
    return _CACHE["model"]


def _forward(B):
    """The batch dict after the forward pass of B synthetic frames (cached), with calibration and a ground-truth table."""
    if ("bd", B) not in _CACHE:
        from hvpr_amd import synthetic
        from eval_tail_cases import G20
        model, cfg = _model()
        g = _CACHE.setdefault("g20", G20())
        frames = [synthetic.hvpr_frame(70 + b)[:20000 - 1500 * b] for b in range(B)]
        pts = np.concatenate([np.concatenate([np.full((len(f), 1), b, np.float32), f], 1) for b, f in enumerate(frames)])
        host = {"frame_id": ["%06d" % b for b in range(B)], "calib": [g.calibs[b % 2] for b in range(B)],
                "image_shape": np.stack([g.image_shape[b % 2 + 2] for b in range(B)])}
        with torch.no_grad():
            preds, _, bd = model({"points": torch.from_numpy(pts).to(DEV), "batch_size": B, **host})
        bd.update(host)
        gt = np.zeros((B, 7, 8), np.float32)
        for b in range(B):
            pb, pl = preds[b]["pred_boxes"].cpu().numpy(), preds[b]["pred_labels"].cpu().numpy()
            far = np.nonzero(pb[:, 0] > 8.0)[0][:5]
            gt[b, :len(far), :7], gt[b, :len(far), 7] = pb[far], pl[far]
            gt[b, :len(far), 0] += np.array([0.0, 0.1, 0.3, 0.6, 5.0])[:len(far)]
        bd["gt_boxes"] = torch.from_numpy(gt).to(DEV)
        _CACHE[("bd", B)] = (bd, gt)
    return _CACHE[("bd", B)]


@gpu
@pytest.mark.parametrize("B", [1, 2, 6])
def test_detector_records_without_a_read(B):
    """B = 6 makes 18 candidate lists, more than kernels.MAX_NMS_SEGMENTS: the chunk join of _nms_of_score_rows is crossed."""
    model, cfg = _model()
    bd, _ = _forward(B)
    nc = len(cfg.CLASS_NAMES)
    post = int(cfg.MODEL.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE)
    assert (B * nc > kernels.MAX_NMS_SEGMENTS) == (B == 6)
    with torch.no_grad():
        want, _, _ = model.post_processing(bd, sync=True)
        model.post_processing(bd, sync=False)                   # workspaces exist before the no-sync run
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got, recall, _ = model.post_processing(bd, sync=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert recall == {} and len(got) == B
    seen = set()
    for b in range(B):
        g, w = got[b], want[b]
        assert g["pred_boxes"].shape == (nc * post, 7) and g["pred_scores"].shape == g["pred_labels"].shape == g["selected"].shape == (nc * post,)
        assert g["pred_count"].shape == (1,) and g["pred_count"].dtype == torch.int32 and g["pred_labels"].dtype == torch.int64
        n = int(g["pred_count"])
        assert n == w["pred_boxes"].shape[0]
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert g[k][:n].cpu().numpy().tobytes() == w[k].cpu().numpy().tobytes(), (b, k)
        seen |= set(w["pred_labels"].cpu().tolist())
        if n < nc * post:                                       # padded rows: anchor 0 of class 0
            assert (g["pred_labels"][n:] == 1).all() and (g["selected"][n:] == 0).all()
            assert torch.equal(g["pred_boxes"][n:], bd["batch_box_preds"][b, :1, :7].expand(nc * post - n, 7))
    assert 2 not in seen and {1, 3} <= seen                     # a class that keeps nothing between two that keep something


# ------------------------------------------------------------------------------------------------ epilogue
@gpu
def test_epilogue_on_multiclass_records_against_the_host_route():
    """The bars of tests/test_gpu_eval_tail.py's whole-path test: recall counters equal, names / scores / dimensions bit-equal,
    every other field within 4 x the host formatter's own float64 error + one float32 ulp of the field's largest value, AP within
    1e-9 of the device evaluator on the host formatter's annotations, the text equal."""
    from eval_tail_cases import FIELDS, annos_f64
    model, cfg = _model()
    cls, thr = list(cfg.CLASS_NAMES), list(cfg.MODEL.POST_PROCESSING.RECALL_THRESH_LIST)
    batches = [_forward(2), _forward(1)]

    class Model:
        def __init__(self):
            self.k = 0

        def eval(self):
            pass

        def __call__(self, batch_dict, sync=True):
            assert sync is False
            bd = batches[self.k][0]
            self.k += 1
            batch_dict.update({k: v for k, v in bd.items() if k not in batch_dict})
            return model.post_processing(bd, sync=False)

    host_annos, gt_annos, want_recall, host_preds = [], [], {}, []
    for bd, gt in batches:
        with torch.no_grad():
            preds, recall, _ = model.post_processing(bd, sync=True)
        for k, v in recall.items():
            want_recall[k] = want_recall.get(k, 0) + v
        host_annos += kitti_eval.generate_prediction_dicts(bd, preds, cls)
        host_preds += [(bd, b, preds[b]) for b in range(bd["batch_size"])]
        for b in range(bd["batch_size"]):
            rows = gt[b][np.abs(gt[b]).sum(1) > 0]
            cam = kitti_eval.boxes3d_lidar_to_kitti_camera(rows[:, :7], bd["calib"][b])
            n = len(rows)
            gt_annos.append({"name": np.array([cls[int(c) - 1] for c in rows[:, 7]], dtype="<U16"), "truncated": np.zeros(n),
                             "occluded": np.zeros(n, np.int64), "alpha": (-np.arctan2(-rows[:, 1], rows[:, 0]) + cam[:, 6]).astype(np.float64),
                             "bbox": kitti_eval.boxes3d_kitti_camera_to_imageboxes(cam, bd["calib"][b], bd["image_shape"][b]).astype(np.float64).reshape(-1, 4),
                             "dimensions": cam[:, 3:6].astype(np.float64), "location": cam[:, 0:3].astype(np.float64),
                             "rotation_y": cam[:, 6].astype(np.float64)})
    feed = [{k: bd[k] for k in ("frame_id", "calib", "image_shape", "gt_boxes", "batch_size")} for bd, _ in batches]
    ep = eval_loop.DeviceEvalEpilogue(cls, thr, 3, eval_loop.post_max_of(cfg))
    with torch.no_grad():
        ret = eval_loop.eval_one_epoch_device(cfg, Model(), feed, gt_annos, epilogue=ep)
    total = want_recall["gt"]
    assert total > 0 and want_recall["rcnn_%s" % str(thr[0])] > 0 and ep.recall_dict() == want_recall
    for t in thr:
        assert ret["recall/rcnn_%s" % str(t)] == want_recall["rcnn_%s" % str(t)] / total
    annos = ep.det_annos()
    assert [len(a["name"]) for a in annos] == [len(a["name"]) for a in host_annos] and sum(len(a["name"]) for a in annos) > 20
    for f, (a, h) in enumerate(zip(annos, host_annos)):
        bd, b, pred = host_preds[f]
        boxes = pred["pred_boxes"].cpu().numpy()
        f64 = annos_f64(boxes, bd["calib"][b], bd["image_shape"][b])
        f64["score"] = pred["pred_scores"].cpu().numpy().astype(np.float64)
        assert a["frame_id"] == h["frame_id"] and list(a["name"]) == list(h["name"])
        assert a["score"].tobytes() == h["score"].tobytes() and a["dimensions"].tobytes() == np.asarray(h["dimensions"], np.float32).tobytes()
        for k in FIELDS:
            ref = np.asarray(h[k], np.float64)
            if k == "boxes_lidar":                                     # the bottom-centre z, as in test_gpu_eval_tail.py
                ref = ref.copy()
                ref[:, 2] = boxes[:, 2] - boxes[:, 5] / 2
            ref_err = float(np.abs(ref - f64[k]).max())
            dev_err = float(np.abs(a[k].astype(np.float64) - f64[k]).max())
            assert dev_err <= 4 * ref_err + 2.0 ** -23 * float(np.abs(f64[k]).max()), (f, k, dev_err, ref_err)
    text_h, ap_h = KD.get_official_eval_result(gt_annos, host_annos, cls)
    text, ap = ep.evaluate(gt_annos)
    assert sorted(ap) == sorted(ap_h) and len(ap) == 36 and max(ap.values()) > 0
    for k, v in ap_h.items():
        assert abs(ap[k] - v) < 1e-9 and ret[k] == ap[k], (k, ap[k], v)
    assert text.splitlines() == text_h.splitlines()
    # and the official host evaluator on the host formatter's annotations, at the bar test_gpu_kitti_ap.py holds the device evaluator to
    _, ap_host = kitti_eval.get_official_eval_result(gt_annos, host_annos, cls)
    for k, v in ap_host.items():
        assert abs(ap[k] - v) < 1e-9, (k, ap[k], v)


def test_more_rows_than_the_evaluator_holds_is_refused_on_the_host():
    """nc * NMS_POST_MAXSIZE > 4096 raises before anything touches a device (no GPU needed: the model is never called)."""
    from hvpr_amd.config import hvpr_3class_cfg
    cfg = hvpr_3class_cfg()
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS = True
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.NMS_POST_MAXSIZE = 1366          # 3 * 1366 = 4098
    assert eval_loop.post_max_of(cfg) == 4098
    with pytest.raises(ValueError, match="post_max"):
        eval_loop.eval_one_epoch_device(cfg, None, [], [])
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS = False
    assert eval_loop.post_max_of(cfg) == 1366
