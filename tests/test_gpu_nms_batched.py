"""GPU: batched rotated NMS (hvpr_nms_bev_batched_f32 / hvpr_gather_predictions_batched_f32) and the detector paths on it.

Every segment of a batched call is pinned, survivor for survivor, to the CPU oracle's O.nms_bev on that segment's live candidates
and to the single entry point on the same segment.  Boxes are clustered car boxes (many overlapping pairs), threshold 0.1."""
import numpy as np
import pytest
import torch

from hvpr_amd import kernels
from oracle import hvpr_oracle as O
from post_paths import car_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.1


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _ref(table, order_row, n, max_keep, thr=THR):
    """O.nms_bev on the live candidates of one segment (scores descending along the order) -> surviving rows of `table`."""
    live = np.arange(n) if order_row is None else np.asarray(order_row[:n], np.int64)
    if n == 0:
        return np.zeros((0,), np.int64)
    got = O.nms_bev(table[live], np.linspace(1.0, 0.1, n).astype(np.float32), thr)
    return live[got][:max_keep]


def _batched(tables, order, counts, n_max, max_keep, spt=1, mto=True, ws=None, thr=THR):
    S = tables.shape[0] * spt
    if ws is None:
        ws = torch.empty(kernels.lib().hvpr_nms_bev_batched_workspace_bytes(S, n_max), dtype=torch.uint8, device=DEV)
    keep, kc = kernels.nms_bev_batched(_t(tables), None if order is None else _t(order, torch.int32),
                                       None if counts is None else _t(np.asarray(counts, np.int32)), n_max, thr, max_keep, ws, mto, spt)
    assert keep.shape == (S, max_keep) and kc.shape == (S,) and keep.dtype == kc.dtype == torch.int32
    return keep.cpu().numpy(), kc.cpu().numpy()


def _single(table, order_row, count, n_max, max_keep, mto=True, thr=THR):
    ws = torch.empty(kernels.lib().hvpr_nms_workspace_bytes(n_max), dtype=torch.uint8, device=DEV)
    keep, kc = kernels.nms_bev(_t(table), None if order_row is None else _t(order_row, torch.int32),
                               None if count is None else _t(np.asarray([count], np.int32)), n_max, thr, max_keep, ws, mto)
    return keep.cpu().numpy()[: int(kc.item())]


def _check(tables, order, counts, n_max, max_keep, spt=1, **kw):
    """One batched call against the oracle and the single entry point, segment by segment.  Returns the survivor lists."""
    keep, kc = _batched(tables, order, counts, n_max, max_keep, spt, **kw)
    out = []
    for s in range(tables.shape[0] * spt):
        n = n_max if counts is None else counts[s]
        row = None if order is None else order[s]
        want = _ref(tables[s // spt], row, n, max_keep)
        assert kc[s] == len(want), f"segment {s}: count {kc[s]}, oracle {len(want)}"
        np.testing.assert_array_equal(keep[s, : kc[s]], want, err_msg=f"segment {s}")
        np.testing.assert_array_equal(_single(tables[s // spt], row, None if counts is None else n, n_max, max_keep), want,
                                      err_msg=f"segment {s}, single form")
        np.testing.assert_array_equal(keep[s, kc[s]:], 0, err_msg=f"segment {s}: rows past the count stay zero")
        out.append(want)
    return out


# ---------------------------------------------------------------------------------------------- 1, 5: ragged counts
RAGGED = [0, 1, 63, 64, 65, 128, 129, 200]


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(21)
    tables = np.stack([car_boxes(rng, 200) for _ in RAGGED])
    order = np.stack([rng.permutation(200) for _ in RAGGED]).astype(np.int32)
    return tables, order


def test_ragged_counts_in_one_call(ragged):
    """Empty, one lane, one box either side of a 64-block edge and of the second block, all in one call; then cut at max_keep = 5."""
    tables, order = ragged
    full = _check(tables, order, RAGGED, 200, 200)
    assert [len(w) for w in full[:2]] == [0, 1]
    assert any(len(w) > 5 for w in full) and any(0 < len(w) < 5 for w in full)
    cut = _check(tables, order, RAGGED, 200, 5)
    for w, c in zip(full, cut):
        np.testing.assert_array_equal(c, w[:5])


def test_segments_are_independent(ragged):
    """Permuting the segments permutes the outputs; one segment equals the single entry point."""
    tables, order = ragged
    keep, kc = _batched(tables, order, RAGGED, 200, 200)
    perm = np.random.default_rng(3).permutation(len(RAGGED))
    keep_p, kc_p = _batched(tables[perm], order[perm], [RAGGED[i] for i in perm], 200, 200)
    np.testing.assert_array_equal(kc_p, kc[perm])
    np.testing.assert_array_equal(keep_p, keep[perm])


@pytest.mark.parametrize("n", [1, 64, 65, 700])
def test_one_segment_equals_single_form(n):
    rng = np.random.default_rng(n)
    table = car_boxes(rng, n)
    order = rng.permutation(n).astype(np.int32)
    _check(table[None], order[None], [n], n, n)


# ---------------------------------------------------------------------------------------------- 2, 7: shared tables
POST = 55        # between the survivor counts of the six segments (48 .. 62): some are cut, some padded


@pytest.fixture(scope="module")
def shared_tables():
    """Two tables of 300 boxes, three score columns each -> six segments, orders and counts from ONE score_topk over the class-major
    scores; the columns are scaled so that SCORE_THRESH leaves a different count in each."""
    rng = np.random.default_rng(8)
    tables = np.stack([car_boxes(rng, 300), car_boxes(rng, 300)])
    scores = (rng.uniform(0, 1, (2, 300, 3)) * np.float32([1.0, 0.7, 0.45])).astype(np.float32)
    rows = np.ascontiguousarray(scores.transpose(0, 2, 1).reshape(6, 300))          # class-major: row t * 3 + k
    ws = kernels.PostWorkspace(6, 300, 300, DEV)
    assert ws.nms.numel() == kernels.lib().hvpr_nms_bev_batched_workspace_bytes(6, 300)
    order, _, counts = kernels.score_topk(_t(rows), 0.3, 300, ws, want_scores=False)
    keep, kc = kernels.nms_bev_batched(_t(tables), order, counts, 300, THR, POST, ws.nms, segments_per_table=3)
    return tables, scores, rows, order, counts, keep, kc


def test_shared_tables_from_one_score_topk(shared_tables):
    tables, scores, rows, order, counts, keep, kc = shared_tables
    cnt = counts.cpu().numpy()
    assert len(set(cnt.tolist())) == 6 and cnt.min() > 0 and cnt.max() < 300
    keep_h, kc_h, order_h = keep.cpu().numpy(), kc.cpu().numpy(), order.cpu().numpy()
    for t in range(2):
        _, lab, _, sel = O.multi_classes_nms(scores[t], tables[t], 0.3, THR, 300, POST)
        got = [keep_h[t * 3 + k, : kc_h[t * 3 + k]] for k in range(3)]
        np.testing.assert_array_equal(np.concatenate(got), sel)
        np.testing.assert_array_equal(np.concatenate([np.full(len(g), k) for k, g in enumerate(got)]), lab)
    for s in range(6):                                                             # six separate single calls
        np.testing.assert_array_equal(_single(tables[s // 3], order_h[s], cnt[s], 300, POST), keep_h[s, : kc_h[s]])
        np.testing.assert_array_equal(_ref(tables[s // 3], order_h[s], cnt[s], POST), keep_h[s, : kc_h[s]])


def test_gather_predictions_batched_row_for_row(shared_tables):
    """Against the single form on every segment, the padded rows past each count included (keep is zero there: row 0)."""
    tables, _, rows, _, _, keep, kc = shared_tables
    assert int(kc.min()) < POST == int(kc.max())                                  # padded rows in some segments, a cut in others
    labels = torch.arange(6 * 300, dtype=torch.int32, device=DEV).reshape(6, 300) % 7 + 1
    tb, tr = _t(tables), _t(rows)
    pb, ps, pl, sel = kernels.gather_predictions_batched(tb, tr, labels, keep, segments_per_table=3)
    assert pb.shape == (6, POST, 7) and ps.shape == pl.shape == sel.shape == (6, POST) and pl.dtype == sel.dtype == torch.int64
    for s in range(6):
        b1, s1, l1, e1 = kernels.gather_predictions(tb[s // 3], tr[s], labels[s].contiguous(), keep[s].contiguous())
        for got, want in ((pb[s], b1), (ps[s], s1), (pl[s], l1), (sel[s], e1)):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"segment {s}")
        np.testing.assert_array_equal(sel[s].cpu().numpy(), keep[s].cpu().numpy())


# ---------------------------------------------------------------------------------------------- 3: the optional arguments
def test_no_order_no_counts_positions_out():
    rng = np.random.default_rng(5)
    tables = np.stack([car_boxes(rng, 130) for _ in range(3)])
    got = _check(tables, None, None, 130, 130, mto=False)
    for t in range(3):
        np.testing.assert_array_equal(got[t], O.nms_sorted(tables[t], THR))
    # with an order but map_through_order = 0, keep holds positions in the order, not rows of the table
    order = np.stack([rng.permutation(130) for _ in range(3)]).astype(np.int32)
    keep, kc = _batched(tables, order, None, 130, 130, mto=False)
    for t in range(3):
        np.testing.assert_array_equal(keep[t, : kc[t]], O.nms_sorted(tables[t][order[t]], THR))


# ---------------------------------------------------------------------------------------------- 4: workspace reuse
def test_workspace_reuse_leaves_nothing_behind():
    """Call A fills every part of a 4 x 700 workspace (mask, pair counts, ClipIndex, prepared boxes); call B, on other boxes with
    fewer candidates, must not see any of it."""
    rng = np.random.default_rng(13)
    ws = torch.empty(kernels.lib().hvpr_nms_bev_batched_workspace_bytes(4, 700), dtype=torch.uint8, device=DEV)
    ta = np.stack([car_boxes(rng, 700, spread=10.0) for _ in range(4)])           # dense: many suppression bits
    oa = np.stack([rng.permutation(700) for _ in range(4)]).astype(np.int32)
    _batched(ta, oa, [700] * 4, 700, 700, ws=ws)
    tb = np.stack([car_boxes(rng, 700) for _ in range(4)])
    ob = np.stack([rng.permutation(700) for _ in range(4)]).astype(np.int32)
    _check(tb, ob, [3, 0, 65, 700], 700, 700, ws=ws)
    _check(tb[:2], np.argsort(ob[:2, :130], axis=1).astype(np.int32), [130, 64], 130, 130, ws=ws)         # fewer, shorter segments on the same workspace


# ---------------------------------------------------------------------------------------------- 6: both size classes
@pytest.mark.parametrize("n_max,counts", [(4096, [4096, 4033, 0]), (4160, [4160, 70])])
def test_size_classes_at_their_edges(n_max, counts):
    """4096: the two-launch mask and the ring sweep with all 64 words, 63 blocks plus one box, and an empty segment.  4160: nb = 65,
    the one-launch mask and the one-wave sweep.  The segments rank one table in different orders."""
    rng = np.random.default_rng(n_max)
    table = car_boxes(rng, n_max)
    S = len(counts)
    order = np.stack([rng.permutation(n_max) for _ in range(S)]).astype(np.int32)
    keep, kc = _batched(table[None], order, counts, n_max, n_max, spt=S)
    for s in range(S):
        want = _ref(table, order[s], counts[s], n_max)
        assert kc[s] == len(want)
        np.testing.assert_array_equal(keep[s, : kc[s]], want, err_msg=f"segment {s}")
    s = 1                                                                          # the single form on the ragged segment
    np.testing.assert_array_equal(_single(table, order[s], counts[s], n_max, n_max), keep[s, : kc[s]])


# ---------------------------------------------------------------------------------------------- 8, 9: detector
class _Cfg:
    raw, nms_thresh, pre, post = False, THR, 512, 50


def _head(seed, B, num_class, A=2000):
    """B frames of A anchors: logits (B, A, num_class), boxes (B, A, 7), gt (B, 8, 8); frame 1 has nothing above SCORE_THRESH."""
    rng = np.random.default_rng(seed)
    boxes = np.stack([car_boxes(rng, A) for _ in range(B)])
    logits = rng.normal(-2.0, 2.0, (B, A, num_class)).astype(np.float32)
    logits[1] = np.minimum(logits[1], -2.5)                                       # sigmoid < 0.076 < SCORE_THRESH
    gt = np.zeros((B, 8, 8), np.float32)
    for b in range(B):
        ids = rng.choice(A, 6, replace=False)
        gt[b, :6, :7] = boxes[b, ids] + np.float32([0.2, -0.1, 0.05, 0.1, 0.05, 0.0, 0.03])
        gt[b, :6, 7] = 1.0
    return logits, boxes, gt


def _detector(multi, num_class):
    from test_gpu_post import _g15_detector

    class C(_Cfg):
        pass
    C.multi, C.num_class = multi, num_class
    return _g15_detector(C)[0]


def _oracle(logits, boxes, gt, multi):
    import g15_cases
    norm = torch.sigmoid(_t(logits)).cpu().numpy()
    return O.post_processing(norm, boxes, gt, g15_cases.SCORE_THRESH, _Cfg.nms_thresh, _Cfg.pre, _Cfg.post, g15_cases.RECALL_THRESH_LIST,
                             normalized=True, multi_classes=multi)


def _bd(logits, boxes, gt):
    return {"batch_size": logits.shape[0], "batch_cls_preds": _t(logits), "batch_box_preds": _t(boxes), "cls_preds_normalized": False,
            "gt_boxes": _t(gt)}


class _Calls:
    """Counting wrappers on kernels.nms_bev, kernels.nms_bev_batched and kernels.PostWorkspace."""

    def __init__(self, monkeypatch):
        self.n = {"nms_bev": 0, "nms_bev_batched": 0, "PostWorkspace": 0}
        for name in self.n:
            monkeypatch.setattr(kernels, name, self._wrap(name, getattr(kernels, name)))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return counted

    def take(self):
        out = dict(self.n)
        for k in self.n:
            self.n[k] = 0
        return out


def _same_records(got, want, keys):
    assert len(got) == len(want)
    for b, (p, w) in enumerate(zip(got, want)):
        for k in keys:
            a = p[k].cpu().numpy() if torch.is_tensor(p[k]) else p[k]
            c = w[k].cpu().numpy() if torch.is_tensor(w[k]) else w[k]
            np.testing.assert_array_equal(a, c, err_msg=f"frame {b} {k}")


def test_detector_class_agnostic_one_batched_call(monkeypatch):
    calls = _Calls(monkeypatch)
    logits, boxes, gt = _head(31, 3, 1)
    want, want_recall = _oracle(logits, boxes, gt, False)
    assert len(want[1]["selected"]) == 0 and len(want[0]["selected"]) > 0 and len(want[2]["selected"]) > 0
    det = _detector(False, 1)
    bd = _bd(logits, boxes, gt)
    det.post_processing(dict(bd))                                                  # first batch: builds the workspace
    assert calls.take()["PostWorkspace"] == 1
    preds, recall, _ = det.post_processing(dict(bd))
    assert calls.take() == {"nms_bev": 0, "nms_bev_batched": 1, "PostWorkspace": 0}
    assert recall == want_recall
    _same_records(preds, want, ("pred_boxes", "pred_scores", "pred_labels", "selected"))
    for p, w in zip(preds, want):
        assert p["pred_count"].shape == (1,) and int(p["pred_count"].item()) == len(w["selected"])
    padded, recall, _ = det.post_processing(dict(bd), sync=False)
    assert calls.take() == {"nms_bev": 0, "nms_bev_batched": 1, "PostWorkspace": 0}
    assert recall == {}
    for b, (p, w) in enumerate(zip(padded, want)):
        n = int(p["pred_count"].item())
        assert n == len(w["selected"]) and p["pred_count"].shape == (1,)
        assert all(p[k].shape[0] == _Cfg.post for k in ("pred_boxes", "pred_scores", "pred_labels", "selected"))
        _same_records([{k: p[k][:n] for k in w}], [w], ("pred_boxes", "pred_scores", "pred_labels", "selected"))
    # chunk boundary: two segments per call -> frames {0, 1} and {2}; the records do not change
    monkeypatch.setattr(kernels, "MAX_NMS_SEGMENTS", 2)
    chunked, recall, _ = det.post_processing(dict(bd))
    assert calls.take() == {"nms_bev": 0, "nms_bev_batched": 2, "PostWorkspace": 0}
    assert recall == want_recall
    _same_records(chunked, preds, ("pred_boxes", "pred_scores", "pred_labels", "selected", "pred_count"))


def test_detector_multi_class_one_batched_call(monkeypatch):
    calls = _Calls(monkeypatch)
    logits, boxes, gt = _head(32, 2, 3)
    want, want_recall = _oracle(logits, boxes, gt, True)
    assert len(want[1]["pred_scores"]) == 0 and len(set(want[0]["pred_labels"].tolist())) == 3
    det = _detector(True, 3)
    bd = _bd(logits, boxes, gt)
    det.post_processing(dict(bd))
    assert calls.take()["PostWorkspace"] == 1
    preds, recall, _ = det.post_processing(dict(bd))
    assert calls.take() == {"nms_bev": 0, "nms_bev_batched": 1, "PostWorkspace": 0}
    assert recall == want_recall
    _same_records(preds, want, ("pred_boxes", "pred_scores", "pred_labels"))
    assert preds[0]["pred_labels"].dtype == torch.int64
    # chunks of whole frames (3 of 4 allowed segments), then fewer segments per call than a frame has classes
    for cap, n_calls in ((4, 2), (2, 4)):
        monkeypatch.setattr(kernels, "MAX_NMS_SEGMENTS", cap)
        chunked, recall, _ = det.post_processing(dict(bd))
        assert calls.take() == {"nms_bev": 0, "nms_bev_batched": n_calls, "PostWorkspace": 0}
        assert recall == want_recall
        _same_records(chunked, preds, ("pred_boxes", "pred_scores", "pred_labels"))


def test_module_level_multi_classes_nms_is_one_call(monkeypatch):
    from hvpr_amd import detector
    from hvpr_amd.config import AttrDict
    calls = _Calls(monkeypatch)
    rng = np.random.default_rng(4)
    boxes = car_boxes(rng, 600)
    cls = rng.uniform(0, 1, (600, 3)).astype(np.float32)
    ncfg = AttrDict(NMS_TYPE="nms_gpu", NMS_THRESH=0.2, NMS_PRE_MAXSIZE=300, NMS_POST_MAXSIZE=40, MULTI_CLASSES_NMS=True)
    sc, lab, bx = detector.multi_classes_nms(_t(cls), _t(boxes), ncfg, score_thresh=0.3)
    assert calls.take() == {"nms_bev": 0, "nms_bev_batched": 1, "PostWorkspace": 1}
    ws_, wl, wb, _ = O.multi_classes_nms(cls, boxes, 0.3, 0.2, 300, 40)
    np.testing.assert_array_equal(sc.cpu().numpy(), ws_)
    np.testing.assert_array_equal(lab.cpu().numpy(), wl)
    np.testing.assert_array_equal(bx.cpu().numpy(), wb)


def test_post_processing_replays_in_a_graph():
    """post_processing(sync=False) of B = 2 captured on one stream (no side branches); new scores and boxes are copied into the
    captured inputs and the replay equals the eager result on them."""
    det = _detector(False, 1)
    l0, b0, _ = _head(41, 2, 1)
    l1, b1, _ = _head(42, 2, 1)
    l1[1] = l0[0]                                                                  # frame 1 of the replay has detections
    static = {"batch_size": 2, "batch_cls_preds": _t(l0), "batch_box_preds": _t(b0), "cls_preds_normalized": False}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        det.post_processing(dict(static), sync=False)                              # eager warm-up: workspace, dynamic-LDS attribute
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = det.post_processing(dict(static), sync=False)[0]
    static["batch_cls_preds"].copy_(_t(l1))
    static["batch_box_preds"].copy_(_t(b1))
    graph.replay()
    torch.cuda.synchronize()
    got = [{k: v.clone() for k, v in rec.items()} for rec in out]
    with torch.no_grad():
        want = det.post_processing({"batch_size": 2, "batch_cls_preds": _t(l1), "batch_box_preds": _t(b1), "cls_preds_normalized": False},
                                   sync=False)[0]
    assert sum(int(w["pred_count"].item()) for w in want) > 0
    for b, (g, w) in enumerate(zip(got, want)):
        n = int(w["pred_count"].item())
        assert int(g["pred_count"].item()) == n
        _same_records([{k: v[:n] for k, v in g.items() if k != "pred_count"}], [{k: v[:n] for k, v in w.items() if k != "pred_count"}],
                      ("pred_boxes", "pred_scores", "pred_labels", "selected"))
