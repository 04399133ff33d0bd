"""GPU: every size-selected path of row a8 against the oracle, exactly — score top-k on its compact / rank / radix paths (the host
model in tests/post_paths.py asserts which path each frame takes), rotated NMS on the n_max > 4096 path (k_nms_mask +
k_nms_sweep) and against the two-launch + ring path, and batched post-processing at the dense-grid anchor count."""
import numpy as np
import pytest
import torch

import post_paths as P
from hvpr_amd import kernels
from oracle import hvpr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------- score top-k
def _check_topk(s, thresh, pre, ws, paths=None):
    """One score_topk call on the frames s (B, A) against the oracle's order; `paths` = the path each frame must take."""
    s = np.atleast_2d(s)
    if paths is not None:
        assert [P.topk_candidates(f, thresh, pre)[1] for f in s] == list(paths)
    order, ss, counts = kernels.score_topk(torch.from_numpy(s).to(DEV), thresh, pre, ws)
    order, ss, counts = order.cpu().numpy(), ss.cpu().numpy(), counts.cpu().numpy()
    for b, f in enumerate(s):
        passing = np.nonzero(P.passing_mask(f, thresh))[0]
        ref = passing[O.stable_order_desc(f[passing])][:pre]
        msg = f"frame {b}, pre_max {pre}, thresh {thresh}"
        assert counts[b] == len(ref), msg
        np.testing.assert_array_equal(order[b, : counts[b]], ref, err_msg=msg)
        # sorted scores bit for bit; -0.0 comes back as +0.0
        np.testing.assert_array_equal(ss[b, : counts[b]].view(np.uint32), (f[ref] + np.float32(0)).view(np.uint32), err_msg=msg)
    return counts


@pytest.mark.parametrize("case", P.SCORE_CASES, ids=[c[0] for c in P.SCORE_CASES])
def test_score_topk_paths_exact(case):
    """Radix path at A = 146 816 and 524 288 (all equal, 20 000 exact 1.0f, one over-full bin; with and without a threshold) at
    every pre_max of PRE_MAXES; n_scores 8192 / 8193 (compact against histogram); 8192 / 8193 candidates after the pre-filter
    (rank against radix); NaN, +-inf, negative scores and mixed +-0.0 ties."""
    _, make, thresh, pres, path = case
    s = make()
    ws = kernels.PostWorkspace(1, s.size, max(pres), DEV)
    for pre in pres:
        _check_topk(s, thresh, pre, ws, [path])


def test_score_topk_signed_zero_ties_small():
    s = np.float32([-0.0, 0.0, -0.0, 0.0])
    ws = kernels.PostWorkspace(1, 4, 4, DEV)
    _check_topk(s, None, 4, ws, ["compact"])
    _check_topk(s, 0.0, 4, ws, ["compact"])
    s = P.scores_special(2000, 4, n_zero=300, n_nan=100, n_inf=20)
    _check_topk(s, None, 1000, kernels.PostWorkspace(1, 2000, 1000, DEV), ["compact"])


@pytest.mark.parametrize("A", [P.A_CAR, 8193])
def test_score_topk_nothing_or_few_pass(A):
    rng = np.random.default_rng(A)
    s = rng.uniform(0, 1, A).astype(np.float32)
    ws = kernels.PostWorkspace(1, A, 4096, DEV)
    assert _check_topk(s, 2.0, 4096, ws, ["rank"])[0] == 0
    few = np.sort(s)[-100]                               # 100 pass, pre_max 4096: cut bin 0, every passing score a candidate
    assert P.cut_bin(s, few, 4096) == 0
    assert _check_topk(s, few, 4096, ws, ["rank"])[0] == 100
    s[rng.choice(A, 50, replace=False)] = np.nan          # NaN: no candidate, not counted
    assert _check_topk(s, None, 4096, ws)[0] == 4096


@pytest.mark.parametrize("A", [P.A_CAR, P.A_GRID])
def test_score_topk_mixed_batch(A):
    """One launch, B = 4: radix, rank, nothing passes, fewer than pre_max pass — k_rank_* and k_topk_select decide per frame."""
    s = P.mixed_batch(A, 5)
    ws = kernels.PostWorkspace(4, A, 4096, DEV)
    counts = _check_topk(s, 0.3, 4096, ws, ["radix", "rank", "rank", "rank"])
    np.testing.assert_array_equal(counts, [4096, 4096, 0, 200])
    _check_topk(s[[3, 0, 2, 1]].copy(), 0.3, 4096, ws, ["rank", "radix", "rank", "rank"])


def test_score_topk_workspace_reuse_across_paths():
    """One PostWorkspace through radix -> rank -> compact -> radix -> compact -> rank: every call must find the counters,
    histogram and rank array at zero, whatever n_scores the previous call had."""
    ws = kernels.PostWorkspace(2, P.A_GRID, 8192, DEV)
    rng = np.random.default_rng(9)
    seq = [(np.stack([P.scores_equal(P.A_GRID), P.scores_saturated(P.A_GRID, 1)]), None, 8192, ["radix", "radix"]),
           (rng.uniform(0, 1, (2, P.A_CAR)).astype(np.float32), 0.2, 4096, ["rank", "rank"]),
           (rng.uniform(0, 1, (2, 5000)).astype(np.float32), 0.5, 3000, ["compact", "compact"]),
           (np.stack([P.scores_cluster(P.A_CAR, 3), P.scores_saturated(P.A_CAR, 4)]), 0.25, 500, ["radix", "radix"]),
           (rng.uniform(0, 1, (2, 8192)).astype(np.float32), None, 8192, ["compact", "compact"]),
           (rng.uniform(0, 1, (2, P.A_GRID)).astype(np.float32), None, 4095, ["rank", "rank"]),
           (np.stack([P.scores_equal(P.A_CAR), P.scores_special(P.A_CAR)]), None, 4096, ["radix", "rank"])]
    for s, thresh, pre, paths in seq:
        _check_topk(s, thresh, pre, ws, paths)
    with pytest.raises(ValueError):
        kernels.score_topk(torch.zeros((1, 100), device=DEV), None, 10, ws)


# ---------------------------------------------------------------------------------------------- rotated NMS
def _nms(boxes, order, live, n_max, thresh, max_keep, map_through_order):
    """kernels.nms_bev with the live count on the device; order padded to n_max (the ring sweep reads it that far)."""
    o = np.zeros(n_max, np.int32)
    o[: len(order)] = order
    ws = kernels.PostWorkspace(1, 1, n_max, DEV).nms
    keep, kc = kernels.nms_bev(torch.from_numpy(boxes).to(DEV), torch.from_numpy(o).to(DEV),
                               torch.tensor([live], dtype=torch.int32, device=DEV), n_max, thresh, max_keep, ws, map_through_order)
    return keep.cpu().numpy()[: int(kc.item())]


def _nms_ref(boxes, order, live, thresh, max_keep, map_through_order):
    pos = O.nms_sorted(boxes[order[:live]], thresh)[:max_keep] if live else np.zeros(0, np.int64)
    return order[pos] if map_through_order else pos


@pytest.mark.parametrize("n", [4097, 6000, 8192, 16384])
def test_nms_large_path_against_oracle(n):
    """k_nms_mask + k_nms_sweep at the n of the box density of test_nms_survivors_bit_exact; survivors and suppressed boxes at
    sorted positions >= 4096 (past the 64 prefetched diagonal blocks, in remv words 1..3)."""
    rng = np.random.default_rng(n)
    boxes = P.car_boxes(rng, n, spread=40.0 * n / 4096)
    scores = rng.uniform(0.1, 1, n).astype(np.float32)
    order = O.stable_order_desc(scores).astype(np.int32)
    late_kept = late_gone = 0
    for thr in (0.0, 0.1, 0.5, 0.7):
        ref = O.nms_sorted(boxes[order], thr)
        got = _nms(boxes, order, n, n, thr, n, False)
        np.testing.assert_array_equal(got, ref, err_msg=f"n {n} thresh {thr}")
        np.testing.assert_array_equal(_nms(boxes, order, n, n, thr, n, True), order[ref], err_msg=f"n {n} thresh {thr}")
        kept = int((ref >= 4096).sum())
        late_kept += kept
        late_gone += n - 4096 - kept
        if n > 4097:
            assert kept > 0 and n - 4096 - kept > 0, thr
    assert late_kept > 0 and late_gone > 0


@pytest.mark.parametrize("map_through_order", [False, True])
def test_nms_paths_agree_on_the_same_candidates(map_through_order):
    """The same 4096 live candidates with n_max 4096 (k_nms_pairs/scan/clip + ring sweep) and n_max 4160 / 16384 (k_nms_mask +
    k_nms_sweep): identical keep lists and counts, equal to the oracle."""
    rng = np.random.default_rng(21)
    boxes = P.car_boxes(rng, 5000)
    scores = rng.uniform(0, 1, 5000).astype(np.float32)
    order = O.stable_order_desc(scores).astype(np.int32)[:4096]
    for thr in (0.1, 0.5):
        want = _nms_ref(boxes, order, 4096, thr, 4096, map_through_order)
        for n_max in (4096, 4160, 16384):
            np.testing.assert_array_equal(_nms(boxes, order, 4096, n_max, thr, 4096, map_through_order), want,
                                          err_msg=f"n_max {n_max} thresh {thr}")


def _grid_boxes(rng, spacing):
    """Axis-aligned 4 x 2 m boxes on a 64 x 64 grid `spacing` apart (x: 4 * spacing, y: 2 * spacing); spacing 1 = touching edges
    and corners.  Every seventh box gets a copy shifted by (1, 0.5) m that overlaps it."""
    gx, gy = np.meshgrid(np.arange(64) * 4.0 * spacing, np.arange(64) * 2.0 * spacing)
    b = np.zeros((4096, 7), np.float32)
    b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4], b[:, 5] = gx.ravel(), gy.ravel(), -1.0, 4.0, 2.0, 1.5
    extra = b[::7].copy()
    extra[:, 0] += 1.0
    extra[:, 1] += 0.5
    b = np.concatenate([b, extra])
    return b[rng.permutation(len(b))]


def _duplicate_boxes(rng, n):
    """n // 2 clustered car boxes and an exact copy of each (shuffled), the copy with the same score: tied scores, IoU 1."""
    base = P.car_boxes(rng, n // 2)
    sc = rng.uniform(0, 1, n // 2).astype(np.float32)
    perm = rng.permutation(n // 2)
    return np.concatenate([base, base[perm]]), np.concatenate([sc, sc[perm]])


@pytest.mark.parametrize("n_max", [4096, 8192])
def test_nms_edges_on_both_paths(n_max):
    """On the ring path (n_max 4096) and the mask path (8192): live count 0, 1, 64, 65, n_max; max_keep 1, 83, 500; exact
    duplicates with tied scores; touching and far-apart boxes."""
    rng = np.random.default_rng(n_max)
    boxes = P.car_boxes(rng, n_max, spread=40.0 * n_max / 4096)
    scores = rng.uniform(0, 1, n_max).astype(np.float32)
    order = O.stable_order_desc(scores).astype(np.int32)
    for live in (0, 1, 64, 65, n_max):
        for max_keep in (1, 83, 500, n_max):
            for mto in (False, True):
                np.testing.assert_array_equal(_nms(boxes, order, live, n_max, 0.1, max_keep, mto),
                                              _nms_ref(boxes, order, live, 0.1, max_keep, mto),
                                              err_msg=f"live {live} max_keep {max_keep} map {mto}")
    cases = [("duplicates",) + _duplicate_boxes(rng, n_max)]
    for name, spacing in (("touching", 1.0), ("far", 25.0)):
        b = _grid_boxes(rng, spacing)[:n_max]
        cases.append((name, b, rng.uniform(0, 1, len(b)).astype(np.float32)))
    for name, b, s in cases:
        order = O.stable_order_desc(s).astype(np.int32)
        n = len(b)
        for thr in (0.0, 0.1, 0.7):
            want = _nms_ref(b, order, n, thr, n, True)
            np.testing.assert_array_equal(_nms(b, order, n, n_max, thr, n, True), want, err_msg=f"{name} thresh {thr}")
            if name == "duplicates":          # every copy goes: IoU ~1 with its twin
                assert len(want) <= n // 2
            elif thr == 0.7:                   # grid neighbours touch or are far apart, the shifted copies have IoU 0.39
                assert len(want) == n


def test_nms_gpu_wrapper_at_8192():
    """iou3d_nms_utils.nms_gpu at its 8192-candidate limit, with and without pre_maxsize (4096: ring path, 5000 and none: mask
    path), equals O.nms_bev on the same candidates; 8193 raises."""
    from hvpr_amd import iou3d_nms_utils
    rng = np.random.default_rng(8192)
    boxes = P.car_boxes(rng, 8192, spread=80.0)
    scores = rng.uniform(0, 1, 8192).astype(np.float32)
    tb, ts = torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV)
    order = O.stable_order_desc(scores)
    for thr in (0.1, 0.5):
        keep, none = iou3d_nms_utils.nms_gpu(tb, ts, thr)
        assert none is None
        np.testing.assert_array_equal(keep.cpu().numpy(), O.nms_bev(boxes, scores, thr))
        for pre in (4096, 5000):
            keep, _ = iou3d_nms_utils.nms_gpu(tb, ts, thr, pre_maxsize=pre)
            np.testing.assert_array_equal(keep.cpu().numpy(), order[:pre][O.nms_sorted(boxes[order[:pre]], thr)])
    with pytest.raises(ValueError):
        iou3d_nms_utils.nms_gpu(torch.zeros((8193, 7), device=DEV), torch.zeros(8193, device=DEV), 0.1)


# ---------------------------------------------------------------------------------------------- batched post-processing
def _dense_head(seed, num_class):
    """B = 4 frames of A = 524 288 anchors (a 512 x 512 grid, headings 0 and pi/2): logits (4, A, num_class), decoded boxes
    (4, A, 7), gt boxes (4, 16, 8).  Frame 0: 20 000 anchors saturate (class 0 logit 20 -> sigmoid exactly 1.0f): the radix path.
    Frame 1: nothing above SCORE_THRESH.  Frames 2 and 3: ordinary."""
    rng = np.random.default_rng(seed)
    A = P.A_GRID
    gx, gy = np.meshgrid((np.arange(512) + 0.5) * 70.4 / 512, (np.arange(512) + 0.5) * 80.0 / 512 - 40.0)
    boxes = np.zeros((4, A, 7), np.float32)
    for b in range(4):
        boxes[b, :, 0] = np.repeat(gx.ravel(), 2) + rng.normal(0, 0.1, A)
        boxes[b, :, 1] = np.repeat(gy.ravel(), 2) + rng.normal(0, 0.1, A)
        boxes[b, :, 2] = rng.normal(-1.0, 0.2, A)
        boxes[b, :, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (A, 3))
        boxes[b, :, 6] = np.tile([0.0, np.pi / 2], A // 2) + rng.normal(0, 0.1, A)
    logits = rng.normal(-4.0, 2.0, (4, A, num_class)).astype(np.float32)
    hot = rng.choice(A, 20000, replace=False)
    logits[0, hot] = -20.0
    logits[0, hot, 0] = 20.0
    logits[1] = np.minimum(logits[1], -2.5)              # sigmoid < 0.076
    gt = np.zeros((4, 16, 8), np.float32)
    for b in (0, 2, 3):
        ids = rng.choice(A, 12, replace=False)
        gt[b, :12, :7] = boxes[b, ids] + np.float32([0.3, -0.2, 0.05, 0.1, 0.05, 0.0, 0.05])
        gt[b, :12, 7] = 1.0
    return logits, boxes, gt


@pytest.mark.parametrize("multi", [False, True])
def test_post_processing_dense_grid_batch(multi):
    """Detector3DTemplate.post_processing on B = 4 frames of 524 288 anchors against O.post_processing: boxes, scores, labels,
    selected ids, pred_count and the recall counters exact.  The oracle gets the device's sigmoid (normalised scores), so both sides
    rank the same fp32 values; anchors whose class maximum is tied get their other classes pushed down (torch's arg-max tie
    rule is not the subject here)."""
    import g15_cases
    from test_gpu_post import _g15_detector

    class C:
        raw, nms_thresh, pre, post = False, 0.1, 4096, 500
    C.multi, C.num_class = multi, 3 if multi else 1
    logits, boxes, gt = _dense_head(17, C.num_class)
    tl = torch.from_numpy(logits).to(DEV)
    norm = torch.sigmoid(tl).cpu().numpy()
    tied = (norm == norm.max(-1, keepdims=True)).sum(-1) > 1
    if tied.any():
        logits[..., 1:][tied] = -20.0
        tl = torch.from_numpy(logits).to(DEV)
        norm = torch.sigmoid(tl).cpu().numpy()
    # the scores each top-k call ranks: the class maximum (class-agnostic), or every class column (one call per class)
    ranked = [[norm[b, :, k] for k in range(C.num_class)] if multi else [norm[b].max(-1)] for b in range(4)]
    paths = [[P.topk_candidates(s, g15_cases.SCORE_THRESH, 4096) for s in frame] for frame in ranked]
    assert (norm[0, :, 0] == 1.0).sum() == 20000
    assert [p for _, p in paths[0]] == ["radix"] + ["rank"] * (len(paths[0]) - 1)
    assert all(c == 0 for c, _ in paths[1])
    assert all(p == "rank" and c > 0 for b in (2, 3) for c, p in paths[b])
    det, cfg, _ = _g15_detector(C)
    bd = {"batch_size": 4, "batch_cls_preds": tl, "batch_box_preds": torch.from_numpy(boxes).to(DEV), "cls_preds_normalized": False,
          "gt_boxes": torch.from_numpy(gt).to(DEV)}
    preds, recall, _ = det.post_processing(dict(bd))
    want, want_recall = O.post_processing(norm, boxes, gt, g15_cases.SCORE_THRESH, C.nms_thresh, C.pre, C.post,
                                          g15_cases.RECALL_THRESH_LIST, normalized=True, multi_classes=multi)
    assert recall == want_recall
    for b, (p, w) in enumerate(zip(preds, want)):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            np.testing.assert_array_equal(p[k].cpu().numpy(), w[k], err_msg=f"frame {b} {k}")
        if not multi:
            np.testing.assert_array_equal(p["selected"].cpu().numpy(), w["selected"], err_msg=f"frame {b}")
            assert int(p["pred_count"].item()) == len(w["selected"])
    assert len(want[1]["selected"]) == 0 and len(want[0]["selected"]) > 0
    if not multi:                        # the no-read-back form: padded rows and a device count
        preds, _, _ = det.post_processing(dict(bd), sync=False)
        for b, (p, w) in enumerate(zip(preds, want)):
            n = int(p["pred_count"].item())
            assert n == len(w["selected"])
            np.testing.assert_array_equal(p["selected"][:n].cpu().numpy(), w["selected"])
            np.testing.assert_array_equal(p["pred_boxes"][:n].cpu().numpy(), w["pred_boxes"])
