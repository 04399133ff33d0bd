"""Shared bodies of the ATSS target-assigner checks (tests/test_atss_host.py on the CPU, tests/test_gpu_atss.py on the device): a
numpy host form of hvpr_assign_targets_atss_f32 over ANY (anchors, ground truths) -> IoU table, the frames fixture G27 adds to
G18's and G26's, and the fixture's reader.  The host form states the semantics include/hvpr_amd.h declares for it: the reference's
ATSSTargetAssigner (atss_target_assigner.py:16-141) with the product's own tie rules — the 64-bit key (bits of the fp32 squared
centre distance, then anchor index) for the TOPK nearest, the first maximum over the ground truths, the last write of the forced
matches — and float64 statistics summed in key order.  G27 (tests/golden/make_golden_atss.py) pins it to the reference's own
class wherever the reference's outcome does not hang on an unspecified tie.

Beside its outputs the host form returns the smallest margins it met, so that a caller can tell an input whose outcome hangs on
rounding from a wrong kernel:
  (i)   `nearest`: k-th against (k+1)-th squared distance of a ground truth, relative, where they DIFFER; keys that tie exactly are
        ordered by the anchor index on the device as here (the same fp32 operations give the same bits) and are counted in `ties`
        instead — torch.topk decides them differently, so against the reference a tie at the cut leaves a frame UNPINNED;
  (ii)  `thresh`: |iou - thresh| over the candidates; a ground truth whose candidates all have IoU exactly 0 is left out: mean and
        std are exactly 0 in every arithmetic and summation order, the threshold is exactly 1e-6 and nothing reaches it;
  (iii) `inside`: the distance in metres of a candidate that passes the IoU test from the nearest face of the inside test; a centre
        exactly on a face (distance 0, inside) is counted in `on_face`, not in the margin;
  (iv)  `maxima`: where a maximum is taken over IoUs — an anchor's positive ground truths, a ground truth's anchors — the gap
        between the values compared where they differ (equal bits, as of identical rows, are decided by the index).  It says
        whether an outcome survives a table that differs in the last bits, as the CPU oracle's does from the device's (their sin
        and cos differ); over ONE table, as in the GPU tests, the maxima are exact and it plays no part."""
import os

import numpy as np

from assign3d_cases import F32, encode, head_index  # noqa: F401  (head_index: for the callers)

INF = float("inf")


def trim_rows(gt):
    """Rows that stay: trailing rows whose signed fp32 sum over the 7 box fields is 0 are cut, row 0 never is (:40-46)."""
    if gt.shape[0] == 0:
        return 0
    s = np.zeros(gt.shape[0], F32)
    for j in range(7):
        s = (s + gt[:, j]).astype(F32)
    nz = np.nonzero(s != 0)[0]
    return (int(nz.max()) if len(nz) else 0) + 1


def distance_keys(anchors, box):
    """(keys (N,) uint64, squared distances (N,) fp32) of one ground truth: (dx*dx + dy*dy) + dz*dz in fp32, then the anchor index."""
    dx, dy, dz = (anchors[:, j].astype(F32) - F32(box[j]) for j in range(3))
    d = ((dx * dx + dy * dy).astype(F32) + dz * dz).astype(F32)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(d), dtype=np.uint64), d


def new_margins():
    return dict(nearest=INF, thresh=INF, inside=INF, maxima=INF, ties=0, on_face=0)


def merge_margins(a, b):
    return dict(nearest=min(a["nearest"], b["nearest"]), thresh=min(a["thresh"], b["thresh"]), inside=min(a["inside"], b["inside"]),
                maxima=min(a["maxima"], b["maxima"]), ties=a["ties"] + b["ties"], on_face=a["on_face"] + b["on_face"])


def host_atss_set(anchors, gt, n_classes, topk, iou):
    """One frame, one anchor set, the set's own anchor order: labels (N,) int32, targets (N, 7) fp32, weights (N,) fp32, margins.
    iou(anchors (N, 7), boxes (M, 7)) -> (N, M) fp32."""
    anchors = np.ascontiguousarray(anchors, F32)
    N, k = anchors.shape[0], int(topk)
    assert 1 <= k <= min(N, 64)
    match = np.full(N, -1, np.int64)
    mg = new_margins()
    n = trim_rows(gt)
    if n:
        gt = np.ascontiguousarray(gt[:n], F32)
        table = np.asarray(iou(anchors[:, :7], gt[:, :7]), F32)
        assert table.shape == (N, n)
        best = np.full(N, -INF)
        for g in range(n):
            keys, d = distance_keys(anchors, gt[g])
            order = np.argsort(keys, kind="stable")
            cand = order[:k]
            if k < N:
                dk, dn = float(d[order[k - 1]]), float(d[order[k]])
                if dk == dn:
                    mg["ties"] += 1
                else:
                    mg["nearest"] = min(mg["nearest"], (dn - dk) / dn)
            c = table[cand, g]
            s = 0.0
            for v in c:                                                    # float64, in key order
                s += float(v)
            mean = s / k
            ss = 0.0
            for v in c:
                ss += (float(v) - mean) * (float(v) - mean)
            with np.errstate(invalid="ignore", divide="ignore"):
                var = np.float64(ss) / np.float64(k - 1)                   # TOPK 1: 0 / 0 = NaN, nothing is positive
                thresh = F32(F32(F32(mean) + F32(np.sqrt(var))) + F32(1e-6))
            if not np.isnan(thresh) and c.any():                           # all candidates exactly 0: thresh is 1e-6 in every order
                mg["thresh"] = min(mg["thresh"], float(np.abs(c.astype(np.float64) - np.float64(thresh)).min()))
            h = F32(-gt[g, 6])
            cs, sn = np.cos(h), np.sin(h)
            dx, dy = anchors[cand, 0] - gt[g, 0], anchors[cand, 1] - gt[g, 1]
            xl = (dx * cs + dy * (-sn)).astype(F32)
            yl = (dx * sn + dy * cs).astype(F32)
            lx, ly = gt[g, 4], gt[g, 3]                                     # as written: x against dy, y against dx
            inside = (xl <= lx / 2) & (xl >= -lx / 2) & (yl <= ly / 2) & (yl >= -ly / 2)
            with np.errstate(invalid="ignore"):
                by_iou = c >= thresh
            if by_iou.any():
                face = np.minimum(np.minimum(np.abs(xl - lx / 2), np.abs(xl + lx / 2)), np.minimum(np.abs(yl - ly / 2), np.abs(yl + ly / 2)))[by_iou]
                mg["on_face"] += int((face == 0).sum())
                if (face > 0).any():
                    mg["inside"] = min(mg["inside"], float(face[face > 0].min()))
            for a, v in zip(cand[by_iou & inside], c[by_iou & inside]):
                if v != best[a] and best[a] > -INF:
                    mg["maxima"] = min(mg["maxima"], abs(float(v) - best[a]))
                if v > best[a]:                                            # the first maximum: the lowest g
                    best[a], match[a] = v, g
        for g in range(n):                                                 # forced, no `> 0` guard; the last write wins
            a = int(table[:, g].argmax())
            match[a] = g
            below = table[:, g][table[:, g] < table[a, g]]
            if N > 1 and len(below) and table[a, g] > 0:
                mg["maxima"] = min(mg["maxima"], float(table[a, g]) - float(below.max()))
    lab = np.zeros(N, np.int32)
    m = match >= 0
    if m.any():
        c = gt[match[m], 7]
        ok = (c >= 0) & (c <= n_classes)
        lab[m] = np.where(ok, np.where(ok, c, 0).astype(np.int32), 0)
    fg = lab > 0
    tgt = np.zeros((N, 7), F32)
    if fg.any():
        tgt[fg] = encode(gt[match[fg], :7], anchors[fg])
    return lab, tgt, fg.astype(F32), mg


def host_atss(sets, gt_batch, n_classes, topk, iou):
    """sets: [(anchors (n, 7), per_loc)], every set over the same locations.  (B, G, 8) -> labels (B, A), targets (B, A, 7), weights
    (B, A) in the head's anchor order, and the margins over all frames and sets."""
    stride = sum(p for _, p in sets)
    n_loc = sets[0][0].shape[0] // sets[0][1]
    A, B = n_loc * stride, gt_batch.shape[0]
    lab, tgt, w = np.zeros((B, A), np.int32), np.zeros((B, A, 7), F32), np.zeros((B, A), F32)
    mg, off = new_margins(), 0
    for anchors, per_loc in sets:
        idx = head_index(anchors.shape[0], per_loc, stride, off)
        for b in range(B):
            lab[b, idx], tgt[b, idx], w[b, idx], m = host_atss_set(anchors, gt_batch[b], n_classes, topk, iou)
            mg = merge_margins(mg, m)
        off += per_loc
    return lab, tgt, w, mg


def oracle_iou(match_height):
    from oracle import hvpr_oracle as O
    fn = O.boxes_iou3d if match_height else O.boxes_iou_bev
    return lambda a, b: fn(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32))


# ------------------------------------------------------------------------------------------------ the frames G27 adds
# Boxes that are well conditioned for ATSS on ALL THREE anchor sets of G18's grid (searched for, 14 of 104 random boxes): on every
# set the eight nearest anchors have distinct IoUs, so mean + std is not 1e-6 away from all of them, and one anchor is the best by
# a margin.  A box that holds every nearby anchor of a set (a car over the pedestrian anchors) or lies inside every one of them
# (a pedestrian under the car anchors) has ONE IoU with all of them up to rounding: threshold and best anchor are noise there, in
# the reference as anywhere, and most of G18's and G26's frames on the three-class head are of that kind.
WELL = [[2.9213, -1.0683, -0.905, 3.6252, 0.2022, 1.7225, 0.0209], [3.3829, -0.2081, -1.0849, 1.6034, 0.6131, 1.4624, -2.7135],
        [2.1486, -0.0711, -0.9506, 0.6188, 1.8739, 1.757, 1.1422], [2.1639, 0.3038, -0.9772, 0.3732, 1.8768, 1.79, -1.6954],
        [4.9597, 0.3164, -0.9537, 3.0635, 0.5283, 1.6796, -1.526], [5.2083, 0.234, -0.7541, 0.4759, 1.4067, 1.7578, -1.9018],
        [5.3798, -1.1913, -0.5939, 1.9052, 0.6205, 1.7099, 0.1957], [3.7712, -1.4816, -0.8116, 2.8089, 0.2742, 1.7771, 0.2246],
        [3.269, 0.411, -0.8609, 1.7355, 0.5564, 1.6737, -0.729], [2.3209, -1.3252, -0.727, 0.8631, 1.5219, 1.526, -2.8162],
        [3.6287, -0.0478, -0.6645, 1.3267, 0.9186, 1.797, 2.4888], [4.7625, 0.1454, -1.0247, 1.127, 0.8334, 1.4177, 0.5077],
        [1.2487, -1.0292, -0.8524, 1.9131, 0.2499, 1.5647, -0.2866], [2.5432, 0.5995, -0.7893, 2.9939, 0.6017, 1.7319, -0.4892]]
WELL_CLASS = [1, 1, 1, 1, 1, 1, 2, 3, 2, 2, 2, 3, 2, 1]


def atss_frames(which, car_anchors=None):
    """{name: (G, 8) fp32} on G18's 40 x 32 grid, built from WELL so that both heads pin them at every TOPK."""
    three = which == "3c"
    w = lambda i, c: WELL[i] + [c]
    f = {}
    # a ground truth of another class on the car anchors: no class mask, every set takes it (one class: class 2 is outside 0 .. 1, the
    # product labels 0 where the reference gives the float 2 — deviation (f), applied to the reference's rows by the fixture maker)
    f["other_class_on_car_anchor"] = [w(6, 2)]
    # a class-0 row in the middle: it is matched like any other and labels its anchors 0
    f["class0_in_the_middle"] = [w(0, 1), w(8, 0), w(13, 1)]
    # an all-zero table: far from every anchor, every IoU 0, thresh 1e-6, the forced match goes to anchor 0
    f["all_zero_table"] = [[40.3, 30.7, -1.0, 3.9, 1.6, 1.56, 0.3, 1]]
    # two ground truths sharing their best anchor (identical boxes): the higher row takes it
    f["shared_best_anchor"] = [w(9, 1), w(9, 3 if three else 1)]
    # out of range with best IoU 0, next to a real one
    f["out_of_range_and_near"] = [w(3, 1), [-35.2, 27.9, -1.0, 3.9, 1.6, 1.56, 0.7, 1]]
    # the candidate path at large: twelve boxes apart from each other, of all classes on the three-class head
    f["spread12"] = [w(i, WELL_CLASS[i] if three else 1) for i in (0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13)]
    return {k: np.asarray(v, F32).reshape(-1, 8) for k, v in f.items()}


def face6_case(nudge=False):
    """(anchors (6, 7), gt (1, 8), topk 6): a heading-0 ground truth 4.0 x 1.0 at the origin and six car anchors of rotation 0.  The
    test as written holds the x offset against dy / 2 = 0.5: anchor 1 sits at x = 0.5 exactly (sin(-0) is -0, the rotation leaves
    the offset's bits alone), which is inside.  IoUs ~ (0.60, 0.51, 4 x 0.04): mean + std ~ 0.48, so anchor 0 (also the forced
    match) and anchor 1 pass the IoU test, and anchor 1 is positive ONLY through the closed inside test.  On G18's grid no such
    frame exists at TOPK 8: the eight nearest anchors are two rotations of four locations within 0.17 m of the centre, a face that
    close needs a box under 0.33 m wide, whose IoUs with the two rotations are bimodal, and mean + std lies above the top mode (a
    search over 6000 boxes met none with margins).  nudge: anchor 1 one fp32 step further out, which is outside."""
    x1 = np.nextafter(F32(0.5), F32(1)) if nudge else F32(0.5)
    a = [[0.1, 0.05], [x1, 0.0], [0.2, 1.2], [-0.2, 1.2], [0.2, -1.2], [-0.3, -1.2]]
    anchors = np.array([[x, y, -1.0, 3.9, 1.6, 1.56, 0.0] for x, y in a], F32)
    return anchors, np.array([[0.0, 0.0, -1.0, 4.0, 1.0, 1.5, 0.0, 1.0]], F32), 6


# ------------------------------------------------------------------------------------------------ fixture G27
def load_g27(golden_dir):
    return np.load(os.path.join(golden_dir, "g27_atss.npz"), allow_pickle=False)


def g27_anchor_sets(z, which):
    """[(anchors (n, 7), per_loc)] of one configuration and its class names, the anchors from the product's own generator."""
    import assign3d_cases as A3
    sets, names = A3.g26_anchor_sets(z, which)
    return [(a, p) for a, p, *_ in sets], names


def g27_runs(z, which):
    """[(topk, match_height)] the fixture holds for a configuration."""
    return [(int(k), int(m)) for k, m in z[which + ".runs"]]


def g27_case(z, which, topk, mh, name):
    """(gt (G, 8), pinned, per set [(labels (n,) int32, targets (n, 7), weights (n,))]) — the reference's rows per anchor set, in the
    set's own order; the head-order mapping is the caller's."""
    key = f"{which}.k{topk}.mh{mh}.{name}."
    gt = z[f"{which}.{name}.gt"]
    if not bool(z[key + "pinned"]):
        return gt, False, None
    per_set = []
    for s in range(int(z[which + ".n_sets"])):
        lab = z[key + f"s{s}.labels"].astype(np.int32)
        tgt = np.zeros((lab.shape[0], 7), F32)
        tgt[z[key + f"s{s}.pos_idx"]] = z[key + f"s{s}.pos_targets"]
        per_set.append((lab, tgt, (lab > 0).astype(F32)))
    return gt, True, per_set


def g27_head_order(sets, per_set):
    """The reference's per-set rows written in the head's order (deviation (b))."""
    stride = sum(p for _, p in sets)
    A = sets[0][0].shape[0] // sets[0][1] * stride
    lab, tgt, w = np.zeros(A, np.int32), np.zeros((A, 7), F32), np.zeros(A, F32)
    off = 0
    for (anchors, per_loc), (l, t, ww) in zip(sets, per_set):
        idx = head_index(anchors.shape[0], per_loc, stride, off)
        lab[idx], tgt[idx], w[idx] = l, t, ww
        off += per_loc
    return lab, tgt, w


def check_equal(got, want, where):
    """Labels and weights exact, targets 1e-5 (the bar of G8, G18 and G26), zero targets off the positives."""
    n_bad = int((got[0] != want[0]).sum())
    assert n_bad == 0, f"{where}: {n_bad} of {want[0].size} labels differ, positives {int((got[0] > 0).sum())} against {int((want[0] > 0).sum())}"
    np.testing.assert_array_equal(got[2], want[2], err_msg=where)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-5, atol=1e-6, err_msg=where)
    assert not got[1][want[0] <= 0].any(), where
