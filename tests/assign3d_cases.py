"""Shared bodies of the MATCH_HEIGHT / NORM_BY_NUM_EXAMPLES target-assigner checks (tests/test_assign3d_host.py on the CPU,
tests/test_gpu_assign3d.py on the device): a numpy host form of the assigner over ANY (anchors, ground truths) -> IoU table, the
frames fixture G26 adds to G18's, a numpy restatement of the two exact rejects (to say how many pairs a workgroup of the kernel
clips), and the fixture's reader.  The host form follows torch_forms._assign_frames, which G8 and G18 pin to the reference for the
nearest-axis table; G26 (tests/golden/make_golden_assign3d.py) pins it for the rotated 3-D IoU of oracle.hvpr_oracle.boxes_iou3d."""
import os

import numpy as np

F32 = np.float32
WAVE = 64                                         # anchors per workgroup of k_assign3d


# ------------------------------------------------------------------------------------------------ the host form
def trim_and_mask(gt, class_index, n_classes):
    """(G, 8) -> (use (G,) bool, class ids (G,) int32): trailing rows whose signed fp32 sum over the 7 box fields is 0 are padding, row
    0 always stays; a row takes part when python's class_names[c - 1] is this set's class."""
    s = np.zeros(gt.shape[0], F32)
    for j in range(7):
        s = (s + gt[:, j]).astype(F32)
    nz = np.nonzero(s != 0)[0]
    last = int(nz.max()) if len(nz) else 0
    c = gt[:, 7].astype(np.int32)
    return (np.arange(gt.shape[0]) <= last) & (((c - 1) % n_classes) == class_index), c


def encode(gt7, an):
    """ResidualCoder.encode_torch (box_coder_utils.py:13-43) in fp32 numpy, row by row."""
    g, a = gt7.astype(F32).copy(), an.astype(F32).copy()
    g[:, 3:6] = np.maximum(g[:, 3:6], F32(1e-5))
    a[:, 3:6] = np.maximum(a[:, 3:6], F32(1e-5))
    diag = np.sqrt(a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4])
    return np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / a[:, 5], np.log(g[:, 3] / a[:, 3]),
                     np.log(g[:, 4] / a[:, 4]), np.log(g[:, 5] / a[:, 5]), g[:, 6] - a[:, 6]], axis=1).astype(F32)


def host_assign_set(anchors, gt, class_index, n_classes, matched, unmatched, norm, iou):
    """One frame, one anchor set, the set's own anchor order: labels (A,) int32, targets (A, 7) fp32, weights (A,) fp32.
    iou(anchors (A, 7), boxes (G, 7)) -> (A, G) fp32."""
    A, G = anchors.shape[0], gt.shape[0]
    lab = np.zeros(A, np.int32)
    tgt = np.zeros((A, 7), F32)
    if G > 0:
        use, cls = trim_and_mask(gt, class_index, n_classes)
        table = np.asarray(iou(anchors[:, :7], gt[:, :7]), F32).copy()
        assert table.shape == (A, G)
        table[:, ~use] = F32(-2.0)                                              # masked ground truths never match
        arg = table.argmax(axis=1)                                              # the first maximum
        best = table[np.arange(A), arg]
        g2a = table.max(axis=0)
        g2a = np.where(g2a <= 0, F32(-1.0), g2a)                               # no overlap at all: no forced match
        force = (table == g2a[None, :]).any(axis=1)
        cls_of = cls[arg]
        lab[:] = -1
        lab = np.where(force, cls_of, lab)
        lab = np.where(best >= F32(matched), cls_of, lab)
        lab = np.where(best < F32(unmatched), 0, lab)
        lab = np.where(force, cls_of, lab).astype(np.int32)                     # forced matches win over background
        fg = lab > 0
        tgt[fg] = encode(gt[arg[fg], :7], anchors[fg])
    fg = lab > 0
    n = max(int((lab >= 0).sum()), 1)
    w = np.where(fg, F32(1.0) / F32(n) if norm else F32(1.0), F32(0.0)).astype(F32)
    return lab, tgt, w


def head_index(n, per_loc, stride, off):
    a = np.arange(n)
    return (a // per_loc) * stride + off + a % per_loc


def host_assign(sets, gt_batch, n_classes, norm, iou):
    """sets: [(anchors (n, 7), per_loc, class_index, matched, unmatched)], every set over the same locations.  (B, G, 8) ->
    labels (B, A), targets (B, A, 7), weights (B, A) in the head's anchor order."""
    stride = sum(s[1] for s in sets)
    n_loc = sets[0][0].shape[0] // sets[0][1]
    A, B = n_loc * stride, gt_batch.shape[0]
    lab, tgt, w = np.zeros((B, A), np.int32), np.zeros((B, A, 7), F32), np.zeros((B, A), F32)
    off = 0
    for anchors, per_loc, class_index, matched, unmatched in sets:
        idx = head_index(anchors.shape[0], per_loc, stride, off)
        for b in range(B):
            lab[b, idx], tgt[b, idx], w[b, idx] = host_assign_set(anchors, gt_batch[b], class_index, n_classes, matched, unmatched, norm, iou)
        off += per_loc
    return lab, tgt, w


def oracle_iou3d():
    from oracle import hvpr_oracle as O
    return lambda a, b: O.boxes_iou3d(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32))


# ------------------------------------------------------------------------------------------------ the two exact rejects, restated
def _lite(b):
    b = b.astype(F32)
    return dict(x=b[:, 0], y=b[:, 1], hx=F32(0.5) * b[:, 3], hy=F32(0.5) * b[:, 4], cs=np.cos(b[:, 6]), sn=np.sin(b[:, 6]),
                rad=F32(0.5) * np.sqrt(b[:, 3] * b[:, 3] + b[:, 4] * b[:, 4]))


def reach_the_clip(anchors, boxes):
    """(A, G) bool: the pairs neither far_apart nor axes_separate (iou_geom.h) rejects — within rounding of the device's sin / cos, so
    use it to describe a case (how many pairs a workgroup clips), not to predict a value."""
    a = {k: v[:, None] for k, v in _lite(anchors).items()}
    g = {k: v[None, :] for k, v in _lite(boxes).items()}
    ddx, ddy = g["x"] - a["x"], g["y"] - a["y"]
    lim = a["rad"] + g["rad"] + F32(0.05)
    far = ddx * ddx + ddy * ddy > lim * lim * F32(1.0001)
    c = np.abs(a["cs"] * g["cs"] + a["sn"] * g["sn"])
    s = np.abs(g["sn"] * a["cs"] - g["cs"] * a["sn"])
    m = F32(0.05)
    sep = ((np.abs(ddx * a["cs"] + ddy * a["sn"]) > a["hx"] + g["hx"] * c + g["hy"] * s + m) |
           (np.abs(ddy * a["cs"] - ddx * a["sn"]) > a["hy"] + g["hx"] * s + g["hy"] * c + m) |
           (np.abs(ddx * g["cs"] + ddy * g["sn"]) > g["hx"] + a["hx"] * c + a["hy"] * s + m) |
           (np.abs(ddy * g["cs"] - ddx * g["sn"]) > g["hy"] + a["hx"] * s + a["hy"] * c + m))
    return ~(far | sep)


def pairs_per_workgroup(anchors, gt, class_index, n_classes):
    """Clipped pairs of every 64-anchor workgroup of one frame and set."""
    use, _ = trim_and_mask(gt, class_index, n_classes)
    live = reach_the_clip(anchors, gt[:, :7])[:, use].sum(axis=1)
    pad = (-len(live)) % WAVE
    return np.concatenate([live, np.zeros(pad, live.dtype)]).reshape(-1, WAVE).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the frames G26 adds to G18's
def extra_frames(which):
    """{name: (G, 8) fp32} for G18's class configuration `which` ("car" / "3c"), on G18's 40 x 32 grid of 0.16 m cells over
    x 0..6.4, y -2.56..2.56 (car anchors 3.9 x 1.6 x 1.56, centres at z -1.0)."""
    three = which == "3c"
    car = [1.5, 1.0, -1.0, 4.0, 1.5, 1.5, 0.0, 1]
    f = {}
    # overlaps anchors in BEV, disjoint in z: the clip runs, the IoU is exactly 0, no forced match (the nearest-axis matcher forces one)
    high = car[:2] + [5.0] + car[3:]
    f["z_disjoint_only"] = [high]
    f["z_disjoint_and_near"] = [high, [4.5, -1.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]]
    f["z_sliver"] = [car[:2] + [0.5] + car[3:]]                           # bottom -0.25 under the anchors' top -0.22: 3 cm in common
    f["zero_row0"] = [[0.0] * 8, car]
    # rows of a foreign class (the one-class reference raises IndexError on class 2: three classes only) and of class 0
    f["foreign_and_class0"] = ([car[:7] + [2]] if three else []) + [car[:7] + [0], [4.0, -1.0, -1.0, 3.9, 1.6, 1.56, 1.2, 1]]
    # headings on +-pi/4, pi/2 and general
    hs = [np.pi / 4, -np.pi / 4, np.pi / 2, 0.3, -2.0, 3.0]
    f["headings"] = [[1.0 + 0.9 * i, -1.5 + 0.6 * i, -1.0, 3.9, 1.6, 1.56, float(F32(h)), 1] for i, h in enumerate(hs)]
    if three:
        f["headings"] += [[1.0 + 0.9 * i, 1.5 - 0.5 * i, -0.6, 0.8, 0.6, 1.73, float(F32(h)), 2] for i, h in enumerate(hs)]
        f["headings"] += [[5.5 - 0.8 * i, 2.0 - 0.7 * i, -0.6, 1.76, 0.6, 1.73, float(F32(h)), 3] for i, h in enumerate(hs)]
    # a ground truth past the grid's far corner: it reaches a handful of anchors there and is alone in their workgroups
    f["corner_reach"] = [[8.9, 4.0, -1.0, 3.9, 1.6, 1.56, 0.6, 1]]
    # ten ground truths stacked on one spot, headings 0.05 apart: every anchor near them meets all ten
    f["stacked10"] = [[3.2, 0.1, -1.0, 3.9, 1.6, 1.56, 0.05 * i, 1] for i in range(10)]
    if three:
        f["stacked10"] += [[3.2, 0.1, -0.6, 0.8, 0.6, 1.73, 0.05 * i, 2] for i in range(10)]
    return {k: np.asarray(v, F32).reshape(-1, 8) for k, v in f.items()}


# ------------------------------------------------------------------------------------------------ fixture G26
def load_g26(golden_dir):
    return np.load(os.path.join(golden_dir, "g26_assigner_match_height.npz"), allow_pickle=False)


def g26_anchor_sets(z, which):
    """[(anchors (n, 7), per_loc, class_index, matched, unmatched)] of one configuration, the anchors generated by the product's
    own generator from the fixture's plain values (G4 pins it to the reference's)."""
    import train_fixture_cases as C
    head = C._g18_head(z, which, "cpu")                                   # G26 keeps the grid and class values under G18's key names
    names = [str(n) for n in z[which + ".class_names"]]
    return [(a.reshape(-1, 7).numpy().astype(F32), int(a.shape[3] * a.shape[4]), k, float(m), float(u))
            for k, (a, m, u) in enumerate(zip(head.anchors, z[which + ".matched"], z[which + ".unmatched"]))], names


def g26_case(z, which, name, norm):
    """(gt (G, 8), labels (A,) int32, targets (A, 7), weights (A,)) the reference gave for one frame."""
    key = f"{which}.{name}."
    lab = z[key + "labels"].astype(np.int32)
    tgt = np.zeros((lab.shape[0], 7), F32)
    tgt[z[key + "pos_idx"]] = z[key + "pos_targets"]
    return z[key + "gt"], lab, tgt, z[key + ("reg_weights_norm" if norm else "reg_weights")]


def check_against_g26(z, which, name, norm, got, tag=""):
    """got: (labels, targets, weights) as numpy.  Labels and weights exact, targets 1e-5 (the bar of G8 and G18)."""
    _, lab, tgt, w = g26_case(z, which, name, norm)
    where = f"{tag}{which}.{name} norm={norm}"
    n_bad = int((got[0] != lab).sum())
    assert n_bad == 0, f"{where}: {n_bad} labels differ, positives {int((got[0] > 0).sum())} against the reference's {int((lab > 0).sum())}"
    np.testing.assert_array_equal(got[2], w, err_msg=where)
    np.testing.assert_allclose(got[1], tgt, rtol=1e-5, atol=1e-6, err_msg=where)
    assert not got[1][lab <= 0].any(), where
