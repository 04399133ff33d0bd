"""GPU: the BEV picture op (csrc/bev_render.hip through kernels.render_bev) against the numpy restatement of
tests/bev_vis_cases.py -- which tests/test_bev_vis_host.py pins to fixture G24, the reference's own tools/vis.py -- byte for byte,
and against G24 itself.

Every generated box keeps the margin rule of bev_vis_cases.settle_boxes (no scaled corner coordinate within 1e-2 px of an integer
under either heading sign), so the device's sinf / cosf and numpy's truncate to the same pixels; everything else is integer or
correctly rounded arithmetic and has no tolerance."""
import os

import numpy as np
import pytest

import bev_vis_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEW = [0.0, -1.85, -1.0, 5.3, 1.85, 1.0]          # 37 x 53 pixels at 0.1 m: a multiple of nothing
PIXEL = 0.1
PALETTE = np.array([[9, 9, 9], [0, 255, 0], [0, 200, 255], [255, 255, 0], [255, 64, 64]], np.uint8)


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


def run_op(points, offsets, xyz_col, rng, pixel, tables, palette=PALETTE, thickness=2, sign=-1, want_counts=True):
    """The op on host inputs -> (image, counts) as numpy."""
    import torch
    from hvpr_amd import kernels
    dt = []
    for t in tables:
        d = {"boxes": _dev(t["boxes"], np.float32), "ink": t.get("ink", 1), "thresh": t.get("thresh", 0.0)}
        d["count"], d["scores"], d["labels"] = _dev(t.get("count"), np.int32), _dev(t.get("scores"), np.float32), _dev(t.get("labels"), np.int64)
        dt.append(d)
    image, counts, _ = kernels.render_bev(_dev(points, np.float32), _dev(offsets, np.int32), rng, pixel, _dev(palette), tables=dt,
                                          xyz_col=xyz_col, thickness=thickness, heading_sign=sign, want_counts=want_counts)
    torch.cuda.synchronize()
    return image.cpu().numpy(), None if counts is None else counts.cpu().numpy()


def check(points, offsets, xyz_col, tables, rng=VIEW, pixel=PIXEL, palette=PALETTE, thickness=2, sign=-1):
    got_im, got_ct = run_op(points, offsets, xyz_col, rng, pixel, tables, palette, thickness, sign)
    want_im, want_ct = C.render_batch(points, offsets, xyz_col, rng, pixel, tables, palette, thickness, sign)
    assert got_ct.dtype == np.int32 and got_ct.shape == want_ct.shape and (got_ct == want_ct).all()
    assert got_im.dtype == np.uint8 and got_im.shape == want_im.shape
    assert (got_im == want_im).all(), f"{int((got_im != want_im).any(axis=-1).sum())} pixels differ"
    return want_im, want_ct


def ragged(gen, sizes, col):
    """(points (sum n, col + 4), offsets): frames of the given sizes, xyz at column `col` (the frame index in front of it)."""
    rows, off = [], [0]
    for b, n in enumerate(sizes):
        p = C.frame_points(gen, n, VIEW)
        rows.append(np.concatenate([np.full((n, col), b, np.float32), p], axis=1))
        off.append(off[-1] + n)
    return np.concatenate(rows, axis=0), np.array(off, np.int32)


# ------------------------------------------------------------------------------------------------ height pass
@pytest.mark.parametrize("col", [0, 1])
@pytest.mark.parametrize("sizes", [(0,), (1,), (63,), (64,), (65,), (2049,), (65, 0, 2049), (0, 0, 1)])
def test_height_and_counts(sizes, col):
    pts, off = ragged(np.random.default_rng(100 + sum(sizes) + col), sizes, col)
    im, ct = check(pts, off, col, [])
    assert ct.shape == (len(sizes), 37, 53)
    inside = sum(int(((p >= np.array(VIEW[:3], np.float32)) & (p < np.array(VIEW[3:], np.float32))).all(axis=1).sum())
                 for p in (pts[off[b]:off[b + 1], col:col + 3] for b in range(len(sizes))))
    assert abs(int(ct.sum()) - inside) <= 2            # cells decide at the borders; the plain test only says most points landed
    for b, n in enumerate(sizes):
        if n == 0:
            assert ct[b].sum() == 0 and (im[b] == 0).all()


def test_borders_and_bad_points():
    lo, hi = np.array(VIEW[:3], np.float32), np.array(VIEW[3:], np.float32)
    mid = (lo + hi) / 2
    rows = []
    for j in range(3):
        for v in (lo[j], hi[j], np.nextafter(hi[j], np.float32(-9), dtype=np.float32), np.nextafter(lo[j], np.float32(-9), dtype=np.float32),
                  np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(3e38)):
            p = mid.copy()
            p[j] = v
            rows.append(p)
    pts = np.concatenate([np.array(rows, np.float32), np.zeros((len(rows), 1), np.float32)], axis=1)
    _, ct = check(pts, np.array([0, len(pts)], np.int32), 0, [])
    # per axis on lo; just under hi on x and y -- on z, (z - z_lo) rounds up to the slice's height in float32 and the point is dropped
    assert ct.sum() == 5


def test_two_thousand_points_in_one_cell():
    gen = np.random.default_rng(3)
    pts = np.zeros((2000, 4), np.float32)
    pts[:, 0] = gen.uniform(2.01, 2.09, 2000)
    pts[:, 1] = gen.uniform(0.36, 0.44, 2000)
    pts[:, 2] = gen.uniform(-0.99, 0.99, 2000)
    im, ct = check(pts, np.array([0, 2000], np.int32), 0, [])
    assert ct.max() == 2000 and (ct > 0).sum() == 1 and im.max() >= 250


def test_rows_no_frame_owns_are_dropped():
    pts, _ = ragged(np.random.default_rng(4), (300,), 1)
    check(pts, np.array([40, 100, 100, 260], np.int32), 1, [])


# ------------------------------------------------------------------------------------------------ box pass
def table(gen, B, P, **kw):
    return dict({"boxes": np.stack([C.random_boxes(gen, P, VIEW, PIXEL) for _ in range(B)]).reshape(B, P, 7)}, **kw)


@pytest.mark.parametrize("P", [0, 1, 65])
@pytest.mark.parametrize("thickness", [1, 2, 5])
def test_boxes(P, thickness):
    gen = np.random.default_rng(10 * P + thickness)
    pts, off = ragged(gen, (200, 0, 300), 1)
    im, _ = check(pts, off, 1, [table(gen, 3, P, ink=1)], thickness=thickness)
    assert ((im == PALETTE[1]).all(axis=-1).any()) == (P > 0)


def test_count_scores_labels_and_a_second_table():
    gen = np.random.default_rng(20)
    pts, off = ragged(gen, (150, 150), 1)
    P = 12
    scores = gen.uniform(0.0, 1.0, (2, P)).astype(np.float32)
    thresh = np.float32(0.3)
    scores[0, 0], scores[0, 1] = thresh, np.nextafter(thresh, np.float32(0), dtype=np.float32)      # drawn / not drawn
    scores[1, 2] = np.nan
    labels = gen.integers(1, 4, (2, P)).astype(np.int64)
    labels[1, 0], labels[1, 1] = 0, 7                                                               # ink 0 and past the palette
    pred = table(gen, 2, P, ink=0, labels=labels, scores=scores, thresh=float(thresh), count=np.array([9, 3], np.int32))
    gt = table(gen, 2, 5, ink=4)
    gt["boxes"] = np.concatenate([gt["boxes"], np.ones((2, 5, 1), np.float32)], axis=2)             # 8 floats per row
    gt["scores"], gt["thresh"] = np.array([[1, 1, 0, 0, 0], [1, 0, 0, 0, 0]], np.float32), 0.5
    check(pts, off, 1, [pred, gt])
    # the threshold row alone, both ways
    one = {"boxes": pred["boxes"][:1, :2], "scores": scores[:1, :2], "thresh": float(thresh), "ink": 2}
    im, _ = check(pts[:150], off[:2], 1, [one])
    only_first = dict(one, boxes=one["boxes"][:, :1], scores=one["scores"][:, :1])
    assert (im == C.render_batch(pts[:150], off[:2], 1, VIEW, PIXEL, [only_first], PALETTE)[0]).all()
    # a count past the table draws the table, a negative one nothing
    check(pts, off, 1, [dict(pred, count=np.array([999, -4], np.int32))])


def test_larger_ink_wins_where_boxes_overlap():
    gen = np.random.default_rng(21)
    a = C.settle_boxes(np.array([[2.6, 0.0, 0, 3.0, 1.6, 1.5, 0.3], [2.7, 0.1, 0, 3.0, 1.6, 1.5, -0.5]], np.float32), VIEW, PIXEL, gen)
    pts = np.zeros((0, 4), np.float32)
    off = np.array([0, 0], np.int32)
    for order in ([0, 1], [1, 0]):
        t = {"boxes": a[order][None], "labels": np.array([order], np.int64) * 2 + 1, "ink": 0}     # box 0: ink 1, box 1: ink 3
        im, _ = check(pts, off, 0, [t], thickness=3)
        both = [(im[0] == PALETTE[k]).all(axis=-1) for k in (1, 3)]
        assert both[0].any() and both[1].any()
    solo = [C.render_batch(pts, off, 0, VIEW, PIXEL, [{"boxes": a[k:k + 1][None], "ink": 1}], PALETTE, 3)[0][0] for k in (0, 1)]
    cross = (solo[0] == PALETTE[1]).all(axis=-1) & (solo[1] == PALETTE[1]).all(axis=-1)
    assert cross.any() and (im[0][cross] == PALETTE[3]).all()


def test_degenerate_bad_and_far_boxes():
    gen = np.random.default_rng(22)
    good = C.random_boxes(gen, 4, VIEW, PIXEL)
    zero = C.settle_boxes(np.array([[2.13, 0.27, 0, 0, 0, 0, 0.4]], np.float32), VIEW, PIXEL, gen)           # segments of length 0
    nan = good[1:2].copy(); nan[0, 4] = np.nan
    inf = good[2:3].copy(); inf[0, 0] = np.inf
    badz = good[3:4].copy(); badz[0, 2] = np.nan                                                           # any non-finite field
    far = np.array([[2.65, 0.0, 0, 3.1, 4000.0, 1.5, 0.0],         # two edges run far past the clamp, through the picture
                    [3e6, 3e6, 0, 4.0, 2.0, 1.5, 0.7],             # wholly beyond it
                    [2.65, 0.0, 0, 3e38, 3e38, 1.5, 0.7]], np.float32)                                    # as large as float32 gets
    far[:1] = C.settle_boxes(far[:1], VIEW, PIXEL, gen)
    boxes = np.concatenate([good[:1], nan, zero, inf, far, badz, good[1:]], axis=0)
    pts, off = ragged(gen, (100,), 0)
    for t in (1, 2):
        im, _ = check(pts, off, 0, [{"boxes": boxes[None], "ink": 2}], thickness=t)
    seg, drawn = C.box_segments(boxes, VIEW, PIXEL, -1)
    assert drawn.tolist() == [True, False, True, False, True, True, True, False, True, True, True]
    assert np.abs(seg[4]).max() == C.CLAMP and (im[0, :, seg[4][0, 0]] == PALETTE[2]).all()               # a whole column inked


def test_g24_is_the_references_record(golden_dir):
    g = np.load(os.path.join(golden_dir, "g24_bev_vis.npz"))
    rng, pixel, pts, boxes = g["range"], float(g["pixel"]), g["full_points"], g["boxes"]
    pal = np.array([[0, 0, 0], [0, 255, 0]], np.uint8)
    off = np.array([0, len(pts), len(pts)], np.int32)                                   # the full frame, then the empty one
    tab = {"boxes": np.stack([boxes, boxes]), "ink": 1}
    im, ct = run_op(pts, off, 0, rng, pixel, [tab], pal, thickness=int(g["segment_thickness"][0]), sign=1)
    assert (ct[0] == g["full_counts"]).all() and (ct[1] == g["empty_counts"]).all()
    for b, tag in enumerate(("full", "empty")):
        ink = np.zeros(ct[b].shape, np.uint32)
        for s in g["segments"]:                                                          # what the reference handed to cv2.line
            C.draw_segment(ink, s, 1, int(g["segment_thickness"][0]))
        want = g[tag + "_image"].copy()
        want[ink > 0] = g["segment_colour"][0]
        assert (im[b] == want).all()
    # the same boxes with negated headings under sign -1: the same bytes
    neg = tab["boxes"].copy()
    neg[:, :, 6] = -neg[:, :, 6]
    im2, _ = run_op(pts, off, 0, rng, pixel, [{"boxes": neg, "ink": 1}], pal, thickness=2, sign=-1)
    assert (im2 == im).all()
    no_boxes, _ = run_op(pts, off, 0, rng, pixel, [], pal)
    assert (no_boxes[0] == g["full_image"]).all() and (no_boxes[1] == g["empty_image"]).all()


# ------------------------------------------------------------------------------------------------ contract
def test_refusals_leave_the_outputs_alone():
    import torch
    from hvpr_amd import _lib
    L = _lib.lib()
    B, H, W = 1, 37, 53
    pts = _dev(C.frame_points(np.random.default_rng(30), 50, VIEW))
    off, pal = _dev(np.array([0, 50], np.int32)), _dev(PALETTE)
    image = torch.full((B, H, W, 3), 171, dtype=torch.uint8, device=DEV)
    counts = torch.full((B, H, W), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((L.hvpr_render_bev_workspace_bytes(B, H, W),), 85, dtype=torch.uint8, device=DEV)
    rng = np.array(VIEW, np.float32)
    boxes = _dev(C.random_boxes(np.random.default_rng(31), 3, VIEW, PIXEL)[None])

    def call(**kw):
        a = dict(points=pts.data_ptr(), n=50, stride=4, col=0, off=off.data_ptr(), B=B, rng=rng.ctypes.data, pixel=PIXEL,
                 boxes=boxes.data_ptr(), rows=3, bstride=7, pal=pal.data_ptr(), n_ink=5, thick=2, sign=-1, image=image.data_ptr(),
                 counts=counts.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(kw)
        return L.hvpr_render_bev_u8(a["points"], a["n"], a["stride"], a["col"], a["off"], a["B"], a["rng"], a["pixel"],
                                    a["boxes"], a["rows"], a["bstride"], None, None, 0.0, None, 1, None, 0, 7, None, None, 0.0, None, 1,
                                    a["pal"], a["n_ink"], a["thick"], a["sign"], a["image"], a["counts"], a["ws"], a["ws_bytes"],
                                    torch.cuda.current_stream().cuda_stream)
    wide = np.array([0.0, -1.85, -1.0, 819.3, 1.85, 1.0], np.float32)                   # W = 8193, one past the cap
    nan_rng = rng.copy(); nan_rng[3] = np.nan
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    for kw, want in (({"points": None}, INVALID), ({"off": None}, INVALID), ({"rng": None}, INVALID), ({"image": None}, INVALID),
                     ({"pal": None}, INVALID), ({"ws": None}, INVALID), ({"n_ink": 0}, INVALID), ({"B": 0}, INVALID),
                     ({"thick": 0}, INVALID), ({"sign": 0}, INVALID), ({"col": 2}, INVALID), ({"pixel": 0.0}, INVALID),
                     ({"bstride": 6}, INVALID), ({"rows": -1}, INVALID), ({"rng": nan_rng.ctypes.data}, INVALID),
                     ({"rng": wide.ctypes.data}, UNSUPPORTED), ({"thick": 256}, UNSUPPORTED), ({"ws_bytes": ws.numel() - 1}, WORKSPACE)):
        assert call(**kw) == want, (kw, want)
    torch.cuda.synchronize()
    assert (image == 171).all() and (counts == -7).all() and (ws == 85).all()
    assert L.hvpr_render_bev_workspace_bytes(1, 37, 8193) == 0 and L.hvpr_render_bev_workspace_bytes(0, 37, 53) == 0
    assert call() == 0                                                                   # and the same call, unchanged, runs
    torch.cuda.synchronize()
    want_im, want_ct = C.render_batch(pts.cpu().numpy(), [0, 50], 0, VIEW, PIXEL, [{"boxes": boxes.cpu().numpy(), "ink": 1}], PALETTE)
    assert (image.cpu().numpy() == want_im).all() and (counts.cpu().numpy() == want_ct).all()


def test_repeatable_and_without_a_host_read():
    import torch
    from hvpr_amd import kernels
    gen = np.random.default_rng(40)
    pts, off = ragged(gen, (2049, 700), 1)
    t = table(gen, 2, 30, ink=0, labels=gen.integers(1, 5, (2, 30)).astype(np.int64), count=np.array([30, 11], np.int32))
    first, ct = run_op(pts, off, 1, VIEW, PIXEL, [t], thickness=5)
    d_pts, d_off, d_pal = _dev(pts), _dev(off), _dev(PALETTE)
    d_t = {"boxes": _dev(t["boxes"]), "labels": _dev(t["labels"]), "count": _dev(t["count"]), "ink": 0}
    image = torch.empty((2, 37, 53, 3), dtype=torch.uint8, device=DEV)
    counts = torch.empty((2, 37, 53), dtype=torch.int32, device=DEV)
    _, _, ws = kernels.render_bev(d_pts, d_off, VIEW, PIXEL, d_pal, tables=[d_t], xyz_col=1, thickness=5, image=image, counts=counts)
    torch.cuda.synchronize()
    image.fill_(3)
    torch.cuda.set_sync_debug_mode("error")
    try:
        kernels.render_bev(d_pts, d_off, VIEW, PIXEL, d_pal, tables=[d_t], xyz_col=1, thickness=5, image=image, counts=counts,
                           workspace=ws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (image.cpu().numpy() == first).all() and (counts.cpu().numpy() == ct).all()


def test_bev_vis_render_bev_on_a_loader_shaped_batch():
    """hvpr_amd.bev_vis.render_bev: the batch column, the records' padded rows, the ground truth's padded rows and its ink."""
    from hvpr_amd import bev_vis
    gen = np.random.default_rng(50)
    pts, off = ragged(gen, (400, 300), 1)
    P = 8
    pred = table(gen, 2, P)
    labels = gen.integers(1, 3, (2, P)).astype(np.int64)
    scores = gen.uniform(0, 1, (2, P)).astype(np.float32)
    count = np.array([5, 0], np.int32)
    gt = np.zeros((2, 3, 8), np.float32)
    gt[0, :2, :7], gt[0, :2, 7] = C.random_boxes(gen, 2, VIEW, PIXEL), [1, 2]
    gt[1, :1, :7], gt[1, :1, 7] = C.random_boxes(gen, 1, VIEW, PIXEL), [2]
    batch = {"points": _dev(pts), "point_frame_offsets": _dev(off), "batch_size": 2, "gt_boxes": _dev(gt)}
    records = [{"pred_boxes": _dev(pred["boxes"][b]), "pred_labels": _dev(labels[b]), "pred_scores": _dev(scores[b]),
                "pred_count": _dev(count[b:b + 1])} for b in range(2)]
    pal = bev_vis.class_palette(2)
    tabs = [{"boxes": pred["boxes"], "labels": labels, "count": count, "ink": 0},
            {"boxes": gt, "scores": gt[:, :, 7], "thresh": 0.5, "ink": 3}]
    got = bev_vis.render_bev(batch, records, point_cloud_range=VIEW, num_class=2).cpu().numpy()
    assert (got == C.render_batch(pts, off, 1, VIEW, PIXEL, tabs, pal, 2, -1)[0]).all()
    tabs[0].update(scores=scores, thresh=0.4)
    got = bev_vis.render_bev(batch, records, point_cloud_range=VIEW, num_class=2, score_thresh=0.4, thickness=1, heading_sign=1)
    assert (got.cpu().numpy() == C.render_batch(pts, off, 1, VIEW, PIXEL, tabs, pal, 1, 1)[0]).all()
    got = bev_vis.render_bev(batch, None, point_cloud_range=VIEW, num_class=2, draw_gt=False).cpu().numpy()
    assert (got == C.render_batch(pts, off, 1, VIEW, PIXEL, [], pal)[0]).all()


def test_replays_from_a_captured_graph():
    """The call only enqueues on the current stream: captured once, it renders whatever the buffers hold at each replay."""
    import torch
    from hvpr_amd import kernels
    gen = np.random.default_rng(60)
    sizes = (500, 0, 321)
    pts, off = ragged(gen, sizes, 1)
    t = table(gen, 3, 6, ink=0, labels=gen.integers(1, 5, (3, 6)).astype(np.int64), count=np.array([6, 2, 0], np.int32))
    d_pts, d_off, d_pal = _dev(pts), _dev(off), _dev(PALETTE)
    d_t = {"boxes": _dev(t["boxes"]), "labels": _dev(t["labels"]), "count": _dev(t["count"]), "ink": 0}
    image = torch.empty((3, 37, 53, 3), dtype=torch.uint8, device=DEV)
    counts = torch.empty((3, 37, 53), dtype=torch.int32, device=DEV)
    _, _, ws = kernels.render_bev(d_pts, d_off, VIEW, PIXEL, d_pal, tables=[d_t], xyz_col=1, image=image, counts=counts)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.render_bev(d_pts, d_off, VIEW, PIXEL, d_pal, tables=[d_t], xyz_col=1, image=image, counts=counts, workspace=ws)
    for seed in (61, 62):                                           # new points, boxes and counts in the same buffers
        g2 = np.random.default_rng(seed)
        pts2, _ = ragged(g2, sizes, 1)
        t2 = dict(t, boxes=table(g2, 3, 6)["boxes"], count=np.array([seed % 7, 6, 1], np.int32))
        d_pts.copy_(_dev(pts2)); d_t["boxes"].copy_(_dev(t2["boxes"])); d_t["count"].copy_(_dev(t2["count"]))
        image.fill_(77); counts.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want_im, want_ct = C.render_batch(pts2, off, 1, VIEW, PIXEL, [t2], PALETTE)
        assert (image.cpu().numpy() == want_im).all() and (counts.cpu().numpy() == want_ct).all()
