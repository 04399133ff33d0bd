"""CPU: the host side of the device KITTI AP evaluator (hvpr_amd/kitti_eval_device.py) — the annotation tables, the closed form
of the counting pass's pick against kitti_eval._pick, the argument checks of the new entry points (answered before anything touches
the device), and that the hand-made edge set of tests/kitti_ap_cases.py really holds the cases it is there for."""
import ctypes

import numpy as np
import pytest

from hvpr_amd import kitti_eval, kitti_eval_device as KD
from kitti_ap_cases import HostRun, edge_set, with_empty_ends
from make_golden import synthetic_kitti_annos

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


def _anno(names, dtype=np.float64, score=False, seed=0):
    rng = np.random.default_rng(seed + len(names))
    n = len(names)
    a = {"name": np.array(names, dtype="<U16"), "truncated": rng.uniform(0, 1, n).astype(dtype), "occluded": rng.integers(0, 4, n),
         "alpha": rng.uniform(-3, 3, n).astype(dtype), "bbox": rng.uniform(0, 500, (n, 4)).astype(dtype),
         "dimensions": rng.uniform(0.5, 4, (n, 3)).astype(dtype), "location": rng.uniform(-20, 40, (n, 3)).astype(dtype),
         "rotation_y": rng.uniform(-3, 3, n).astype(dtype)}
    if score:
        a["score"] = rng.uniform(0, 1, n).astype(dtype)
    return a


# ------------------------------------------------------------------------------------------------ tables
def test_names_classes_and_the_dontcare_bit():
    names = ["car", "CAR", "Van", "dontcare", "DontCare", "Tram", "Person_sitting", "truck", "Cyclist", "pedestrian"]
    t = KD.AnnoTables([_anno(names)], [_anno(names, score=True)])
    assert list(t.gt_cls) == [0, 0, 3, -1, -1, -1, 4, 5, 2, 1] and t.gt_cls.dtype == np.int32
    assert list(t.dt_cls) == list(t.gt_cls)
    assert list(t.gt_dontcare) == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]          # the lower-case spelling is NOT DontCare (clean_data)
    g = _anno(names)
    dc = kitti_eval.clean_data(g, _anno(names, score=True), 0, 0)[3]
    np.testing.assert_array_equal(dc, t.gt_rows[t.gt_dontcare.astype(bool), 0:4])


def test_offsets_with_empty_frames_and_row_layout():
    counts_g, counts_d = [0, 3, 0, 0, 2, 0], [0, 2, 4, 0, 5, 0]
    gts = [_anno(["Car"] * n, seed=i) for i, n in enumerate(counts_g)]
    dts = [_anno(["Car"] * n, score=True, seed=10 + i) for i, n in enumerate(counts_d)]
    t = KD.AnnoTables(gts, dts)
    assert t.gt_off.dtype == t.dt_off.dtype == t.pair_off.dtype == np.int64
    assert list(t.gt_off) == [0, 0, 3, 3, 3, 5, 5] and list(t.dt_off) == [0, 0, 2, 6, 6, 11, 11]
    assert list(np.diff(t.pair_off)) == [d * g for d, g in zip(counts_d, counts_g)] and t.pair_off[0] == 0
    assert (t.n_frames, t.n_gt, t.n_dt, t.n_pairs) == (6, 5, 11, 16)
    assert t.gt_rows.shape == (5, 16) and t.dt_rows.shape == (11, 16) and t.gt_rows.dtype == np.float64
    g, d = gts[4], dts[4]
    r = t.gt_rows[3:5]
    for key, col in (("bbox", slice(0, 4)), ("alpha", 4), ("location", slice(5, 8)), ("dimensions", slice(8, 11)), ("rotation_y", 11),
                     ("occluded", 12), ("truncated", 13)):
        np.testing.assert_array_equal(r[:, col], g[key])
        np.testing.assert_array_equal(t.dt_rows[6:11][:, col], d[key])
    np.testing.assert_array_equal(t.dt_rows[6:11, 14], d["score"])
    assert (r[:, 14:] == 0).all() and (t.dt_rows[:, 15] == 0).all()
    empty = KD.AnnoTables([], [])
    assert list(empty.pair_off) == [0] and empty.gt_rows.shape == (0, 16) and empty.dt_box7.shape == (0, 7)


def test_float32_annotations_are_widened():
    g32, d32 = _anno(["Car", "Van", "DontCare"], np.float32), _anno(["Car", "Car"], np.float32, score=True)
    t = KD.AnnoTables([g32], [d32])
    assert t.gt_rows.dtype == t.dt_rows.dtype == np.float64
    np.testing.assert_array_equal(t.gt_rows[:, 8:11], g32["dimensions"].astype(np.float64))
    np.testing.assert_array_equal(t.dt_rows[:, 14], d32["score"].astype(np.float64))
    wide = lambda a: {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in a.items()}
    t64 = KD.AnnoTables([wide(g32)], [wide(d32)])
    for k in ("gt_rows", "dt_rows", "gt_box7", "dt_box7"):
        np.testing.assert_array_equal(getattr(t, k), getattr(t64, k))
    assert "incoming dtype" in KD.AnnoTables.__doc__ and "widened" in KD.AnnoTables.__doc__


def test_box7_rows_are_what_hip_rotated_intersection_builds(monkeypatch):
    import torch
    from hvpr_amd import kernels
    seen = []

    def capture(a, b, mode):
        seen.append((a.numpy().copy(), b.numpy().copy(), mode))
        return torch.zeros((a.shape[0], b.shape[0]))
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(kernels, "boxes_pairwise", capture)
    gts, dts = synthetic_kitti_annos(1212, 6)
    t = KD.AnnoTables(gts, dts)
    for dtype in (np.float64, np.float32):
        for f, (g, d) in enumerate(zip(gts, dts)):
            if not len(g["name"]) or not len(d["name"]):
                continue
            cast = lambda a: {k: (v.astype(dtype) if v.dtype == np.float64 else v) for k, v in a.items()}
            del seen[:]
            kitti_eval.frame_overlap(cast(g), cast(d), 1, kitti_eval.hip_rotated_intersection)
            (a7, b7, mode), = seen
            assert mode == 0 and a7.dtype == np.float32
            t_f = KD.AnnoTables([cast(g)], [cast(d)]) if dtype == np.float32 else None
            np.testing.assert_array_equal(a7, (t_f.dt_box7 if t_f else t.dt_box7[t.dt_off[f]:t.dt_off[f + 1]]))
            np.testing.assert_array_equal(b7, (t_f.gt_box7 if t_f else t.gt_box7[t.gt_off[f]:t.gt_off[f + 1]]))


def test_frames_over_the_limits_raise():
    ok_g, ok_d = _anno(["Car"] * 1024), _anno(["Car"] * 4096, score=True)
    KD.AnnoTables([ok_g], [ok_d])
    with pytest.raises(ValueError, match="4096 detections"):
        KD.AnnoTables([ok_g], [_anno(["Car"] * 4097, score=True)])
    with pytest.raises(ValueError, match="1024 ground truths"):
        KD.AnnoTables([_anno(["Car"] * 1025)], [ok_d])
    with pytest.raises(ValueError):
        KD.AnnoTables([ok_g], [])


# ------------------------------------------------------------------------------------------------ the counting pass's pick
def closed_form_pick(col, cand, dflag):
    """What csrc/kitti_ap.hip computes: among the candidates, the evaluated one (dflag 0) with the largest overlap, lowest index
    on ties; failing those the first ignored one (dflag 1); else -1.  Holds for candidates with a positive overlap."""
    js = np.nonzero(cand)[0]
    ev = js[dflag[js] == 0]
    if len(ev):
        return int(ev[np.argmax(col[ev])])
    ig = js[dflag[js] == 1]
    return int(ig[0]) if len(ig) else -1


def test_closed_form_pick_equals_the_scan():
    rng = np.random.default_rng(41)
    values = np.array([0.26, 0.5, 0.7, 0.93])
    n_match = n_ignored = n_ties = 0
    for _ in range(20000):
        n = int(rng.integers(1, 13))
        col = values[rng.integers(0, 4, n)]
        dflag = rng.choice([-1, 0, 1], n, p=[0.2, 0.45, 0.35])
        cand = rng.random(n) < 0.7
        score = rng.uniform(0, 1, n)
        want = kitti_eval._pick(col, cand, dflag, score, True)
        assert closed_form_pick(col, cand, dflag) == want, (col, cand, dflag)
        n_match += want >= 0
        n_ignored += want >= 0 and dflag[want] == 1
        ev = np.nonzero(cand & (dflag == 0))[0]
        n_ties += len(ev) > 1 and (col[ev] == col[ev].max()).sum() > 1
    assert n_match > 15000 and n_ignored > 1000 and n_ties > 3000       # the draw really covers the branches
    hand = [  # (col, dflag, expected): all candidates
        ([0.9, 0.6], [1, 0], 1),            # ignored first, then an evaluated one with the smaller overlap: the evaluated one
        ([0.9, 0.6, 0.8], [1, 0, 0], 2),
        ([0.7, 0.7], [0, 0], 0),            # two evaluated at equal overlap: the first
        ([0.5, 0.7, 0.7], [0, 0, 0], 1),
        ([0.6, 0.9], [1, 1], 0),            # only ignored: the first
        ([0.6, 0.9], [-1, 1], 1),
        ([0.6, 0.9], [-1, -1], -1),
        ([0.6, 0.9, 0.95], [0, 1, 1], 0),   # an ignored one never replaces an evaluated one
    ]
    for col, dflag, want in hand:
        col, dflag, cand = np.array(col), np.array(dflag), np.ones(len(col), bool)
        assert kitti_eval._pick(col, cand, dflag, np.zeros(len(col)), True) == want
        assert closed_form_pick(col, cand, dflag) == want


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope="module")
def L():
    from hvpr_amd import build, _lib
    build.build()
    return _lib.lib()


P = ctypes.c_void_p(0x1000)          # fake non-null device pointer: every call below must return before a launch


def test_ragged_pairwise_and_overlap_argument_checks(L):
    f = L.hvpr_boxes_pairwise_ragged_f32
    assert f(None, None, None, None, None, 0, 0, None, None) == OK
    assert f(P, P, P, P, P, 5, 0, P, None) == OK                       # frames without any pair
    assert f(P, P, P, P, P, -1, 10, P, None) == INVALID
    assert f(P, P, P, P, P, 5, -1, P, None) == INVALID
    for i in (0, 1, 2, 3, 4, 7):
        a = [P, P, P, P, P, 5, 10, P, None]
        a[i] = None
        assert f(*a) == INVALID, i
    g = L.hvpr_kitti_overlaps_f64
    assert g(None, None, None, None, None, None, 0, 0, 0, None, None) == OK
    assert g(P, P, P, P, P, P, 4, 0, 2, P, None) == OK
    assert g(P, P, P, P, P, P, -1, 10, 0, P, None) == INVALID
    assert g(P, P, P, P, P, P, 4, -1, 0, P, None) == INVALID
    assert g(P, P, P, P, P, P, 4, 10, 3, P, None) == INVALID
    assert g(P, P, P, P, P, P, 4, 10, -1, P, None) == INVALID
    assert g(P, P, None, P, P, P, 4, 10, 1, P, None) == INVALID           # BEV and 3-D need the intersections
    for i in (0, 1, 3, 4, 5, 9):
        a = [P, P, P, P, P, P, 4, 10, 2, P, None]
        a[i] = None
        assert g(*a) == INVALID, i


def _match(L, **kw):
    classes = kw.pop("classes", [0, 1, 2])
    mo = kw.pop("mo", [0.7, 0.5, 0.5, 0.5, 0.25, 0.25])
    a = dict(gt=P, gt_cls=P, gt_dc=P, dt=P, dt_cls=P, gt_off=P, dt_off=P, pair_off=P, F=24, NG=100, ov=P, metric=0, pas=1,
             classes=(ctypes.c_int32 * len(classes))(*classes) if classes is not None else None, C=len(classes or []),
             mo=(ctypes.c_double * len(mo))(*mo) if mo is not None else None, K=2, th=P, th_n=P, T=41, aos=1, tp_score=P, n_valid=P,
             counts=P, sim=P, ws=P, ws_bytes=None, stream=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.hvpr_kitti_match_workspace_bytes(max(a["F"], 0), max(a["C"], 0), max(a["K"], 0), max(a["T"], 0))
    return L.hvpr_kitti_match_f64(*a.values())


def test_match_argument_checks(L):
    q = L.hvpr_kitti_match_workspace_bytes
    assert q(0, 3, 2, 41) == q(24, 0, 2, 41) == q(24, 3, 0, 41) == q(24, 3, 2, 0) == 0
    assert q(24, 3, 2, 41) == 24 * 18 * 41 * 24 and q(3769, 3, 2, 41) == 3769 * 18 * 41 * 24
    for bad in (dict(F=-1), dict(NG=-1), dict(metric=3), dict(metric=-1), dict(pas=2), dict(pas=-1), dict(C=0), dict(C=9), dict(K=0),
                dict(K=5), dict(classes=None), dict(mo=None), dict(classes=[0, 6, 2]), dict(classes=[0, -1, 2]),
                dict(mo=[0.7, 0.5, -0.1, 0.5, 0.25, 0.25]), dict(mo=[0.7, 0.5, float("nan"), 0.5, 0.25, 0.25]),
                dict(T=0), dict(th=None), dict(th_n=None), dict(counts=None), dict(sim=None), dict(ws=None),
                dict(gt_off=None), dict(dt_off=None), dict(pair_off=None), dict(gt=None), dict(gt_cls=None), dict(gt_dc=None),
                dict(pas=0, n_valid=None), dict(pas=0, tp_score=None)):
        assert _match(L, **bad) == INVALID, bad
    assert _match(L, ws_bytes=q(24, 3, 2, 41) - 1) == WORKSPACE
    assert _match(L, ws_bytes=0) == WORKSPACE
    assert _match(L, F=1 << 30) == UNSUPPORTED                           # more waves than one grid holds


# ------------------------------------------------------------------------------------------------ the edge set
def _oracle_intersection(a5, b5):
    from oracle import hvpr_oracle as O

    def as7(b):
        t = np.zeros((len(b), 7), np.float32)
        t[:, 0:2], t[:, 3:5], t[:, 5], t[:, 6] = b[:, 0:2], b[:, 2:4], 1.0, -b[:, 4]
        return t
    if len(a5) == 0 or len(b5) == 0:
        return np.zeros((len(a5), len(b5)))
    return O.boxes_overlap_bev(as7(a5), as7(b5)).astype(np.float32).astype(np.float64)


def test_edge_set_holds_what_it_is_for():
    gts, dts = edge_set()
    assert len(gts) == len(dts) <= 8
    assert len(dts[0]["name"]) == 130 and len(gts[0]["name"]) == 3
    assert [len(g["name"]) for g in gts][6] == 0 and len(dts[6]["name"]) == 0 and len(dts[7]["name"]) == 0
    assert set(gts[4]["name"]) == {"DontCare"}
    assert "Cyclist" in set(dts[5]["name"]) and not any("Cyclist" in set(g["name"]) for g in gts)
    h = dts[2]["bbox"][:, 3] - dts[2]["bbox"][:, 1]
    assert (h == 40.0).any() and ((h < 40.0) & (h > 39.98)).sum() == 2
    assert {0.15, 0.3, 0.5} <= set(gts[2]["truncated"])
    mo = kitti_eval._OVERLAPS[:, :, [0, 1, 2]]
    for metric in (0, 1, 2):
        run = HostRun(gts, dts, [0, 1, 2], metric, mo, metric == 0, _oracle_intersection)
        n_th = np.array([len(t) for t in run.thresholds]).reshape(3, 3, 2)
        assert (n_th[0] > 0).all() and (n_th[1] > 0).all(), (metric, n_th)     # cars and pedestrians: thresholds at every difficulty
        assert (n_th[2] == 0).all() and (run.n_valid[2] == 0).all()            # cyclists: no ground truth, rows of zeros
        assert (run.result["precision"][2] == 0).all()
    # the pick crosses the chunks of 64 in frame 0: the exact copies win the counting pass, higher scores elsewhere the threshold pass
    ov = kitti_eval.frame_overlap(gts[0], dts[0], 0, None)
    _, gflag, dflag, _ = kitti_eval.clean_data(gts[0], dts[0], 0, 0)
    score = dts[0]["score"]
    hits = kitti_eval._match(ov, gflag, dflag, score, 0.7, 0.0, True)[2]
    assert sorted(j // 64 for _, j in hits) == [0, 1, 2], hits
    hits0 = kitti_eval._match(ov, gflag, dflag, score, 0.7, 0.0, False)[2]
    assert len({j // 64 for _, j in hits0}) > 1 and [j for _, j in hits0] != [j for _, j in hits]
    # frame 2, cars, easy: an ignored detection is matched (its ground truth neither a true positive nor a miss), and the ignored
    # detection with the larger overlap loses to the evaluated one behind it
    ov = kitti_eval.frame_overlap(gts[2], dts[2], 0, None)
    _, gflag, dflag, _ = kitti_eval.clean_data(gts[2], dts[2], 0, 0)
    tp, fn, hits, assigned, _ = kitti_eval._match(ov, gflag, dflag, dts[2]["score"], 0.7, 0.0, True)
    assert (assigned & (dflag == 1)).any() and (0, 1) in hits and ov[0, 0] > ov[1, 0] > 0.7 and dflag[0] == 1 and dflag[1] == 0
    # frame 1: equal overlap and equal score
    assert dts[1]["score"][0] == dts[1]["score"][1] and (dts[1]["bbox"][0] == dts[1]["bbox"][1]).all()
    # frame 3: DontCare regions take a false positive away, once, though two of them cover it
    ov = kitti_eval.frame_overlap(gts[3], dts[3], 0, None)
    _, gflag, dflag, dc = kitti_eval.clean_data(gts[3], dts[3], 0, 0)
    assert len(dc) == 2 and (kitti_eval.image_box_overlap(dts[3]["bbox"], dc, 0)[1] > 0.7).all()
    a = (ov, gts[3]["alpha"], dts[3]["alpha"], dts[3]["bbox"], gflag, dflag, dts[3]["score"])
    assert kitti_eval._frame_stats(*a, dc, 0, 0.7, 0.0, False)[1] == 1
    assert kitti_eval._frame_stats(*a, dc[:0], 0, 0.7, 0.0, False)[1] == 2
    g2, d2 = with_empty_ends(gts, dts)
    assert len(g2) == 10 and len(g2[0]["name"]) == len(d2[-1]["name"]) == 0
