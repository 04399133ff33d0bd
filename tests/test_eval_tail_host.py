"""CPU: the host side of the device evaluation epilogue (hvpr_amd/eval_loop.py, csrc/eval_tail.hip) — the argument checks of the two
entry points (answered before anything touches the device), the calibration table, the label map, and that the float64 formulas
the GPU tests measure against restate the reference's (fixture G20)."""
import ctypes
import types

import numpy as np
import pytest

from eval_tail_cases import FIELDS, G20, annos_f64
from hvpr_amd import eval_loop, preprocess

OK, INVALID, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(0x1000)          # fake non-null device pointer: every call below must return before a launch


@pytest.fixture(scope="module")
def L():
    from hvpr_amd import build, _lib
    build.build()
    return _lib.lib()


def _recall(L, **kw):
    thr = (ctypes.c_float * 9)(*[0.1 * i for i in range(1, 10)])
    a = dict(pred=P, count=P, B=2, Pn=64, gt=P, G=5, C=8, thr=thr, T=3, counts=P, best=P, stream=None)
    a.update(kw)
    return L.hvpr_recall_record_f32(*a.values())


def test_recall_record_argument_checks(L):
    assert _recall(L, T=9) == UNSUPPORTED
    assert _recall(L, B=1 << 16) == UNSUPPORTED
    for bad in (dict(B=-1), dict(Pn=-1), dict(G=-1), dict(T=-1), dict(C=6), dict(C=-8), dict(counts=None), dict(gt=None),
                dict(pred=None), dict(count=None), dict(thr=None)):
        assert _recall(L, **bad) == INVALID, bad
    assert _recall(L, B=0) == OK                                           # an empty batch: nothing to do, nothing launched
    assert _recall(L, B=0, counts=None, gt=None, pred=None, count=None) == OK


def _annos(L, **kw):
    cmap = (ctypes.c_int32 * 17)(*([0, 1, 2] + [-1] * 14))
    a = dict(boxes=P, scores=P, labels=P, count=P, B=2, Pn=64, calib=P, cmap=cmap, n_labels=3, row_base=P, cap=ctypes.c_longlong(1000),
             frame_base=4, max_frames=6, rows=P, cls=P, label=P, box7=P, lidar=P, off=P, overflow=P, stream=None)
    a.update(kw)
    return L.hvpr_prediction_annos_f32(*a.values())


def test_prediction_annos_argument_checks(L):
    assert _annos(L, n_labels=17) == UNSUPPORTED
    assert _annos(L, B=1 << 16, max_frames=1 << 20) == UNSUPPORTED
    assert _annos(L, cap=ctypes.c_longlong(1 << 31)) == UNSUPPORTED
    for bad in (dict(B=-1), dict(Pn=-1), dict(n_labels=-1), dict(cap=ctypes.c_longlong(-1)), dict(frame_base=-1), dict(max_frames=-1),
                dict(frame_base=5), dict(max_frames=5),                                  # the frames would run past dt_off
                dict(boxes=None), dict(scores=None), dict(labels=None), dict(count=None), dict(calib=None), dict(cmap=None),
                dict(row_base=None), dict(rows=None), dict(cls=None), dict(label=None), dict(box7=None), dict(lidar=None),
                dict(off=None), dict(overflow=None)):
        assert _annos(L, **bad) == INVALID, bad
    assert _annos(L, B=0) == OK
    assert _annos(L, B=0, frame_base=6) == OK


def test_calibration_table_is_the_reference_product():
    g = G20()
    table = eval_loop.pack_calib([g.calibs[c] for c in g.calib_of], g.image_shape)
    assert eval_loop.CALIB_WORDS == 26 and table.shape == (g.n_frames, 26) and table.dtype == np.float32
    for f in range(g.n_frames):
        a, p = preprocess.fov_matrices(g.calibs[g.calib_of[f]], "cpu")
        assert np.array_equal(table[f, 0:12].reshape(4, 3), a.numpy())
        assert np.array_equal(table[f, 12:24].reshape(3, 4).T, p.numpy())
        assert table[f, 24] == g.image_shape[f][0] and table[f, 25] == g.image_shape[f][1]
    c = g.calibs[0]
    obj = types.SimpleNamespace(V2C=c["Tr_velo2cam"], R0=c["R0"], P2=c["P2"])          # the reference's Calibration object
    assert np.array_equal(eval_loop.pack_calib([obj], [(375, 1242)]), eval_loop.pack_calib([c], [(375, 1242)]))
    assert not np.array_equal(table[0, :12], table[1, :12]) and (g.calibs[1]["R0"] == np.eye(3)).all()


def test_label_map_sends_other_names_to_minus_one():
    assert eval_loop.class_of_label(["Car", "Pedestrian", "Cyclist"]) == [0, 1, 2]
    assert eval_loop.class_of_label(["Cyclist", "Tram", "van", "Misc", "Person_sitting", "TRUCK", "DontCare"]) == [2, -1, 3, -1, 4, 5, -1]
    assert eval_loop.class_of_label([]) == []


def test_fixture_holds_the_scene_and_the_float64_formulas_restate_the_reference():
    g = G20()
    assert [len(g.pred(f)[0]) for f in range(6)] == [0, 1, 5, 12, 3, 7] and g.batch == 2
    assert len({tuple(s) for s in g.image_shape.tolist()}) == 2 and set(g.calib_of.tolist()) == {0, 1}
    assert {int(l) for f in range(6) for l in g.pred(f)[2]} == {1, 2, 3}
    clipped = 0
    for f in range(6):
        boxes, scores, labels = g.pred(f)
        ref, want = g.anno(f), annos_f64(boxes, g.calibs[g.calib_of[f]], g.image_shape[f])
        assert ref["name"].shape == (len(boxes),) and (ref["truncated"] == 0).all() and (ref["occluded"] == 0).all()
        if not len(boxes):
            continue
        assert list(ref["name"]) == [g.class_names[l - 1] for l in labels] and np.array_equal(ref["score"], scores)
        for k in FIELDS:
            if k != "score":
                scale = max(1.0, np.abs(want[k]).max())
                assert np.abs(ref[k] - want[k]).max() <= 4e-6 * scale, (f, k)           # float32 arithmetic, a few steps deep
        # the reference returns the array it lowered z of
        assert np.array_equal(ref["boxes_lidar"][:, 2], boxes[:, 2] - boxes[:, 5] / 2) and not np.array_equal(ref["boxes_lidar"][:, 2], boxes[:, 2])
        h, w = g.image_shape[f]
        clipped += int(((ref["bbox"][:, [0, 2]] == 0) | (ref["bbox"][:, [0, 2]] == w - 1)).sum() + ((ref["bbox"][:, [1, 3]] == 0) | (ref["bbox"][:, [1, 3]] == h - 1)).sum())
    assert clipped >= 8
    assert g.recall() == {"gt": 19, "rcnn_0.3": 11, "rcnn_0.5": 9, "rcnn_0.7": 7, "roi_0.3": 0, "roi_0.5": 0, "roi_0.7": 0}
    assert sum(g.recall(b)["gt"] for b in range(3)) == 19


def test_result_files_have_the_kitti_columns(tmp_path):
    g = G20()
    annos = [dict(g.anno(f), frame_id=g.frame_id[f]) for f in range(g.n_frames)]
    eval_loop.write_kitti_txt(annos, tmp_path)
    for f, a in enumerate(annos):
        lines = (tmp_path / (g.frame_id[f] + ".txt")).read_text().splitlines()
        assert len(lines) == len(a["name"])
        for i, line in enumerate(lines):
            w = line.split(" ")
            assert w[:3] == [str(a["name"][i]), "-1", "-1"] and len(w) == 16
            want = [a["alpha"][i], *a["bbox"][i], a["dimensions"][i][1], a["dimensions"][i][2], a["dimensions"][i][0], *a["location"][i],
                    a["rotation_y"][i], a["score"][i]]                               # kitti_dataset.py:313-318: dimensions as h w l
            assert w[3:] == ["%.4f" % v for v in want]
