"""CPU: the pieces the data path shares.  hvpr_amd.calibration against the reference's formulas (calibration_kitti.py:50-73,
restated here in numpy) and against itself across its three forms of the lidar-to-rect product; gt_database.chunk_layout; the
one create_logger.  No GPU and no pinned memory."""
import itertools
import logging
import types

import numpy as np
import pytest

import kitti_infos_cases as KC


def random_calib(seed):
    """A float32 calibration with nothing special about it: a perturbed rotation, a mount, a projection."""
    r = np.random.RandomState(seed)
    return {"Tr_velo2cam": np.concatenate([KC.V2C[:, :3] + r.normal(0, 0.05, (3, 3)), r.uniform(-1, 1, (3, 1))], axis=1).astype(np.float32),
            "R0": (np.eye(3) + r.normal(0, 0.02, (3, 3))).astype(np.float32),
            "P2": (KC.P2 + r.normal(0, 1.0, (3, 4))).astype(np.float32)}


CALIBS = [("fixture %d" % k, KC.make_calib(k)) for k in range(3)] + [("random %d" % s, random_calib(s)) for s in (1, 2, 3, 4)]


def ref_lidar_to_rect(V2C, R0, pts_lidar):
    """calibration_kitti.py:65-73 (cart_to_hom at :47)."""
    pts_lidar_hom = np.hstack((pts_lidar, np.ones((pts_lidar.shape[0], 1), dtype=np.float32)))
    return np.dot(pts_lidar_hom, np.dot(V2C.T, R0.T))


def ref_rect_to_lidar(V2C, R0, pts_rect):
    """calibration_kitti.py:50-63."""
    pts_rect_hom = np.hstack((pts_rect, np.ones((pts_rect.shape[0], 1), dtype=np.float32)))
    R0_ext = np.hstack((R0, np.zeros((3, 1), dtype=np.float32)))
    R0_ext = np.vstack((R0_ext, np.zeros((1, 4), dtype=np.float32)))
    R0_ext[3, 3] = 1
    V2C_ext = np.vstack((V2C, np.zeros((1, 4), dtype=np.float32)))
    V2C_ext[3, 3] = 1
    pts_lidar = np.dot(pts_rect_hom, np.linalg.inv(np.dot(R0_ext, V2C_ext).T))
    return pts_lidar[:, 0:3]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name,calib", CALIBS, ids=[n for n, _ in CALIBS])
def test_calibration_is_one_product_and_the_references_transforms(name, calib):
    from hvpr_amd import calibration, eval_loop, kitti_eval, preprocess
    assert eval_loop.pack_calib is calibration.pack_calib and eval_loop.CALIB_WORDS == calibration.CALIB_WORDS == 26
    assert preprocess.fov_matrices is calibration.fov_matrices
    V2C, R0, P2 = calib["Tr_velo2cam"], calib["R0"], calib["P2"]
    shape = (375, 1242)
    # the packed table, the FOV matrix and the shared product
    product = calibration.lidar_to_rect_matrix(V2C, R0)
    table = calibration.pack_calib([calib], [shape])
    a, p = calibration.fov_matrices(calib, "cpu")
    assert product.dtype == np.float32 and product.shape == (4, 3)
    assert table.dtype == np.float32 and table.shape == (1, 26)
    assert np.array_equal(table[:, :12].reshape(4, 3), product) and np.array_equal(a.numpy(), product)
    assert np.array_equal(table[0, 12:24].reshape(3, 4), P2) and np.array_equal(p.numpy(), P2.T) and table[0, 24:].tolist() == [375.0, 1242.0]
    # the point transforms, on float32 and on float64 points
    r = np.random.RandomState(5)
    for pts in (r.uniform(-40, 70, (33, 3)).astype(np.float32), r.uniform(-40, 70, (7, 3)), np.zeros((0, 3), np.float32)):
        assert same(calibration.lidar_to_rect(pts, calib), ref_lidar_to_rect(V2C, R0, pts)), name
        assert same(calibration.rect_to_lidar(pts, calib), ref_rect_to_lidar(V2C, R0, pts)), name
    # a dict and the reference's Calibration object are one calibration
    obj = types.SimpleNamespace(V2C=V2C, R0=R0, P2=P2)
    assert calibration.parts(obj)[0] is V2C and calibration.as_dict(calib) is calib and calibration.as_dict(None) is None
    back = calibration.as_dict(obj)
    assert list(back) == ["Tr_velo2cam", "R0", "P2"] and back["Tr_velo2cam"] is V2C and back["R0"] is R0 and back["P2"] is P2
    assert same(calibration.pack_calib([obj], [shape]), table)
    assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(calibration.fov_matrices(obj, "cpu"), (a, p)))
    pts = r.uniform(-40, 70, (9, 3)).astype(np.float32)
    assert same(calibration.lidar_to_rect(pts, obj), calibration.lidar_to_rect(pts, calib))
    assert same(calibration.rect_to_lidar(pts, obj), calibration.rect_to_lidar(pts, calib))
    # the packed table and the FOV matrices cast to float32; the transforms take the matrices as given
    c64 = {k: np.asarray(v, np.float64) for k, v in calib.items()}
    assert same(calibration.pack_calib([c64], [shape]), table) and np.array_equal(calibration.fov_matrices(c64, "cpu")[0].numpy(), product)
    assert same(calibration.lidar_to_rect(pts, c64), ref_lidar_to_rect(c64["Tr_velo2cam"], c64["R0"], pts))
    assert calibration.lidar_to_rect(pts, c64).dtype == np.float64
    assert same(calibration.rect_to_lidar(pts, c64), ref_rect_to_lidar(c64["Tr_velo2cam"], c64["R0"], pts))
    # kitti_eval casts its matrices to float32 first: float64 matrices give what their float32 casts give
    boxes = np.concatenate([r.uniform(0, 60, (6, 3)), r.uniform(1, 4, (6, 3)), r.uniform(-3, 3, (6, 1))], axis=1)
    cam64, cam32 = kitti_eval.boxes3d_lidar_to_kitti_camera(boxes, c64), kitti_eval.boxes3d_lidar_to_kitti_camera(boxes, calib)
    assert same(cam64, cam32)
    b = boxes.astype(np.float32)
    b[:, 2] -= b[:, 5] / 2
    assert np.array_equal(cam32[:, 0:3], ref_lidar_to_rect(V2C, R0, b[:, 0:3]))


SECTION_BYTES = {"pt_off": lambda B, M, N, F: 4 * (B + 1), "box_off": lambda B, M, N, F: 4 * (B + 1), "boxes": lambda B, M, N, F: 28 * M,
                 "centres": lambda B, M, N, F: 24 * M, "calib": lambda B, M, N, F: 4 * 26 * B, "points": lambda B, M, N, F: 4 * F * N}


@pytest.mark.parametrize("B,M,N", [(1, 0, 0), (1, 1, 1), (2, 3, 0), (3, 256, 1000)])
def test_chunk_layout(B, M, N):
    from hvpr_amd.gt_database import chunk_layout
    F = 4
    totals = {}
    for centres, calib, points in itertools.product((False, True), repeat=3):
        at, total = chunk_layout(B, M, N, F, centres=centres, calib=calib, points=points)
        asked = {"pt_off", "box_off", "boxes"} | ({"centres"} if centres else set()) | ({"calib"} if calib else set()) | \
            ({"points"} if points else set())
        assert set(at) == asked
        spans = sorted((o, o + SECTION_BYTES[k](B, M, N, F), k) for k, o in at.items())
        assert spans[0][0] == 0 and all(o % 256 == 0 for o, _, _ in spans)
        assert all(e0 <= o1 for (_, e0, _), (o1, _, _) in zip(spans, spans[1:])), spans          # ascending, nothing overlaps
        assert total == max((e + 255) // 256 * 256 for _, e, _ in spans), (total, spans)          # the end of the last section, aligned
        totals[centres, calib, points] = total
    # a section that was not asked for takes no bytes: each one adds exactly its own aligned size
    pad = lambda n: (n + 255) // 256 * 256
    for key, total in totals.items():
        want = 2 * pad(4 * (B + 1)) + pad(28 * M) + key[0] * pad(24 * M) + key[1] * pad(4 * 26 * B) + key[2] * pad(4 * F * N)
        assert total == want, (key, total, want)


def test_create_logger_twice_leaves_one_stream_handler(tmp_path):
    from hvpr_amd import demo, evaluate, train
    from hvpr_amd.common_utils import create_logger
    assert evaluate.create_logger is create_logger and train.create_logger is create_logger and demo.create_logger is create_logger
    a, b = create_logger(name="hvpr_amd.test_fold"), create_logger(name="hvpr_amd.test_fold")
    assert a is b and a.level == logging.INFO and not a.propagate
    streams = [h for h in a.handlers if type(h) is logging.StreamHandler]
    assert len(streams) == 1 and len(a.handlers) == 1
    assert streams[0].formatter._fmt == "%(asctime)s  %(levelname)5s  %(message)s"
    log = tmp_path / "log.txt"
    c = create_logger(log, 0, name="hvpr_amd.test_fold")
    assert c is create_logger(log, 0, name="hvpr_amd.test_fold") and c is not a
    assert sorted(type(h).__name__ for h in c.handlers) == ["FileHandler", "StreamHandler"]
    c.info("one line")
    assert "one line" in log.read_text()
    d = create_logger(tmp_path / "other.txt", 1, name="hvpr_amd.test_fold")                   # another rank: errors only, no file
    assert d.level == logging.ERROR and [type(h).__name__ for h in d.handlers] == ["StreamHandler"]
    for lg in (a, c, d):
        for h in list(lg.handlers):
            h.close()
            lg.removeHandler(h)
