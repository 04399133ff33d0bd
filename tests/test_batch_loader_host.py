"""CPU: the numpy restatement of the batch loader's whole path (tests/batch_loader_cases.py) reproduces fixture G22, the
reference's own __getitem__-after-the-FOV-filter + prepare_data + collate_batch on a canned scene
(tests/golden/make_golden_batch.py), and the workspace / tile queries of csrc/collate.hip need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_loader_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hvpr_ragged_select_tile_rows", "hvpr_ragged_select_workspace_bytes", "hvpr_ragged_select_count_f32",
               "hvpr_ragged_select_write_f32"]


@pytest.fixture(scope="module")
def z():
    return BC.g22()


@pytest.fixture(scope="module")
def restated(z):
    from hvpr_amd.augment import AugmentPlanner
    cfg = BC.g22_config(z)
    bank = BC.g22_bank(z, device="cpu")
    planner = AugmentPlanner(cfg["DATA_AUGMENTOR"], [str(c) for c in z["class_names"]], bank)
    gens = BC.g22_generators(z)
    points, gt, slots = BC.prepare_batch_host(BC.g22_frames(z), z["train.indices"].tolist(), planner, bank, gens, z["range"],
                                              int(z["num_frames"]))
    return points, gt, slots, gens


def test_scene_shows_what_it_is_there_for(z):
    items = [z[f"train.b{b}.items"].tolist() for b in range(4)]
    assert [len(i) for i in items[:3]] == [1, 1, 1] and len(items[3]) >= 2, "the last frame is redrawn"
    assert int(z["train.b1.boxes_before_trim"]) == 1 and int(z["train.b1.num_boxes"]) == 0, "every box of frame 1 falls to the trim"
    assert int(z["test.num_points"][2]) == 0 and int(z["train.b2.num_points"]) > 0, "frame 2 is empty after the FOV filter"
    assert z["train.gt_boxes"].shape[1] == max(int(z[f"train.b{b}.num_boxes"]) for b in range(4))
    assert len(np.unique(z["train.points"][:, [0, 4]], axis=0)) == len(z["train.points"]), "the feature column names a frame's points"


def test_restatement_reproduces_g22_train(z, restated, observed):
    points, gt, slots, gens = restated
    BC.assert_train_batch_is_g22(z, points, gt, observed)
    for b, s in enumerate(slots):
        k = f"train.b{b}."
        assert s["items"] == z[k + "items"].tolist(), ("frames served, redraw index", b)
        assert np.array_equal(s["perm"], z[k + "perm"]), ("permutation", b)
        assert BC.state_matches(gens[b], z, b), ("generator state after the frame", b)
        assert len(s["r"]["boxes"]) == int(z[k + "num_boxes"]) and len(s["points"]) == int(z[k + "num_points"])


def test_restatement_reproduces_g22_test_mode(z):
    points, gt = BC.test_batch_host(BC.g22_frames(z), z["train.indices"].tolist(), [str(c) for c in z["class_names"]], z["range"])
    assert points.tobytes() == z["test.points"].tobytes() and points.shape == z["test.points"].shape
    assert gt.tobytes() == z["test.gt_boxes"].tobytes() and gt.shape == z["test.gt_boxes"].shape
    assert np.diff(np.searchsorted(points[:, 0], np.arange(5))).tolist() == z["test.num_points"].tolist()


def test_workspace_and_tile_queries_need_no_gpu():
    from hvpr_amd import _lib
    L = _lib.lib()
    T = L.hvpr_ragged_select_tile_rows()
    assert T > 0 and T % 64 == 0
    q = L.hvpr_ragged_select_workspace_bytes

    def need(tiles, frames):            # per-tile counts, their prefix (one more), one partial count per offset: 256-byte slots
        up = lambda n: (4 * n + 255) // 256 * 256
        return up(tiles + 1) + up(tiles + 1) + up(frames + 1)

    for rows, tiles in ((0, 0), (1, 1), (T, 1), (T + 1, 2)):
        assert q(rows, 4) == need(tiles, 4), rows
    assert q(70 * T, 1024) == need(70, 1024)
    assert q(-1, 4) == 0 and q(10, 0) == 0


def test_new_symbols_in_header_bindings_and_exports():
    from hvpr_amd import _lib, build
    L = ctypes.CDLL(build.build())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvpr_amd.h")).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert _lib.ABI_VERSION == 8


def test_refusals_need_no_gpu():
    """Every check is made on the host, before any launch."""
    from hvpr_amd import _lib
    L, fake = _lib.lib(), ctypes.c_void_p(256)
    rxy = np.zeros((4,), np.float32)
    ok = dict(points=fake, rows=100, F=4, off=fake, B=2, mask=3, calib=fake, range_xy=rxy.ctypes.data, new_off=fake, ws=fake,
              ws_bytes=1 << 20)

    def count(**o):
        a = dict(ok)
        a.update(o)
        return L.hvpr_ragged_select_count_f32(*a.values(), None)

    assert count(rows=-1) == -1 and count(F=2) == -1 and count(B=0) == -1 and count(mask=4) == -1 and count(off=None) == -1
    assert count(calib=None) == -1 and count(range_xy=None) == -1 and count(new_off=None) == -1 and count(ws=None) == -1
    assert count(B=1025) == -2 and count(rows=2 ** 31 - 1) == -2
    assert count(ws_bytes=L.hvpr_ragged_select_workspace_bytes(100, 2) - 1) == -3


def test_unsupported_processor_is_named():
    from hvpr_amd.batch_loader import DeviceBatchLoader
    cfg = {"POINT_CLOUD_RANGE": [0, -40, -3, 70.4, 40, 1], "FOV_POINTS_ONLY": True,
           "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                              {"NAME": "sample_points", "NUM_POINTS": {"train": 16384, "test": 16384}}]}
    with pytest.raises(NotImplementedError, match="sample_points"):
        DeviceBatchLoader(cfg, ["Car"], lambda i: None, 1, training=False)
