"""CPU: the GT-sampling database's C ABI is there and bound, its workspace query needs no GPU, and the host form of
tests/gt_database_cases.py — the checker of the GPU tests — reproduces fixture G21, the reference's own
KittiDataset.create_groundtruth_database: records (keys, order, value types, values) and every file's bytes."""
import ctypes

import numpy as np
import pytest

import gt_database_cases as GC

NAMES = ["hvpr_gt_database_block_points", "hvpr_gt_database_workspace_bytes", "hvpr_gt_database_count_f32",
         "hvpr_gt_database_extract_f32"]


@pytest.fixture(scope="module")
def L():
    from hvpr_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def g21():
    z = GC.g21()
    infos, clouds, used, split = GC.g21_scene(z)
    want_infos, want_files = GC.g21_expected(z)
    return {"infos": infos, "clouds": clouds, "used": used, "split": split, "want_infos": want_infos, "want_files": want_files}


def test_symbols_exported_and_bound(L):
    from hvpr_amd import _lib, kernels
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["hvpr_gt_database_count_f32"][1]) == 14
    assert len(_lib.SIGNATURES["hvpr_gt_database_extract_f32"][1]) == 19
    for w in ("gt_database_block_points", "gt_database_count", "gt_database_extract"):
        assert callable(getattr(kernels, w))
    from hvpr_amd import gt_database
    from hvpr_amd.augment import ObjectBank
    assert callable(ObjectBank.from_device) and callable(gt_database.create_groundtruth_database)


def test_abi_version_is_still_8(L):
    from hvpr_amd import _lib
    assert L.hvpr_abi_version() == _lib.ABI_VERSION == 8


def test_block_points_needs_no_gpu(L):
    blk = L.hvpr_gt_database_block_points()
    assert blk >= 64 and blk % 64 == 0


def test_workspace_query_monotone_and_zero_for_empty(L):
    ws = L.hvpr_gt_database_workspace_bytes
    blk = L.hvpr_gt_database_block_points()
    assert ws(0, 1000, 5) == 0 and ws(3, 1000, 0) == 0 and ws(3, -1, 5) == 0 and ws(-1, 10, 5) == 0
    assert ws(1, 0, 1) > 0                                                   # boxes over an empty frame still get their counts
    last = 0
    for n_obj in (1, 2, 64, 257, 4096):
        prev = 0
        for pts in (0, 1, blk - 1, blk, blk + 1, 2 * blk + 1, 120000):
            b = ws(4, pts, n_obj)
            assert b >= prev, (n_obj, pts)
            prev = b
        assert prev >= last
        last = prev
    assert ws(4, 120000, 4096) >= 2 * 4 * 4096 * ((120000 + blk - 1) // blk)    # counts and their prefix, per box and block


def test_host_form_reproduces_g21(g21):
    infos, files, objects = GC.host_database(g21["infos"], lambda i: g21["clouds"][i].copy(), g21["used"], g21["split"])
    GC.assert_same_infos(infos, g21["want_infos"])
    assert sorted(files) == sorted(g21["want_files"])
    for p in files:
        assert files[p] == g21["want_files"][p], p
    assert len(objects) == 12 and sum(len(o) == 0 for o in objects) == 1
    assert "Van" not in infos and any("Van" in p for p in files)            # used_classes filters the records, not the files
    assert [r["num_points_in_gt"] for v in infos.values() for r in v] == [len(files[r["path"]]) // 16 for v in infos.values() for r in v]


def test_float32_centre_form_differs_from_g21(g21):
    """The move into the box frame is float32 minus FLOAT64, rounded once.  Rounding the centre first is a different function,
    and the fixture shows it."""
    _, files, _ = GC.host_database(g21["infos"], lambda i: g21["clouds"][i].copy(), g21["used"], g21["split"], centre_dtype=np.float32)
    differ = total = 0
    for p, want in g21["want_files"].items():
        assert len(files[p]) == len(want), p                                 # the same points ...
        a, b = np.frombuffer(files[p], np.float32).reshape(-1, 4), np.frombuffer(want, np.float32).reshape(-1, 4)
        assert a[:, 3].tobytes() == b[:, 3].tobytes(), p                     # ... the same features ...
        differ += int((a[:, :3] != b[:, :3]).sum())                          # ... other coordinates
        total += a[:, :3].size
    assert total > 0 and differ >= 1, (differ, total)


def test_generators_keep_the_margin_rule():
    infos, clouds = GC.make_case([0, 1, 255, 513], [0, 1, 5, 64], seed=3, trailing_dontcare=2)
    import augment_cases as AC
    assert [len(clouds[i["point_cloud"]["lidar_idx"]]) for i in infos] == [0, 1, 255, 513]
    for info in infos:
        pts, a = clouds[info["point_cloud"]["lidar_idx"]], info["annos"]
        assert len(a["name"]) >= a["gt_boxes_lidar"].shape[0]
        for b in a["gt_boxes_lidar"].astype(np.float32):
            if len(pts):
                assert AC.point_face_distance(pts, b)[0].min() >= GC.MARGIN
    infos, clouds, inside = GC.boundary_case()
    _, _, objects = GC.host_database(infos, lambda i: clouds[i].copy())
    assert (objects[0][:, 3] / 0.25).astype(int).tolist() == inside          # <= on the top and bottom faces, < on the sides
