"""GPU: get_infos' counts on the device (csrc/kitti_infos.hip), KittiDataset.get_infos and create_kitti_infos against the numpy
checker of tests/kitti_infos_cases.py (which test_kitti_infos_host.py pins to fixture G23, the reference's own get_infos, on the
CPU) and against G23 itself.  Counts are integers and compared exactly.

Every cloud keeps the margin rule of kitti_infos_cases (no point within 1e-3 m of a box face, 1e-3 px of an image border or
1e-3 m of depth 0; removed before any side sees the cloud), so the device's cosf, the reference's BLAS products and Qhull's
tolerance all decide as the checker does."""
import pickle

import numpy as np
import pytest

import batch_loader_cases as BC
import kitti_infos_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = ["Car", "Pedestrian", "Cyclist"]
CFG = {"POINT_CLOUD_RANGE": [0, -40, -3, 70.4, 40, 1], "FOV_POINTS_ONLY": True,
       "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                          {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}}]}


def blk_():
    from hvpr_amd import kernels
    return kernels.kitti_infos_block_points()


def chunk_of(frames, on_device=False):
    import torch
    from hvpr_amd import gt_database as GD
    pts = [torch.from_numpy(f["points"]).to(DEV) if on_device else f["points"] for f in frames]
    return GD.StagedChunk(pts, [f["boxes"] for f in frames], DEV, calibs=[f["calib"] for f in frames], image_shapes=[f["image_shape"] for f in frames])


def device_counts(frames, on_device=False):
    """-> (per frame the counts, per frame the points in view), one chunk, read here."""
    chunk = chunk_of(frames, on_device)
    obj, fov, _ = chunk.count(want_fov=True)
    obj, fov, off = obj.cpu().numpy(), fov.cpu().numpy(), chunk.box_off_host.numpy()
    return [obj[off[f]: off[f + 1]] for f in range(len(frames))], fov.tolist()


def assert_counts(frames, on_device=False):
    got, got_fov = device_counts(frames, on_device)
    want, want_fov = KC.counts_of(frames)
    assert got_fov == want_fov, (got_fov, want_fov)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.tolist() == w.tolist(), (f, g.tolist(), w.tolist())
    return want, want_fov


# ------------------------------------------------------------------------------------------------ the kernel
def test_frame_sizes_around_the_block():
    blk = blk_()
    sizes = [0, 1, blk - 1, blk, blk + 1, 2 * blk + 1]
    want, fov = assert_counts(KC.make_case(sizes, [3, 2, 5, 4, 6, 7], seed=11))
    assert sum(int(c.sum()) for c in want) > 0 and fov[0] == 0 and all(v <= n for v, n in zip(fov, sizes))


def test_frame_without_boxes_between_frames_with_boxes():
    want, fov = assert_counts(KC.make_case([700, 900, 600], [4, 0, 5], seed=12))
    assert len(want[1]) == 0 and fov[1] > 0 and int(want[0].sum()) > 0 and int(want[2].sum()) > 0


def test_only_frames_without_boxes_still_count_the_view():
    _, fov = assert_counts(KC.make_case([300, 0, 513], [0, 0, 0], seed=13))
    assert fov[0] > 0 and fov[1] == 0


def test_256_boxes_in_one_frame_and_257_refused():
    from hvpr_amd import kitti_dataset as KD
    frames = KC.make_case([1500, 400], [256, 3], seed=14)
    want, _ = assert_counts(frames)
    assert (want[0] > 0).sum() >= 8 and (want[0] == 0).sum() >= 8                 # boxes in view and boxes out of it
    big = KC.make_case([64], [257], seed=15)
    with pytest.raises(ValueError, match="256 boxes"):
        chunk_of(big)
    with pytest.raises(ValueError, match="256 boxes"):
        KD.InfoCounter(DEV).count([big[0]["points"]], [big[0]["boxes"]], [big[0]["calib"]], [big[0]["image_shape"]])


def test_wider_rows_and_resident_frames():
    """F = 5 takes the scalar loads, F = 4 the 16-byte ones; frames already on the device are not staged."""
    assert_counts(KC.make_case([600, 300], [4, 3], seed=16, F=5))
    assert_counts(KC.make_case([600, 300], [4, 3], seed=16, F=5), on_device=True)
    assert_counts(KC.make_case([600, 300], [4, 3], seed=17), on_device=True)


def test_calibrations_differ_inside_one_chunk():
    frames = KC.make_case([900, 900, 900], [6, 6, 6], seed=18)
    assert len({f["calib"]["P2"].tobytes() for f in frames}) == 3 and len({tuple(f["image_shape"]) for f in frames}) == 3
    _, fov = assert_counts(frames)
    # the case tells the calibrations apart: every frame under frame 0's calibration has another view
    same = [KC.count_host(f["points"], f["boxes"], frames[0]["calib"], frames[0]["image_shape"])[1] for f in frames]
    assert same[1] != fov[1] and same[2] != fov[2]


def test_fov_count_is_what_point_flags_flags():
    import torch
    from hvpr_amd import preprocess
    frames = KC.make_case([1000, 2 * blk_() + 1], [3, 3], seed=19)
    _, fov = device_counts(frames)
    for f, n in zip(frames, fov):
        flags = preprocess.get_fov_flag(torch.from_numpy(f["points"]).to(DEV), f["calib"], f["image_shape"])
        assert int(flags.to(torch.int64).sum().item()) == n


def test_two_calls_give_identical_bytes():
    frames = KC.make_case([1200, 700, 0, 900], [5, 0, 2, 9], seed=20)
    a, b = chunk_of(frames), chunk_of(frames)
    oa, fa, _ = a.count(want_fov=True)
    ob, fb, _ = b.count(want_fov=True)
    o2, f2, _ = a.count(want_fov=True)
    assert oa.cpu().numpy().tobytes() == ob.cpu().numpy().tobytes() == o2.cpu().numpy().tobytes()
    assert fa.cpu().numpy().tobytes() == fb.cpu().numpy().tobytes() == f2.cpu().numpy().tobytes()


def test_counts_without_the_view_counts_are_the_same():
    frames = KC.make_case([800, 500], [4, 3], seed=21)
    chunk = chunk_of(frames)
    obj, fov, _ = chunk.count()
    assert fov is None
    want, _ = KC.counts_of(frames)
    assert obj.cpu().numpy().tolist() == np.concatenate(want).tolist()


# ------------------------------------------------------------------------------------------------ get_infos
def test_five_frames_two_per_call_three_reads(tmp_path):
    from hvpr_amd import kitti_dataset as KD
    blk = blk_()
    frames, splits = KC.labelled_frames([900, blk + 1, 0, 2 * blk + 1, 700], [4, 3, 2, 0, 5], seed=22)
    KC.write_tree(tmp_path, KC.tree_files(frames, splits))
    ds = KD.KittiDataset(CFG, CLASSES, training=False, root_path=tmp_path, device=DEV)
    ds.set_split("train")
    infos = ds.get_infos(frames_per_call=2)
    assert ds.reads == 3 and len(infos) == 5
    for f, info in zip(frames, infos):
        a = info["annos"]
        n = a["gt_boxes_lidar"].shape[0]
        assert KC.margins_hold(f["points"], a["gt_boxes_lidar"], f["calib"], f["image_shape"])
        want, _ = KC.count_host(f["points"], a["gt_boxes_lidar"], f["calib"], f["image_shape"])
        assert a["num_points_in_gt"].dtype == np.int32 and a["num_points_in_gt"][:n].tolist() == want.tolist(), f["id"]
        assert (a["num_points_in_gt"][n:] == -1).all() and len(a["num_points_in_gt"]) == len(a["name"])
    assert sum(int(i["annos"]["num_points_in_gt"].clip(0).sum()) for i in infos) > 0
    one = ds.get_infos(frames_per_call=32)
    assert ds.reads == 4
    KC.assert_same_infos(one, infos, centre_tol=0.0)


def test_g23_straddling_behind_and_two_box_cases(tmp_path):
    from hvpr_amd import gt_database, kitti_dataset as KD
    z = KC.g23()
    KC.write_tree(tmp_path, KC.g23_tree(z))
    ds = KD.KittiDataset(CFG, CLASSES, training=False, root_path=tmp_path, device=DEV)
    ds.set_split("train")
    infos = ds.get_infos()
    KC.assert_same_infos(infos, KC.g23_infos(z, "train"))
    a = infos[1]["annos"]
    plain = gt_database.count_points_in_boxes([ds.get_lidar("000001")], [a["gt_boxes_lidar"]], device=DEV)[0]
    hull = a["num_points_in_gt"]
    assert 0 < hull[0] < plain[0] and hull[1] == plain[1] > 0 and hull[2] == 0 < plain[2]
    pts, calib, shape = KC.g23_frame_inputs(z, "train")[1]
    one = KD.InfoCounter(DEV).count([pts[7:8]], [a["gt_boxes_lidar"]], [calib], [shape])[0]
    assert one.tolist() == [1, 1, 0]                                             # one point inside two boxes


def test_create_kitti_infos_end_to_end(tmp_path):
    from hvpr_amd import kitti_dataset as KD
    from hvpr_amd.batch_loader import DeviceBatchLoader
    z = KC.g23()
    KC.write_tree(tmp_path, KC.g23_tree(z))
    KD.create_kitti_infos(CFG, CLASSES, tmp_path, tmp_path, device=DEV, frames_per_call=2)
    for split in ("train", "val", "trainval", "test"):
        with open(tmp_path / ("kitti_infos_%s.pkl" % split), "rb") as f:
            KC.assert_same_infos(pickle.load(f), KC.g23_infos(z, split))
    with open(tmp_path / "kitti_dbinfos_train.pkl", "rb") as f:
        db = pickle.load(f)
    want_train = KC.g23_infos(z, "train")
    assert sorted(db) == sorted({str(n) for i in want_train for n in i["annos"]["name"] if n != "DontCare"})
    assert sum(len(v) for v in db.values()) == sum(i["annos"]["gt_boxes_lidar"].shape[0] for i in want_train)
    assert all((tmp_path / r["path"]).exists() for v in db.values() for r in v)
    # the dataset serves the loader: the frames of the val split through the FOV filter and the range mask
    ds = KD.KittiDataset(CFG, CLASSES, training=False, root_path=tmp_path, device=DEV)
    assert ds.split == "val" and len(ds) == 2
    loader = DeviceBatchLoader(CFG, CLASSES, ds.frame, len(ds), training=False, device=DEV)
    batch = loader.prepare_batch([0, 1])
    got = np.diff(batch["point_frame_offsets"].cpu().numpy()).tolist()
    want = []
    for pts, calib, shape in KC.g23_frame_inputs(z, "val"):
        want.append(int((BC.fov_flag(pts, calib, shape) & BC.range_flag(pts, CFG["POINT_CLOUD_RANGE"])).sum()))
    assert got == want and min(want) > 0 and loader.reads == 1
    assert batch["frame_id"] == ["000002", "000003"] and tuple(batch["gt_boxes"].shape) == (2, 4, 8)
    # the ground truth served back as detections: the evaluator runs over the dataset's infos
    dets = []
    for info in ds.kitti_infos:
        n = info["annos"]["gt_boxes_lidar"].shape[0]
        d = {k: v[:n].copy() for k, v in info["annos"].items() if k not in ("gt_boxes_lidar", "num_points_in_gt", "index", "difficulty")}
        d["score"] = np.linspace(0.9, 0.5, n)
        dets.append(d)
    text, ap = ds.evaluation(dets, ["Car"])
    assert isinstance(text, str) and "Car_3d/moderate_R40" in ap
