"""CPU: the KITTI readers and get_infos' host part against fixture G23 (the reference's own get_infos on a canned tree, see
tests/golden/make_golden_kitti_infos.py); the numpy count of tests/kitti_infos_cases.py, the checker of the GPU tests, against
G23's num_points_in_gt; the C ABI of the count: bound, its workspace query needs no GPU, and every refusal is decided on the host
copies before anything is launched (so it is testable here)."""
import ctypes

import numpy as np
import pytest

import kitti_infos_cases as KC

NAMES = ["hvpr_kitti_infos_block_points", "hvpr_kitti_infos_workspace_bytes", "hvpr_kitti_infos_count_f32"]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
CFG = {"POINT_CLOUD_RANGE": [0, -40, -3, 70.4, 40, 1], "FOV_POINTS_ONLY": True}


@pytest.fixture(scope="module")
def L():
    from hvpr_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def z():
    return KC.g23()


@pytest.fixture(scope="module")
def root(z, tmp_path_factory):
    d = tmp_path_factory.mktemp("g23_tree")
    KC.write_tree(d, KC.g23_tree(z))
    return d


def _dataset(root, split):
    from hvpr_amd import kitti_dataset as KD
    ds = KD.KittiDataset(CFG, ["Car", "Pedestrian", "Cyclist"], training=False, root_path=root, device="cpu")
    ds.set_split(split)
    return ds


# ------------------------------------------------------------------------------------------------ the readers
def test_readers_on_the_tree(root):
    from hvpr_amd import kitti_dataset as KD
    calib = KD.read_calib(root / "training/calib/000001.txt")
    want = KC.make_calib(1)
    assert list(calib) == ["P2", "P3", "R0", "Tr_velo2cam"]
    for k in calib:
        assert calib[k].dtype == np.float32 and calib[k].tobytes() == want[k].tobytes(), k
    shape = KD.read_image_shape(root / "training/image_2/000001.png")
    assert shape.dtype == np.int32 and shape.tolist() == [370, 1224]
    with pytest.raises(ValueError):
        KD.read_image_shape(root / "training/calib/000001.txt")
    plane = KD.read_road_plane(root / "training/planes/000000.txt")
    assert plane.dtype == np.float64 and plane.shape == (4,) and plane[1] < 0 and abs(np.linalg.norm(plane[:3]) - 1) < 1e-15
    raw = np.array([-7.051e-03, -9.997e-01, -2.292e-02, 1.681e+00])
    assert np.array_equal(plane, raw / np.linalg.norm(raw[:3]))
    objs = KD.read_label(root / "training/label_2/000000.txt")
    assert [o["name"] for o in objs] == ["Car", "Pedestrian", "Cyclist", "Van", "DontCare", "DontCare"]
    assert objs[0]["score"] == 0.8765 and objs[1]["score"] == -1.0                       # a 16th field, and none
    assert objs[0]["bbox"].dtype == np.float32 and objs[0]["location"].dtype == np.float32
    assert KD.read_split(root, "train") == ["000000", "000001"] and KD.read_split(root, "nope") is None


def test_difficulty_rule_every_branch():
    from hvpr_amd.kitti_dataset import _level
    box = lambda h: np.array([0, 0, 10, h - 1], np.float32)          # height = y2 - y1 + 1
    assert _level(box(40), 0.15, 0) == 0 and _level(box(39.5), 0.15, 0) == 1 and _level(box(40), 0.16, 0) == 1
    assert _level(box(25), 0.3, 1) == 1 and _level(box(25), 0.31, 1) == 2 and _level(box(25), 0.3, 2) == 2
    assert _level(box(25), 0.5, 2) == 2 and _level(box(24.5), 0.0, 0) == -1 and _level(box(80), 0.51, 0) == -1
    assert _level(box(80), 0.0, 3) == -1


def _with_checker_counts(infos, z, split):
    """num_points_in_gt filled in by the numpy checker: what get_infos does with the device's counts."""
    for info, (pts, calib, shape) in zip(infos, KC.g23_frame_inputs(z, split)):
        a = info["annos"]
        n = a["gt_boxes_lidar"].shape[0]
        num = -np.ones(len(a["name"]), dtype=np.int32)
        num[:n] = KC.count_host(pts, a["gt_boxes_lidar"], calib, shape)[0]
        a["num_points_in_gt"] = num
    return infos


@pytest.mark.parametrize("split", ["train", "val"])
def test_get_infos_host_part_is_g23(root, z, split):
    """Parsed fields, dtypes, key order, index, difficulty and -(pi/2 + ry) bit for bit; the centres within 1e-4 m."""
    ds = _dataset(root, split)
    infos = ds.get_infos(has_label=True, count_inside_pts=False)
    assert all("num_points_in_gt" not in i["annos"] for i in infos) and ds.reads == 0
    want = KC.g23_infos(z, split)
    KC.assert_same_infos(_with_checker_counts(infos, z, split), want)
    for g, w in zip(infos, want):
        a = w["annos"]
        assert a["location"].dtype == np.float32 and a["dimensions"].dtype == np.float64 and a["gt_boxes_lidar"].dtype == np.float64
        assert a["num_points_in_gt"].dtype == np.int32 and a["index"].dtype == np.int32 and a["difficulty"].dtype == np.int32
        n = a["gt_boxes_lidar"].shape[0]
        assert g["annos"]["gt_boxes_lidar"][:, 6].tobytes() == (-(np.pi / 2 + a["rotation_y"][:n])).tobytes()
        assert a["index"].tolist() == list(range(n)) + [-1] * (len(a["name"]) - n)


def test_get_infos_without_labels_is_g23(root, z):
    infos = _dataset(root, "test").get_infos(has_label=False, count_inside_pts=False)
    KC.assert_same_infos(infos, KC.g23_infos(z, "test"))
    assert list(infos[0]) == ["point_cloud", "image", "calib"]
    assert infos[0]["calib"]["P2"].dtype == np.float64 and infos[0]["calib"]["R0_rect"].dtype == np.float32


def test_frame_is_getitem_before_the_fov_filter(root, z):
    """gt_boxes from the FLOAT32 camera boxes, DontCare dropped, road_plane only where the file is."""
    import pickle
    ds = _dataset(root, "train")
    ds.kitti_infos = KC.g23_infos(z, "train")
    assert len(ds) == 2
    f0, f1 = ds.frame(0), ds.frame(1)
    assert f0["frame_id"] == "000000" and list(f0["gt_names"]) == ["Car", "Pedestrian", "Cyclist", "Van"]
    assert "road_plane" in f0 and "road_plane" not in f1
    assert f0["image_shape"].tolist() == [375, 1242] and tuple(f0["points"].shape) == (2500, 4)
    for fr, info in ((f0, ds.kitti_infos[0]), (f1, ds.kitti_infos[1])):
        b, w = fr["gt_boxes"], info["annos"]["gt_boxes_lidar"]
        assert b.dtype == np.float32 and b.shape == w.shape
        assert np.abs(b[:, :3] - w[:, :3]).max() <= 1e-4                          # another rounding path, the same boxes
        assert np.array_equal(b[:, 3:6], w[:, 3:6].astype(np.float32))
        # ry rounded to float32 (|ry| <= pi: 2^-23) plus one float32 sum below 8 (2^-22)
        assert np.abs(b[:, 6] - w[:, 6]).max() <= 2.0 ** -21
    ds.kitti_infos = KC.g23_infos(z, "test")
    ds.set_split("test")
    ft = ds.frame(0)
    assert "gt_boxes" not in ft and ft["frame_id"] == "000004"
    assert ds.evaluation([], ["Car"]) == (None, {})
    pickle.dumps(f0["calib"])


# ------------------------------------------------------------------------------------------------ the checker against G23
def test_numpy_count_reproduces_g23(z):
    for split in ("train", "val"):
        for info, (pts, calib, shape) in zip(KC.g23_infos(z, split), KC.g23_frame_inputs(z, split)):
            a = info["annos"]
            n = a["gt_boxes_lidar"].shape[0]
            assert KC.margins_hold(pts, a["gt_boxes_lidar"], calib, shape)
            got, _ = KC.count_host(pts, a["gt_boxes_lidar"], calib, shape)
            assert got.tolist() == a["num_points_in_gt"][:n].tolist(), info["point_cloud"]["lidar_idx"]
            assert (a["num_points_in_gt"][n:] == -1).all()


def test_straddling_and_behind_boxes_differ_from_the_plain_count(z):
    info, (pts, calib, shape) = KC.g23_infos(z, "train")[1], KC.g23_frame_inputs(z, "train")[1]
    a = info["annos"]
    hull, plain = a["num_points_in_gt"][:3], KC.plain_count_host(pts, a["gt_boxes_lidar"])
    assert 0 < hull[0] < plain[0]                                                # the van across the image border
    assert hull[1] == plain[1] > 0                                               # the pedestrian, wholly in view
    assert hull[2] == 0 < plain[2]                                               # the car behind the camera
    assert KC.count_host(pts[7:8], a["gt_boxes_lidar"], calib, shape)[0].tolist() == [1, 1, 0]     # one point, two boxes


def test_generators_keep_the_margin_rule():
    blk = 256
    frames = KC.make_case([0, 1, blk - 1, 2 * blk + 1], [0, 1, 5, 64], seed=3)
    assert [len(f["points"]) for f in frames] == [0, 1, blk - 1, 2 * blk + 1]
    counts, fov = KC.counts_of(frames)
    assert [len(c) for c in counts] == [0, 1, 5, 64] and fov[0] == 0 and 0 < fov[3] < 2 * blk + 1
    fr, splits = KC.labelled_frames([300, 0, 257], [3, 2, 0], seed=4)
    assert [len(f["points"]) for f in fr] == [300, 0, 257] and splits["train"] == ["000400", "000401", "000402"]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_exported_and_bound(L):
    from hvpr_amd import _lib, kernels, kitti_dataset
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["hvpr_kitti_infos_count_f32"][1]) == 17
    assert callable(kernels.kitti_infos_count) and callable(kitti_dataset.create_kitti_infos)
    assert L.hvpr_abi_version() == _lib.ABI_VERSION == 8


def test_block_is_the_databases(L):
    assert L.hvpr_kitti_infos_block_points() == L.hvpr_gt_database_block_points()


def test_workspace_query_needs_no_gpu(L):
    ws, blk = L.hvpr_kitti_infos_workspace_bytes, L.hvpr_kitti_infos_block_points()
    assert ws(0, 1000, 5) == 0 and ws(-1, 10, 5) == 0 and ws(3, -1, 5) == 0 and ws(3, 10, -1) == 0
    assert ws(1, 0, 1) > 0 and ws(3, 1000, 0) > 0                               # the frames' own partial counts
    last = 0
    for n_obj in (0, 1, 64, 257, 4096):
        prev = 0
        for pts in (0, 1, blk - 1, blk, blk + 1, 2 * blk + 1, 120000):
            b = ws(4, pts, n_obj)
            assert b >= prev, (n_obj, pts)
            prev = b
        assert prev >= last
        last = prev
    assert ws(4, 120000, 4096) >= 4 * (4096 + 4) * ((120000 + blk - 1) // blk)     # per box and per frame a count per block


class _Call:
    """A well-formed call over host memory whose `device` pointers are never followed: every variation below is refused on the
    host copies, and a refused call launches nothing."""

    def __init__(self, L):
        self.L = L
        self.pt_off = np.array([0, 300, 300, 1000], np.int32)
        self.box_off = np.array([0, 2, 2, 5], np.int32)
        self.calib = np.zeros((3, 26), np.float32)
        self.calib[:, 24], self.calib[:, 25] = 375, 1242
        self.dummy = np.zeros((64,), np.float32)
        self.a = dict(points=self.dummy.ctypes.data, n_points=1000, F=4, pt_off_host=self.pt_off.ctypes.data, pt_off=self.dummy.ctypes.data,
                      B=3, boxes=self.dummy.ctypes.data, box_off_host=self.box_off.ctypes.data, box_off=self.dummy.ctypes.data, n_obj=5,
                      calib_host=self.calib.ctypes.data, calib=self.dummy.ctypes.data, obj_count=self.dummy.ctypes.data,
                      fov_count=self.dummy.ctypes.data, ws=self.dummy.ctypes.data, ws_bytes=0, stream=None)

    def __call__(self, **kw):
        a = dict(self.a, **kw)
        return self.L.hvpr_kitti_infos_count_f32(*[a[k] for k in self.a])


def test_every_refusal_is_made_on_the_host(L):
    c = _Call(L)
    need = L.hvpr_kitti_infos_workspace_bytes(3, 700, 5)
    assert need > 0 and c() == WORKSPACE and c(ws_bytes=need - 1) == WORKSPACE       # the well-formed call, short of workspace only
    for name in ("points", "pt_off_host", "pt_off", "boxes", "box_off_host", "box_off", "calib_host", "calib", "obj_count", "ws"):
        assert c(ws_bytes=need, **{name: None}) == INVALID, name
    assert c(B=0) == INVALID and c(n_obj=-1) == INVALID and c(n_points=-1) == INVALID
    assert c(F=2) == INVALID and c(F=9) == INVALID
    assert c(n_points=999) == INVALID and c(n_obj=4) == INVALID                     # the offsets' ends
    assert c(n_points=1 << 31) == UNSUPPORTED and c(B=65536) == UNSUPPORTED
    c.pt_off[:] = [0, 400, 300, 1000]
    assert c(ws_bytes=need) == INVALID                                             # falling offsets
    c.pt_off[:] = [1, 300, 300, 1000]
    assert c(ws_bytes=need) == INVALID
    c.pt_off[:] = [0, 300, 300, 1000]
    c.box_off[:] = [0, 3, 2, 5]
    assert c(ws_bytes=need) == INVALID
    c.box_off[:] = [0, 257, 257, 300]
    assert c(ws_bytes=1 << 30, n_obj=300) == UNSUPPORTED                           # 257 boxes in a frame
    c.box_off[:] = [0, 2, 2, 5]
    for col, bad in ((24, 0.0), (25, 0.0), (24, -1.0), (25, float("nan"))):
        c.calib[1, col] = bad
        assert c(ws_bytes=need) == INVALID, (col, bad)
        c.calib[1, col] = 375.0
    c.box_off[:] = [0, 0, 0, 0]
    assert c(n_obj=0, fov_count=None, boxes=None, obj_count=None, ws=None) == OK   # nothing to count: nothing launched
    assert c(n_obj=0, ws=None) == INVALID                                          # the frames' counts need the workspace
