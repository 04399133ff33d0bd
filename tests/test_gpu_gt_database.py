"""GPU: the GT-sampling database kernels (csrc/gt_database.hip), DatabaseBuilder and create_groundtruth_database against the
host form of tests/gt_database_cases.py (which test_gt_database_host.py pins to fixture G21, the reference's own method, on the
CPU) and against G21 itself.  Everything is compared bit for bit: counts, offsets, arena rows and their order, records, files.

Every general-heading case keeps the margin rule of gt_database_cases (no point within 1e-3 m of a box face, removed before
either side sees the cloud), so the device's cosf and glibc's decide inside / outside alike; the exact-boundary case uses
heading 0 and dyadic numbers.  The arena's values are then exact functions of the inputs on both sides: float32 minus float64
rounded once, and copies."""
import json

import numpy as np
import pytest

import gt_database_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.5
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def torch_():
    import torch
    return torch


def blk_():
    from hvpr_amd import kernels
    return kernels.gt_database_block_points()


def lidar(clouds):
    return lambda idx: clouds[idx].copy()


# ------------------------------------------------------------------------------------------------ the library, called raw
def raw_inputs(infos, clouds, F=4):
    """A chunk's arrays as the entry points take them (host offsets, device everything)."""
    torch = torch_()
    pts = [clouds[i["point_cloud"]["lidar_idx"]] for i in infos]
    boxes = [i["annos"]["gt_boxes_lidar"] for i in infos]
    b64 = np.concatenate([b.reshape(-1, 7) for b in boxes]) if boxes else np.zeros((0, 7))
    inp = {"F": F, "B": len(infos), "n_obj": len(b64),
           "pt_off_host": torch.from_numpy(np.cumsum([0] + [len(p) for p in pts]).astype(np.int32)),
           "box_off_host": torch.from_numpy(np.cumsum([0] + [len(b) for b in boxes]).astype(np.int32)),
           "points": torch.from_numpy(np.ascontiguousarray(np.concatenate(pts).reshape(-1, F), np.float32)).to(DEV),
           "boxes": torch.from_numpy(b64.astype(np.float32)).to(DEV),
           "centres": torch.from_numpy(np.ascontiguousarray(b64[:, :3])).to(DEV)}
    inp["pt_off"], inp["box_off"] = inp["pt_off_host"].to(DEV), inp["box_off_host"].to(DEV)
    return inp


def count_args(inp, counts, ws):
    torch = torch_()
    return [("points", inp["points"].data_ptr()), ("n_points", inp["points"].shape[0]), ("F", inp["F"]),
            ("pt_off_host", inp["pt_off_host"].data_ptr()), ("pt_off", inp["pt_off"].data_ptr()), ("B", inp["B"]),
            ("boxes", inp["boxes"].data_ptr()), ("box_off_host", inp["box_off_host"].data_ptr()), ("box_off", inp["box_off"].data_ptr()),
            ("n_obj", inp["n_obj"]), ("obj_count", counts.data_ptr()), ("ws", ws.data_ptr()), ("ws_bytes", ws.numel()),
            ("stream", torch.cuda.current_stream().cuda_stream)]


def extract_args(inp, counts_host, counts, obj_off, arena, ws):
    a = count_args(inp, counts, ws)
    return a[:9] + [("centres", inp["centres"].data_ptr()), a[9], ("obj_count_host", counts_host.data_ptr()), a[10],
                    ("obj_off", obj_off.data_ptr()), ("arena", arena.data_ptr()), ("capacity", arena.shape[0])] + a[11:]


def call(name, args, **override):
    from hvpr_amd import _lib
    unknown = set(override) - {k for k, _ in args}
    assert not unknown, unknown
    return getattr(_lib.lib(), name)(*[override.get(k, v) for k, v in args])


def workspace(inp):
    from hvpr_amd import _lib
    torch = torch_()
    off = inp["pt_off_host"].numpy()
    need = _lib.lib().hvpr_gt_database_workspace_bytes(inp["B"], int(np.diff(off).max()) if inp["B"] else 0, inp["n_obj"])
    return torch.zeros((max(int(need), 256),), dtype=torch.uint8, device=DEV)


def raw_run(infos, clouds, F=4, slack=3):
    """count, the host read, extract into an arena with `slack` spare rows -> counts, obj_off, arena rows, the spare rows."""
    torch = torch_()
    inp, = (raw_inputs(infos, clouds, F),)
    ws = workspace(inp)
    counts = torch.full((max(inp["n_obj"], 1),), -3, dtype=torch.int32, device=DEV)
    assert call("hvpr_gt_database_count_f32", count_args(inp, counts, ws)) == 0
    counts_host = counts.cpu()
    rows = int(counts_host[: inp["n_obj"]].sum())
    arena = torch.full((rows + slack, F), SENTINEL, dtype=torch.float32, device=DEV)
    obj_off = torch.full((inp["n_obj"] + 2,), -5, dtype=torch.int32, device=DEV)
    assert call("hvpr_gt_database_extract_f32", extract_args(inp, counts_host, counts, obj_off, arena, ws)) == 0
    torch.cuda.synchronize()
    a = arena.cpu().numpy()
    return {"counts": counts_host.numpy()[: inp["n_obj"]], "obj_off": obj_off.cpu().numpy(), "arena": a[:rows], "spare": a[rows:]}


def check_raw(got, objects):
    """Against the host form's objects: counts, offsets (and the word after them untouched), every row, the spare rows untouched."""
    want_n = [len(o) for o in objects]
    assert got["counts"].tolist() == want_n
    assert got["obj_off"][:-1].tolist() == np.cumsum([0] + want_n).tolist() and got["obj_off"][-1] == -5
    want = np.concatenate(objects) if objects else np.zeros((0, got["arena"].shape[1]), np.float32)
    assert got["arena"].shape == want.shape
    assert got["arena"].tobytes() == want.tobytes()
    assert (got["spare"] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ shared cases
@pytest.fixture(scope="module")
def block_case():
    """Frames of 0, 1, blk - 1, blk, blk + 1 and 2 blk + 1 points."""
    blk = blk_()
    infos, clouds = GC.make_case([0, 1, blk - 1, blk, blk + 1, 2 * blk + 1], [3, 2, 4, 5, 3, 6], seed=1, trailing_dontcare=1)
    return infos, clouds, GC.host_database(infos, lidar(clouds))


@pytest.fixture(scope="module")
def box_case():
    """Frames of 0, 1, 63, 64, 65 and 256 boxes."""
    infos, clouds = GC.make_case([300, 200, 1200, 1200, 1200, 4000], [0, 1, 63, 64, 65, 256], seed=2)
    return infos, clouds, GC.host_database(infos, lidar(clouds))


def test_frame_sizes_around_the_block(block_case):
    infos, clouds, (_, _, objects) = block_case
    assert sum(len(o) for o in objects) > 100 and any(len(o) == 0 for o in objects)
    check_raw(raw_run(infos, clouds), objects)


def test_box_counts_up_to_the_limit(box_case):
    infos, clouds, (_, _, objects) = box_case
    assert len(objects) == 0 + 1 + 63 + 64 + 65 + 256 and sum(len(o) > 0 for o in objects) > 350
    check_raw(raw_run(infos, clouds), objects)


def test_257_boxes_refused_and_nothing_touched():
    torch = torch_()
    names, boxes = GC.grid_boxes(257, seed=9, per_row=20)
    infos = [GC.make_info("000001", names[:3], boxes[:3]), GC.make_info("000002", names, boxes)]
    clouds = {"000001": GC.frame_points(40, boxes[:3], 91), "000002": GC.frame_points(40, boxes[:3], 92)}
    inp = raw_inputs(infos, clouds)
    ws = workspace(inp)
    counts = torch.full((260,), -3, dtype=torch.int32, device=DEV)
    assert call("hvpr_gt_database_count_f32", count_args(inp, counts, ws)) == UNSUPPORTED
    arena = torch.full((64, 4), SENTINEL, dtype=torch.float32, device=DEV)
    obj_off = torch.full((262,), -5, dtype=torch.int32, device=DEV)
    zeros = torch.zeros((260,), dtype=torch.int32)
    assert call("hvpr_gt_database_extract_f32", extract_args(inp, zeros, counts, obj_off, arena, ws)) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (counts == -3).all() and (obj_off == -5).all() and (arena == SENTINEL).all() and not ws.any()
    from hvpr_amd.gt_database import DatabaseBuilder
    with pytest.raises(ValueError, match="256 boxes"):
        DatabaseBuilder().add_frames(infos, lidar(clouds))


def three_block_case():
    """One frame of 3 blk points; box 1 holds the end of block 0, all of block 1 and the start of block 2, nothing else."""
    blk = blk_()
    names, boxes = GC.grid_boxes(3, seed=4)
    n = 3 * blk
    pts = GC.frame_points(n, boxes, 41)
    inside = np.arange(blk - 3, 2 * blk + 4)
    b = boxes[1]
    r = np.random.RandomState(42)
    l = r.uniform(-0.4, 0.4, (len(inside), 3)) * b[3:6]
    c, s = np.cos(b[6]), np.sin(b[6])
    pts[inside, :3] = np.stack([l[:, 0] * c - l[:, 1] * s + b[0], l[:, 0] * s + l[:, 1] * c + b[1], l[:, 2] + b[2]], axis=1)
    keep = np.setdiff1d(np.arange(n), inside)
    also_in = GC.AC.point_face_distance(pts[keep], b.astype(np.float32))[1]
    pts[keep[also_in], 2] += 40.0
    pts[:, 3] = np.arange(n) / 1024.0                                        # a point's feature names its place in the frame
    assert len(GC.clean_points(pts, boxes)) == n
    return [GC.make_info("000300", names, boxes)], {"000300": pts}, inside


def test_object_over_three_blocks_keeps_the_frame_order():
    infos, clouds, inside = three_block_case()
    _, _, objects = GC.host_database(infos, lidar(clouds))
    got = raw_run(infos, clouds)
    check_raw(got, objects)
    o = got["obj_off"]
    assert (got["arena"][o[1]: o[2], 3] * 1024).astype(int).tolist() == inside.tolist()


def overlap_case():
    """Boxes A, an empty one, B inside A, C, an empty one: some points lie in A and B both."""
    _, g = GC.grid_boxes(5, seed=6)
    g[1, :2] += [0.0, 400.0]
    g[4, :2] += [400.0, 0.0]
    g[0, 3:6], g[2, 0:3], g[2, 3:6] = GC.SIZES["Van"], g[0, 0:3] + [0.2, -0.1, 0.02], GC.PED
    names = ["Van", "Car", "Pedestrian", "Cyclist", "Car"]
    pts = GC.frame_points(900, g[[0, 2, 3]], 61)
    return [GC.make_info("000600", names, g, trailing_dontcare=2)], {"000600": pts}


def test_point_in_two_boxes_and_empty_objects():
    infos, clouds = overlap_case()
    _, _, objects = GC.host_database(infos, lidar(clouds))
    n = [len(o) for o in objects]
    assert n[1] == 0 and n[4] == 0 and n[0] > n[2] > 0 and n[3] > 0          # an empty object in the middle and one at the end
    in_a = {round(float(v), 6) for v in objects[0][:, 3]}
    assert all(round(float(v), 6) in in_a for v in objects[2][:, 3])         # every point of B is one of A's too
    check_raw(raw_run(infos, clouds), objects)


@pytest.mark.parametrize("F", [4, 5])
def test_feature_widths(F):
    blk = blk_()
    infos, clouds = GC.make_case([blk + 9, 77], [4, 3], seed=10 + F, F=F)
    _, _, objects = GC.host_database(infos, lidar(clouds))
    assert objects[0].shape[1] == F and sum(len(o) for o in objects) > 20
    check_raw(raw_run(infos, clouds, F=F), objects)


def test_exact_faces():
    """|z - cz| == dz/2 is inside, |x| == dx/2 and |y| == dy/2 are outside; heading 0, dyadic numbers."""
    infos, clouds, inside = GC.boundary_case()
    got = raw_run(infos, clouds)
    assert (got["arena"][:, 3] / 0.25).astype(int).tolist() == inside
    _, _, objects = GC.host_database(infos, lidar(clouds))
    check_raw(got, objects)


# ------------------------------------------------------------------------------------------------ the builder
def built(infos, clouds, **kw):
    from hvpr_amd.gt_database import DatabaseBuilder
    b = DatabaseBuilder(**kw).add_frames(infos, lidar(clouds))
    torch_().cuda.synchronize()
    return b, b.arena().cpu().numpy().tobytes(), [(s, n) for _, _, s, n in b.objects]


def test_frames_alone_and_together_and_chunk_sizes_agree(block_case):
    infos, clouds, (want_infos, _, objects) = block_case
    want = np.concatenate(objects).tobytes()
    _, whole, seg = built(infos, clouds)
    assert whole == want and [n for _, n in seg] == [len(o) for o in objects]
    alone = b"".join(built([i], clouds)[1] for i in infos)
    assert alone == want
    b1, one, seg1 = built(infos, clouds, frames_per_call=1)
    b4, four, seg4 = built(infos, clouds, frames_per_call=4)
    assert one == want and four == want and seg1 == seg and seg4 == seg
    GC.assert_same_infos(b4.db_infos(), want_infos)


def test_second_run_gives_the_same_bytes(box_case):
    infos, clouds, (_, _, objects) = box_case
    a, b = raw_run(infos, clouds), raw_run(infos, clouds)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert built(infos, clouds)[1] == built(infos, clouds)[1] == np.concatenate(objects).tobytes()


def test_count_only_mode(block_case):
    from hvpr_amd.gt_database import count_points_in_boxes
    infos, clouds, (_, _, objects) = block_case
    torch = torch_()
    pts = [clouds[i["point_cloud"]["lidar_idx"]] for i in infos]
    boxes = [i["annos"]["gt_boxes_lidar"] for i in infos]
    want, k = [], 0
    for b in boxes:
        want.append([len(o) for o in objects[k: k + len(b)]])
        k += len(b)
    got = count_points_in_boxes(pts, boxes, DEV, frames_per_call=4)
    assert [g.tolist() for g in got] == want and all(g.dtype == np.int32 for g in got)
    got = count_points_in_boxes([torch.from_numpy(p).to(DEV) for p in pts], boxes, DEV)          # frames already on the device
    assert [g.tolist() for g in got] == want


def test_refusals_leave_the_outputs_alone(block_case):
    torch = torch_()
    infos, clouds, (_, _, objects) = block_case
    inp = raw_inputs(infos, clouds)
    ws = workspace(inp)
    counts = torch.full((inp["n_obj"],), -3, dtype=torch.int32, device=DEV)
    bad_off = inp["pt_off_host"].clone()
    bad_off[2], bad_off[3] = int(inp["pt_off_host"][3]), int(inp["pt_off_host"][2])             # not ascending
    bad_box = inp["box_off_host"].clone()
    bad_box[1], bad_box[2] = int(inp["box_off_host"][2]), int(inp["box_off_host"][1])
    ca = count_args(inp, counts, ws)
    for over in ({"points": None}, {"pt_off_host": None}, {"pt_off": None}, {"boxes": None}, {"box_off_host": None}, {"box_off": None},
                 {"obj_count": None}, {"ws": None}, {"pt_off_host": bad_off.data_ptr()}, {"box_off_host": bad_box.data_ptr()},
                 {"F": 2}, {"F": 9}, {"n_points": inp["points"].shape[0] - 1}, {"n_obj": inp["n_obj"] + 1}):
        assert call("hvpr_gt_database_count_f32", ca, **over) == INVALID, over
    assert call("hvpr_gt_database_count_f32", ca, ws_bytes=ws.numel() // 2) == WORKSPACE
    torch.cuda.synchronize()
    assert (counts == -3).all() and not ws.any()

    assert call("hvpr_gt_database_count_f32", ca) == 0
    counts_host = counts.cpu()
    rows = int(counts_host.sum())
    assert rows == sum(len(o) for o in objects) > 0
    arena = torch.full((rows, 4), SENTINEL, dtype=torch.float32, device=DEV)
    obj_off = torch.full((inp["n_obj"] + 1,), -5, dtype=torch.int32, device=DEV)
    ea = extract_args(inp, counts_host, counts, obj_off, arena, ws)
    more = counts_host.clone()
    more[0] = int(inp["pt_off_host"][1] - inp["pt_off_host"][0]) + 1                             # more points than its frame has
    for over in ({"points": None}, {"pt_off_host": None}, {"pt_off": None}, {"boxes": None}, {"box_off_host": None}, {"box_off": None},
                 {"centres": None}, {"obj_count_host": None}, {"obj_count": None}, {"obj_off": None}, {"arena": None}, {"ws": None},
                 {"pt_off_host": bad_off.data_ptr()}, {"box_off_host": bad_box.data_ptr()}, {"obj_count_host": more.data_ptr()},
                 {"capacity": rows - 1}, {"capacity": -1}):                                      # one row short
        assert call("hvpr_gt_database_extract_f32", ea, **over) == INVALID, over
    assert call("hvpr_gt_database_extract_f32", ea, ws_bytes=ws.numel() // 2) == WORKSPACE
    torch.cuda.synchronize()
    assert (arena == SENTINEL).all() and (obj_off == -5).all()
    assert call("hvpr_gt_database_extract_f32", ea) == 0                                         # and the same call, unspoilt, goes through
    torch.cuda.synchronize()
    assert arena.cpu().numpy().tobytes() == np.concatenate(objects).tobytes()


# ------------------------------------------------------------------------------------------------ G21, files, banks
def read_tree(root, dirname="gt_database"):
    return {f"{dirname}/{p.name}": p.read_bytes() for p in (root / dirname).iterdir()}


def test_g21_on_the_device(tmp_path):
    import pickle
    from hvpr_amd.gt_database import create_groundtruth_database
    z = GC.g21()
    infos, clouds, used, split = GC.g21_scene(z)
    want_infos, want_files = GC.g21_expected(z)
    builder = create_groundtruth_database(tmp_path, infos, lidar(clouds), used_classes=used, split=split)
    GC.assert_same_infos(builder.db_infos(), want_infos)
    with open(tmp_path / ("kitti_dbinfos_%s.pkl" % split), "rb") as f:
        GC.assert_same_infos(pickle.load(f), want_infos)
    got = read_tree(tmp_path)
    assert sorted(got) == sorted(want_files)
    for p in got:
        assert got[p] == want_files[p], p
    assert sum(len(v) == 0 for v in got.values()) == 1                       # the empty object: a zero-byte file


PREPARE = {"filter_by_min_points": ["Car:5", "Pedestrian:3", "Cyclist:3"], "filter_by_difficulty": [-1]}
CLASSES = ["Car", "Pedestrian", "Cyclist"]


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """A database of 6 frames, built once: the builder and the directory it wrote (info file given by path, split 'val')."""
    import pickle
    from hvpr_amd.gt_database import create_groundtruth_database
    root = tmp_path_factory.mktemp("gtdb")
    infos, clouds = GC.make_case([900, 1300, 700, 1100, 1000, 1200], [8, 12, 6, 10, 9, 11], seed=7, trailing_dontcare=1)
    with open(root / "kitti_infos_val.pkl", "wb") as f:
        pickle.dump(infos, f)
    builder = create_groundtruth_database(root, root / "kitti_infos_val.pkl", lidar(clouds), split="val", frames_per_call=4)
    return root, builder, infos, clouds


@pytest.mark.parametrize("prepare", [None, PREPARE])
def test_round_trip_through_the_files(written, prepare):
    from hvpr_amd.augment import ObjectBank
    root, builder, infos, clouds = written
    want_infos, want_files, _ = GC.host_database(infos, lidar(clouds), split="val")
    assert read_tree(root, "gt_database_val") == want_files
    loaded = ObjectBank.from_db_info_files(root, ["kitti_dbinfos_val.pkl"], CLASSES, prepare=prepare, device=DEV)
    direct = builder.object_bank(CLASSES, prepare=prepare)
    n_all = sum(len(want_infos[c]) for c in CLASSES)
    assert len(loaded) == len(direct) and (0 < len(direct) < n_all if prepare else len(direct) == n_all)
    assert list(direct.class_ids) == list(loaded.class_ids)
    for c in CLASSES:
        assert np.array_equal(direct.class_ids[c], loaded.class_ids[c]) and direct.class_ids[c].dtype == loaded.class_ids[c].dtype
    assert direct.obj_box.dtype == loaded.obj_box.dtype and direct.obj_box.tobytes() == loaded.obj_box.tobytes()
    (da, db), (la, lb) = direct.on_device(), loaded.on_device()
    assert da.dtype == la.dtype and da.shape == la.shape and da.cpu().numpy().tobytes() == la.cpu().numpy().tobytes()
    assert db.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
    (dh, doff), (lh, loff) = direct.host_points(), loaded.host_points()
    assert dh.dtype == lh.dtype and dh.tobytes() == lh.tobytes() and lh.shape[0] > 0
    assert doff.dtype == loff.dtype and np.array_equal(doff, loff)


def test_augmented_batch_from_either_bank_is_the_same(written):
    """One DeviceAugmentor batch with a fixed seed, planned against the device-built bank and against the file-loaded one."""
    torch = torch_()
    from hvpr_amd.augment import DeviceAugmentor, ObjectBank
    root, builder, infos, clouds = written
    cfg = {"AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": ["kitti_dbinfos_val.pkl"], "PREPARE": PREPARE,
         "SAMPLE_GROUPS": ["Car:6", "Pedestrian:4", "Cyclist:4"], "NUM_POINT_FEATURES": 4, "DATABASE_WITH_FAKELIDAR": False,
         "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": False},
        {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
        {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
        {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]}
    rng6 = np.array([0, -60, -3, 120, 80, 1], np.float32)
    banks = [builder.object_bank(CLASSES, prepare=PREPARE),
             ObjectBank.from_db_info_files(root, ["kitti_dbinfos_val.pkl"], CLASSES, prepare=PREPARE, device=DEV)]
    outs = []
    for bank in banks:
        frames = []
        for info in infos[:3]:
            a = info["annos"]                                                 # two ground truths: most grid places stay free
            frames.append({"points": torch.from_numpy(clouds[info["point_cloud"]["lidar_idx"]]).to(DEV),
                           "gt_boxes": a["gt_boxes_lidar"][:2].astype(np.float32), "gt_names": a["name"][:2]})
        out = DeviceAugmentor(cfg, CLASSES, bank, rng6)(frames, rng=np.random.RandomState(2121))
        torch.cuda.synchronize()
        outs.append(out)
    a, b = outs
    assert a["valid"].cpu().numpy().sum() >= 3                                # something was pasted
    assert np.array_equal(a["num_points"], b["num_points"]) and np.array_equal(a["num_boxes"], b["num_boxes"])
    for k in ("points", "gt_boxes", "point_frame_offsets", "valid"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert json.dumps([p["cand_obj"].tolist() for p in a["plans"]]) == json.dumps([p["cand_obj"].tolist() for p in b["plans"]])
