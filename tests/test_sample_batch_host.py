"""CPU: `sample_points` for a whole batch.  The planner that draws over ordinals from the two counts of a frame
(hvpr_amd.preprocess.plan_sample_points, which preprocess.sample_points_choice is built on) against the oracle's independent
per-frame form that sees the flags (oracle.hvpr_oracle.sample_points_choice); the numpy restatement (tests/sample_batch_cases.py) against fixture G23, the reference's own path
(tests/golden/make_golden_sample_batch.py); the shipped configs; the new entry points of csrc/collate.hip, which make every
argument check on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_loader_cases as BC
import sample_batch_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hvpr_ragged_sample_workspace_bytes", "hvpr_ragged_sample_count_f32", "hvpr_ragged_sample_write_f32"]


@pytest.fixture(scope="module")
def z():
    return SC.g23()


def same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return bool(np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:])


# ------------------------------------------------------------------------------------------------ 1. the planner
def flag_cases():
    """(name, near flags, P): every branch of data_processor.py:77-108."""
    g = np.random.RandomState(77)

    def flags(n, c):
        f = np.zeros((n,), np.uint8)
        f[g.permutation(n)[:c]] = 1
        return f

    return [("n > P, near and far", flags(300, 200), 128), ("n > P, one near row drawn", flags(130, 2), 129),
            ("n > P, no far row", flags(200, 200), 64), ("n > P, every near row taken", flags(100, 36), 99),
            ("want == 0", flags(180, 52), 128), ("want == 0, one near row", flags(91, 1), 90),
            ("n == P", flags(128, 70), 128), ("n < P", flags(100, 60), 128), ("n < P, doubled", flags(64, 1), 128),
            ("n == 1, P == 2", flags(1, 1), 2), ("P == -1", flags(50, 20), -1), ("P == 0 of some", flags(5, 5), 0),
            ("empty, P == 0", flags(0, 0), 0), ("empty, P == -1", flags(0, 0), -1)]


@pytest.mark.parametrize("shuffle", [False, True])
def test_planner_equals_the_per_frame_form(shuffle):
    from hvpr_amd.batch_loader import plan_sample_points, resolve_sample_choice, sample_destinations
    from oracle import hvpr_oracle as O
    seen = set()
    for k, (name, near, P) in enumerate(flag_cases()):
        n, c = len(near), int(near.sum())
        a, b = np.random.RandomState(900 + k), np.random.RandomState(900 + k)
        want = O.sample_points_choice(near, P, a)
        want_perm = a.permutation(len(want)) if shuffle else None
        plan = plan_sample_points(n, c, P, b, shuffle=shuffle)
        got = resolve_sample_choice(plan, near)
        assert np.array_equal(got, want), name
        assert same_state(a, b), name
        order = got if not shuffle else got[plan["perm"]]
        if shuffle:
            assert np.array_equal(plan["perm"], want_perm), name
        assert np.array_equal(resolve_sample_choice(dict(plan, choice=plan["order"]), near), order), name
        # the table the write pass reads: output row j holds source order[j]
        dest = sample_destinations(plan["order"], n)
        assert dest.shape == (n, 2) and dest.dtype == np.int32
        back = np.full((len(order),), -1, np.int64)
        for col in (0, 1):
            src = np.nonzero(dest[:, col] >= 0)[0]
            assert (back[dest[src, col]] == -1).all()
            back[dest[src, col]] = src
        assert np.array_equal(back, plan["order"]), name
        assert ((dest[:, 1] == -1) | (dest[:, 0] >= 0)).all()
        if not (0 <= P and n < P):
            assert (dest[:, 1] == -1).all(), "two destinations only where a frame is padded"
        seen.add((P == -1, 0 <= P < n, plan["mode"], n < P, n == P))
    assert {(False, True, 1, False, False), (False, True, 0, False, False), (False, False, 0, True, False),
            (False, False, 0, False, True), (True, False, 0, False, False)} <= seen


def test_refusals_are_the_references(z):
    from hvpr_amd.batch_loader import plan_sample_points
    from oracle import hvpr_oracle as O
    P = int(z["num_sample_points"])
    assert bool(z["raises.more_far_than_p"]) and bool(z["raises.two_n_less_than_p"]) and bool(z["raises.empty_frame"])
    assert not bool(z["raises.control_far_equals_p"]) and not bool(z["raises.control_two_n_equals_p"])
    for n, c in ((P + 11, 10), (P // 2 - 1, P // 2 - 1), (0, 0)):              # the fixture's three frames
        near = np.r_[np.ones((c,), np.uint8), np.zeros((n - c,), np.uint8)]
        with pytest.raises(ValueError):
            O.sample_points_choice(near, P, np.random.RandomState(1))
        with pytest.raises(ValueError):
            plan_sample_points(n, c, P, np.random.RandomState(1))
    plan_sample_points(P + 10, 10, P, np.random.RandomState(1))                 # and its two controls
    plan_sample_points(P // 2, P // 2, P, np.random.RandomState(1))
    with pytest.raises(ValueError):
        plan_sample_points(5, 6, P, np.random.RandomState(1))


# ------------------------------------------------------------------------------------------------ 2. the restatement on G23
def test_scene_shows_what_it_is_there_for(z):
    P = int(z["num_sample_points"])
    n, c = [int(z[f"train.b{b}.n"]) for b in range(2)], [int(z[f"train.b{b}.c"]) for b in range(2)]
    assert n[0] > P and 0 < c[0] < n[0] and n[0] - c[0] < P and P / 2 <= n[1] < P
    assert [len(z[f"train.b{b}.items"]) for b in range(2)] == [1, 1], "no redraw"
    tn, tc = [int(z[f"test.b{b}.n"]) for b in range(4)], [int(z[f"test.b{b}.c"]) for b in range(4)]
    assert tn[0] > P and tn[0] - tc[0] < P and tn[1] < P and tn[2] == P and tn[3] > P and tn[3] - tc[3] == P
    assert [str(z[f"test.b{b}.draw_tags"]) for b in range(4)] == ["ccs", "cs", "s", "ccs"]
    assert str(z["train.b0.draw_tags"]).endswith("ccsp") and str(z["train.b1.draw_tags"]).endswith("csp")
    cfg = SC.g23_config(z)
    assert [p["NAME"] for p in cfg["DATA_PROCESSOR"]] == ["mask_points_and_boxes_outside_range", "sample_points", "shuffle_points"]
    for m in ("train", "test"):
        assert len(np.unique(z[m + ".points"][:, [0, 4]], axis=0)) < len(z[m + ".points"]), "padded rows repeat"


def test_restatement_reproduces_g23_train(z, observed):
    from hvpr_amd.augment import AugmentPlanner
    cfg, P = SC.g23_config(z), int(z["num_sample_points"])
    bank = BC.g22_bank(z, device="cpu")
    planner = AugmentPlanner(cfg["DATA_AUGMENTOR"], [str(c) for c in z["class_names"]], bank)
    gens = SC.g23_generators(z, "train")
    points, gt, slots = SC.prepare_batch_host(BC.g22_frames(z), z["train.indices"].tolist(), planner, bank, gens, z["range"],
                                              int(z["num_frames"]), P)
    BC.assert_same_batch(z["train.points"], z["train.gt_boxes"], points, gt, observed, "G23 restatement")
    for b, s in enumerate(slots):
        k = f"train.b{b}."
        assert s["items"] == z[k + "items"].tolist() and (s["n"], s["c"]) == (int(z[k + "n"]), int(z[k + "c"])), b
        assert np.array_equal(s["choice"], z[k + "choice"]) and np.array_equal(s["perm"], z[k + "perm"]), b
        assert SC.state_matches(gens[b], z, "train", b), ("generator state after the frame", b)
        assert len(s["points"]) == P and len(s["r"]["boxes"]) == int(z[k + "num_boxes"])


def test_restatement_reproduces_g23_test_mode(z):
    P = int(z["num_sample_points"])
    gens = SC.g23_generators(z, "test")
    points, gt, slots = SC.test_batch_host(BC.g22_frames(z), z["test.indices"].tolist(), [str(c) for c in z["class_names"]], gens,
                                           z["range"], P)
    assert points.shape == z["test.points"].shape and points.tobytes() == z["test.points"].tobytes()
    assert gt.shape == z["test.gt_boxes"].shape and gt.tobytes() == z["test.gt_boxes"].tobytes()
    for b, s in enumerate(slots):
        assert (s["n"], s["c"]) == (int(z[f"test.b{b}.n"]), int(z[f"test.b{b}.c"])), b
        assert np.array_equal(s["choice"], z[f"test.b{b}.choice"]), b
        assert SC.state_matches(gens[b], z, "test", b), ("generator state after the frame", b)


def test_planner_reproduces_g23_test_choices_from_the_counts(z):
    """What the loader does on the host: n and c in, the fixture's choice out (test mode has no draw in front of the step)."""
    from hvpr_amd.batch_loader import plan_sample_points, resolve_sample_choice
    P, frames = int(z["num_sample_points"]), BC.g22_frames(z)
    gens = SC.g23_generators(z, "test")
    for b, i in enumerate(z["test.indices"].tolist()):
        pts = frames[i]["points"]
        kept = pts[BC.fov_flag(pts, frames[i]["calib"], frames[i]["image_shape"]) & BC.range_flag(pts, z["range"])]
        plan = plan_sample_points(int(z[f"test.b{b}.n"]), int(z[f"test.b{b}.c"]), P, gens[b])
        assert np.array_equal(resolve_sample_choice(plan, SC.near_flag(kept)), z[f"test.b{b}.choice"]), b
        assert SC.state_matches(gens[b], z, "test", b), b
    assert [plan_sample_points(int(z[f"test.b{b}.n"]), int(z[f"test.b{b}.c"]), P, np.random.RandomState(b))["mode"]
            for b in range(4)] == [1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 3. the shipped configs
def shipped(name):
    from hvpr_amd import config
    cfg = config.hvpr_car_cfg() if name == "car" else config.hvpr_3class_cfg()
    aug = config.cfg_from_yaml_file(os.path.join(config.CFG_DIR, "dataset_configs", "kitti_augmentor.yaml"))
    data = dict(cfg.DATA_CONFIG)
    data["DATA_AUGMENTOR"] = aug["DATA_AUGMENTOR" if name == "car" else "DATA_AUGMENTOR_3CLASS"]
    return data, list(cfg.CLASS_NAMES)


@pytest.mark.parametrize("name", ["car", "3class"])
@pytest.mark.parametrize("training", [True, False])
def test_shipped_configs_are_accepted_with_the_keyword(z, name, training):
    from hvpr_amd.augment import ObjectBank
    from hvpr_amd.batch_loader import DeviceBatchLoader
    data, classes = shipped(name)
    off = z["db.point_off"]
    bank = ObjectBank.from_arrays([str(n) for n in z["db.names"]], z["db.boxes"], [z["db.points"][off[i]: off[i + 1]] for i in
                                  range(len(off) - 1)], classes, num_points_in_gt=z["db.num_points_in_gt"],
                                  difficulty=z["db.difficulty"], prepare=data["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0]["PREPARE"],
                                  device="cpu") if training else None
    loader = DeviceBatchLoader(data, classes, lambda i: None, 1, bank=bank, training=training, device="cpu", sample_points=True)
    assert loader.num_points == 16384 and loader.mask_range and loader.shuffle == training
    with pytest.raises(NotImplementedError, match="sample_points"):
        DeviceBatchLoader(data, classes, lambda i: None, 1, bank=bank, training=training, device="cpu")


def test_queue_positions():
    from hvpr_amd.batch_loader import DeviceBatchLoader
    mask = {"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True}
    sample = {"NAME": "sample_points", "NUM_POINTS": {"train": 64, "test": 32}}
    shuffle = {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": True}}
    voxels = {"NAME": "transform_points_to_voxels"}

    def make(queue, **kw):
        cfg = {"POINT_CLOUD_RANGE": [0, -40, -3, 70.4, 40, 1], "FOV_POINTS_ONLY": True, "DATA_PROCESSOR": queue}
        return DeviceBatchLoader(cfg, ["Car"], lambda i: None, 1, training=False, device="cpu", **kw)

    assert make([mask, sample, shuffle, voxels], sample_points=True).num_points == 32
    assert make([mask, sample], sample_points=True).num_points == 32
    assert make([mask, shuffle, voxels], sample_points=True).num_points is None
    assert make([mask, dict(sample, NUM_POINTS={"train": 64, "test": -1}), shuffle], sample_points=True).num_points is None
    for bad in ([mask, shuffle, sample], [sample, mask, shuffle], [shuffle, mask, sample], [sample], [mask, sample, sample]):
        with pytest.raises(NotImplementedError, match="sample_points"):
            make(bad, sample_points=True)
    with pytest.raises(NotImplementedError, match="sample_points"):
        make([mask, sample, shuffle])


# ------------------------------------------------------------------------------------------------ 4. the ABI
def test_new_symbols_in_header_bindings_and_exports():
    from hvpr_amd import _lib, build
    L = ctypes.CDLL(build.build())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvpr_amd.h")).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert _lib.ABI_VERSION == 8 and _lib.lib().hvpr_abi_version() == 8


def test_workspace_query_needs_no_gpu():
    from hvpr_amd import _lib
    L = _lib.lib()
    T = L.hvpr_ragged_select_tile_rows()
    for rows, frames in ((0, 4), (1, 1), (T, 4), (T + 1, 4), (70 * T, 1024)):     # both counts: twice the select layout
        assert L.hvpr_ragged_sample_workspace_bytes(rows, frames) == 2 * L.hvpr_ragged_select_workspace_bytes(rows, frames)
    assert L.hvpr_ragged_sample_workspace_bytes(-1, 4) == 0 and L.hvpr_ragged_sample_workspace_bytes(10, 0) == 0


def test_refusals_need_no_gpu():
    """Every check is made on the host, before any launch."""
    from hvpr_amd import _lib
    L, fake = _lib.lib(), ctypes.c_void_p(256)
    rxy = np.zeros((4,), np.float32)
    need = L.hvpr_ragged_sample_workspace_bytes(100, 2)
    ok_c = dict(points=fake, rows=100, F=4, off=fake, B=2, mask=3, calib=fake, range_xy=rxy.ctypes.data, near=40.0, new_off=fake,
                near_off=fake, ws=fake, ws_bytes=1 << 20)
    ok_w = dict(points=fake, rows=100, F=4, off=fake, B=2, mask=3, calib=fake, range_xy=rxy.ctypes.data, near=40.0, new_off=fake,
                near_off=fake, mode=fake, dest=fake, n_dest=100, P=64, batch_column=1, out=fake, cap=128, flag=fake, ws=fake,
                ws_bytes=1 << 20)

    def call(fn, ok, **o):
        a = dict(ok)
        assert set(o) <= set(a)
        a.update(o)
        return fn(*a.values(), None)

    for fn, ok in ((L.hvpr_ragged_sample_count_f32, ok_c), (L.hvpr_ragged_sample_write_f32, ok_w)):
        for bad in (dict(rows=-1), dict(F=2), dict(B=0), dict(mask=4), dict(mask=-1), dict(off=None), dict(points=None),
                    dict(calib=None), dict(range_xy=None), dict(new_off=None), dict(near_off=None), dict(ws=None),
                    dict(near=-1.0), dict(near=float("nan"))):
            assert call(fn, ok, **bad) == -1, bad
        assert call(fn, ok, B=1025) == -2 and call(fn, ok, rows=2 ** 31 - 1) == -2 and call(fn, ok, F=65) == -2
        assert call(fn, ok, ws_bytes=need - 1) == -3
        assert call(fn, ok, ws_bytes=L.hvpr_ragged_select_workspace_bytes(100, 2)) == -3, "the select layout is too short"
    w = L.hvpr_ragged_sample_write_f32
    for bad in (dict(mode=None), dict(dest=None), dict(n_dest=-1), dict(P=-1), dict(out=None), dict(cap=-1), dict(flag=None),
                dict(dest=ctypes.c_void_p(260))):
        assert call(w, ok_w, **bad) == -1, bad
    assert call(w, ok_w, cap=2 ** 31) == -2 and call(w, ok_w, n_dest=2 ** 30) == -2
    assert call(w, ok_w, rows=0, points=None) == 0, "nothing to do: accepted without a launch"


def test_wrappers_reject_cpu_tensors():
    import torch
    from hvpr_amd import kernels
    pts, off = torch.zeros((8, 4)), torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.ragged_sample_count(pts, off, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.ragged_sample_write(pts, off, 0, off, off, torch.zeros((1,), dtype=torch.int32),
                                    torch.zeros((8, 2), dtype=torch.int32), 4, torch.zeros((4096,), dtype=torch.uint8))
