"""CPU: the host side of the training augmentation (hvpr_amd/augment.py) and the numpy restatement the GPU tests check against
(tests/augment_cases.py), both pinned to fixture G19 = the reference's own DataAugmentor.forward + box trim
(tests/golden/make_golden_augment.py; the two natives the reference calls are absent upstream and stay unpinned)."""
import ctypes
import os
import re

import numpy as np
import pytest

import augment_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hvpr_augment_block_points", "hvpr_augment_collide_f32", "hvpr_augment_boxes_f32",
               "hvpr_augment_points_workspace_bytes", "hvpr_augment_points_f32"]


@pytest.fixture(scope="module")
def z():
    return AC.g19()


@pytest.fixture(scope="module")
def planned(z):
    """Every run of G19 through AugmentPlanner under the fixture's seed: [(run, frame, frame dict, plan, planner, bank, rng state)]."""
    import json
    from hvpr_amd.augment import AugmentPlanner
    out = []
    for run in (0, 1):
        cfg = AC.g19_config(z, run)
        bank = AC.g19_bank(z, json.loads(str(z["prepare"])), device="cpu")
        planner = AugmentPlanner(cfg, [str(c) for c in z["class_names"]], bank)
        rng = np.random.RandomState(int(z[f"run{run}.seed"]))
        for f, fr in AC.g19_frames(z, run):
            plan = planner.plan_frame(fr["gt_names"], fr.get("calib"), fr.get("road_plane"), rng)
            out.append((run, f, fr, plan, planner, bank, rng.get_state()))
    return out


def uid_of(z, bank):
    """bank object id -> row of the fixture's database arrays."""
    return np.array([int(np.nonzero((z["db.boxes"] == b).all(axis=1))[0][0]) for b in bank.obj_box], np.int64)


def test_object_bank_filters_give_the_recorded_survivors(z, planned):
    for run in (0, 1):
        bank = [p for p in planned if p[0] == run][0][5]
        uid = uid_of(z, bank)
        for c in bank.class_names:
            assert uid[bank.class_ids[c]].tolist() == z[f"run{run}.survivors.{c}"].tolist(), (run, c)
        arena, off = bank.host_points()
        assert (np.diff(off) == 0).any(), "the empty object survives"
        for i, u in enumerate(uid):
            assert np.array_equal(arena[off[i]: off[i + 1]], z["db.points"][z["db.point_off"][u]: z["db.point_off"][u + 1]])


def test_planner_makes_the_recorded_draws_and_leaves_the_recorded_state(z, planned):
    wraps = shorts = 0
    for run, f, fr, plan, planner, bank, state in planned:
        k = f"f{f}."
        uid = uid_of(z, bank)
        assert uid[plan["cand_obj"]].tolist() == z[k + "cand_uid"].tolist(), f
        sizes = [len(g) for g in plan["group_idx"] if len(g)]
        assert sizes == z[k + "group_sizes"].tolist(), f
        assert np.array_equal(state[1], z[k + "rng_keys"]) and [state[2], state[3]] == z[k + "rng_pos"].tolist(), f
        assert state[4] == float(z[k + "rng_gauss"])
        # the draws themselves, in order: permutations (as class-list indices), flip choices, uniforms
        tags, vals, pos = str(z[k + "draw_tags"]), z[k + "draw_values"], 0
        uni = [plan["angle"]] if "random_world_rotation" in [c["NAME"] for c in planner.queue] else []
        uni += [float(plan["scale"])] if AC.OP_SCALE in planner.ops else []
        flips = [plan["flip_" + a] for c in planner.queue if c["NAME"] == "random_world_flip" for a in c["ALONG_AXIS_LIST"]]
        for t, n in zip(tags, z[k + "draw_sizes"]):
            v = vals[pos: pos + n]
            pos += n
            if t == "c":
                assert bool(v[0]) == flips.pop(0), f
            elif t == "u":
                u = uni.pop(0)
                assert v[0] == u or np.float32(v[0]) == np.float32(u), f
            else:
                wraps += 1
        assert not flips and not uni, f
        shorts += any(len(g) and len(g) < int(planner.groups[c]["sample_num"]) for c, g in zip(planner.groups, plan["group_idx"]))
    assert wraps > 6 and shorts > 0          # more permutations than first calls: a pointer wrapped; a last slice was short


def _restated(z, planned):
    for run, f, fr, plan, planner, bank, _ in planned:
        arena, off = bank.host_points()
        cls = np.array([bank.class_names.index(n) + 1 if n in bank.class_names else 0 for n in fr["gt_names"]], np.int32)
        yield f, AC.augment_frame(fr["points"], fr["gt_boxes"], cls, plan, planner.ops, arena, off, bank.obj_box,
                                  planner.extra_width, z["range"])


def ulps(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / AC.ulp32(ref)


def test_restatement_reproduces_g19(z, planned):
    """Exact: valid masks, counts, the kept set and the point order (by the bit-equal feature column), classes.  Floats that
    take no sum of products (z, the box sizes, the heading) within 4 fp32 ulp of the fixture."""
    for f, r in _restated(z, planned):
        k = f"f{f}."
        assert r["valid"].tolist() == z[k + "valid"].tolist(), f
        ref_p, ref_b = z[k + "out_points"], z[k + "out_boxes"]
        assert r["points"].shape == ref_p.shape and r["boxes"].shape == ref_b.shape, f
        assert r["points"][:, 3].tobytes() == ref_p[:, 3].tobytes(), f
        assert np.array_equal(r["boxes"][:, 7], ref_b[:, 7]), f
        assert np.array_equal(r["boxes_before_trim"].shape[0], z[k + "out_boxes_before_trim"].shape[0]), f
        for name, e in (("z", ulps(r["points"][:, 2], ref_p[:, 2])), ("box z, sizes, heading", ulps(r["boxes"][:, 2:7], ref_b[:, 2:7]))):
            print(f"frame {f} {name}: max error {e.max() if e.size else 0:.2f} ulp")
            assert (e <= 4).all(), (f, name)


def test_restatement_xy_within_4_ulp_of_g19(z, planned):
    """The issue's bound against the fixture: x, y of points and boxes within 4 fp32 ulp at the magnitude of the output value.

    It holds because the rotation of POINTS fuses its second product into the sum (x' = fma(y, -s, x c), y' = fma(y, c, x s)), as
    the float32 gemm behind the reference's torch.matmul does for a frame's points (45 rows and more), while a frame's few boxes
    take torch's unfused small-matrix sum.  With an unfused sum for points the same check measured 23, 13 and 83 ulp in the three
    rotated frames: half an ulp of one product is many ulp of the result where the two products cancel.  The wider statement
    holds either way and is asserted first: both sides are within 3 * 2^-24 (|x| + |y|) scale of the exact value, so within
    twice that of each other, and |x| + |y| <= sqrt(2) (|x'| + |y'|)."""
    worst = 0.0
    for (run, f, fr, plan, planner, bank, _), (_, r) in zip(planned, _restated(z, planned)):
        k = f"f{f}."
        for name, got, ref in (("points", r["points"], z[k + "out_points"]), ("boxes", r["boxes"], z[k + "out_boxes"])):
            if not len(ref):
                continue
            mag = np.sqrt(2.0) * (np.abs(ref[:, 0:1]) + np.abs(ref[:, 1:2])).astype(np.float64)
            assert (np.abs(got[:, :2].astype(np.float64) - ref[:, :2]) <= 6 * 2.0 ** -24 * mag).all(), (f, name)
            e = ulps(got[:, :2], ref[:, :2])
            print(f"frame {f} {name} x, y: max error {e.max():.2f} ulp of the value")
            worst = max(worst, e.max())
    assert worst <= 4, worst


def test_new_symbols_in_header_bindings_and_exports():
    from hvpr_amd import _lib, build
    L = ctypes.CDLL(build.build())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvpr_amd.h")).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert _lib.lib().hvpr_augment_block_points() == 256
    assert _lib.lib().hvpr_augment_points_workspace_bytes(2, 1000, 5, 1500) > 1500
    assert _lib.ABI_VERSION == 8


def test_plan_refusals_need_no_gpu():
    """Every check of a plan is made on its host copy, before any launch."""
    from hvpr_amd import _lib
    from hvpr_amd.augment import pack_plans, plan_words
    plan = AC.make_plan([0], AC.grid_boxes(1), [0, 1])
    buf = np.zeros((plan_words(1, 1, 0, 1),), np.int32)
    n = pack_plans(buf, [plan], [np.zeros((0, 7), np.float32)], [np.zeros((0,), np.int32)], [0], 0, 1, np.array([0, 3]))
    L, fake = _lib.lib(), ctypes.c_void_p(256)
    assert L.hvpr_augment_collide_f32(buf.ctypes.data, fake, n - 1, fake, None) == -1          # word count does not match
    bad = buf.copy()
    bad[0] = 7
    assert L.hvpr_augment_collide_f32(bad.ctypes.data, fake, n, fake, None) == -1              # not a plan
    ex = np.zeros((3,), np.float32)
    args = lambda F, n_obj, cap: (buf.ctypes.data, fake, n, fake, fake, 0, F, fake, 3, fake, n_obj, 4, ex.ctypes.data, fake, cap, fake,
                                  fake, 1 << 20, None)
    assert L.hvpr_augment_points_f32(*args(5, 1, 3)) == -1                                     # feature widths differ
    assert L.hvpr_augment_points_f32(*args(4, 0, 3)) == -1                                     # candidate id outside the bank
    assert L.hvpr_augment_points_f32(*args(4, 1, 2)) == -1                                     # capacity too small
