"""GPU: the training augmentation kernels (csrc/augment.hip) and DeviceAugmentor against fixture G19 (the reference's own
DataAugmentor.forward + box trim) and against the numpy restatement of tests/augment_cases.py, which test_augment_host.py pins
to G19 on the CPU.  Every case keeps the margin condition of augment_cases (asserted there), so zero / non-zero IoU and
inside / outside are decided alike in float64 and in the fp32 kernels; exact-boundary behaviour is tested with headings of 0.

Float bound against the restatement run in float64 on the same float32 cos, sin and scale (a derivation, not a measurement):
a rotated coordinate is a sum of two products, then one product with the scale: at most three rounded operations (two for a
point, whose second product is fused into the sum), each within 2^-24 of a value no larger than (|x| + |y|) scale, so
|d| <= 3 * 2^-24 (|x| + |y|) scale.  z and the box sizes take one rounded product:
bit-equal to the float32 product.  A heading takes at most one sum with pi, one with the angle and the four operations of
limit_period, all on values below |h| + |angle| + 3 pi: |d| <= 6 * 2^-24 (|h| + |angle| + 3 pi)."""
import json

import numpy as np
import pytest

import augment_cases as AC

pytestmark = pytest.mark.gpu
RANGE = np.array([0, -40, -3, 70.5, 40, 1], np.float32)
CLASSES = ["Car", "Pedestrian", "Cyclist"]
E24 = 2.0 ** -24


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def bank():
    from hvpr_amd.augment import ObjectBank
    names, pts = AC.synthetic_bank_arrays(48)
    boxes = np.zeros((48, 7), np.float32)
    boxes[:, :3] = np.random.RandomState(3).uniform(-20, 20, (48, 3))
    boxes[:, 3:6] = AC.CAR
    b = ObjectBank.from_arrays(names, boxes, pts, CLASSES)
    b.on_device()
    return b


def run_device(frames, ops, bank, extra=(0, 0, 0), rng6=RANGE, remove_outside=True, g_cap=None):
    """frames: [dict(points (n, F) numpy, gt_boxes, gt_cls, plan)] -> everything the kernels write, on the host."""
    torch = torch_()
    from hvpr_amd import kernels
    from hvpr_amd.augment import pack_plans, plan_words
    B = len(frames)
    NG = len(frames[0]["plan"]["group_off"]) - 1
    G, C = sum(len(f["gt_boxes"]) for f in frames), sum(len(f["plan"]["cand_obj"]) for f in frames)
    stage = torch.empty((plan_words(B, NG, G, C),), dtype=torch.int32).pin_memory()
    ops_word = sum(op << (4 * k) for k, op in enumerate(ops))
    words = pack_plans(stage.numpy(), [f["plan"] for f in frames], [f["gt_boxes"] for f in frames], [f["gt_cls"] for f in frames],
                       [len(f["points"]) for f in frames], ops_word, NG, bank.host_points()[1])
    dev = stage.to("cuda:0")
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([f["points"] for f in frames]), np.float32)).to("cuda:0")
    if g_cap is None:
        g_cap = max(1, max(int((np.asarray(f["gt_cls"]) > 0).sum()) + len(f["plan"]["cand_obj"]) for f in frames))
    out = kernels.augment_batch(stage, dev, words, pts, bank, np.asarray(extra, np.float32), rng6, remove_outside, g_cap)
    torch.cuda.synchronize()
    counts = out["counts"].cpu().numpy()
    return {"off": counts[: B + 1], "nbox": counts[B + 1:], "points": out["points"].cpu().numpy(), "gt": out["gt_boxes"].cpu().numpy(),
            "valid": out["valid"].cpu().numpy().astype(bool)}


def restate(frames, ops, bank, extra=(0, 0, 0), rng6=RANGE, remove_outside=True, dtype=np.float64):
    arena, off = bank.host_points()
    return [AC.augment_frame(f["points"], f["gt_boxes"], f["gt_cls"], f["plan"], ops, arena, off, bank.obj_box, extra, rng6,
                             remove_outside, dtype) for f in frames]


def entering(rows, plan, sc):
    """|x| + |y| of what entered the rotation, (n, 1): the float64 output un-scaled and turned back (cos^2 + sin^2 of the float32
    pair is 1 within 2^-23: the 1e-6 covers it)."""
    c, s = float(plan["cos"]), float(plan["sin"])
    x, y = rows[:, 0] / sc, rows[:, 1] / sc
    return ((np.abs(x * c + y * s) + np.abs(-x * s + y * c)) * (1 + 1e-6))[:, None]


def check_against_restatement(frames, ops, bank, got, want32, want64):
    """Offsets, kept sets and order equal; floats within the derived bound (module docstring)."""
    c0 = 0
    for f, (fr, w32, w64) in enumerate(zip(frames, want32, want64)):
        nc = len(fr["plan"]["cand_obj"])
        assert got["valid"][c0: c0 + nc].tolist() == w64["valid"].tolist(), f
        c0 += nc
        p = got["points"][got["off"][f]: got["off"][f + 1]]
        assert p.shape == w64["points"].shape, (f, p.shape, w64["points"].shape)
        assert p[:, 3:].tobytes() == w64["points"][:, 3:].astype(np.float32).tobytes(), f       # kept set, order, features
        sc = float(fr["plan"]["scale"]) if AC.OP_SCALE in ops else 1.0
        assert (np.abs(p[:, :2] - w64["points"][:, :2]) <= 3 * E24 * entering(w64["points"], fr["plan"], sc) * sc).all(), f
        assert p[:, 2].tobytes() == w32["points"][:, 2].tobytes(), f
        nb = int(got["nbox"][f])
        assert nb == len(w64["boxes"]), (f, nb, len(w64["boxes"]))
        b = got["gt"][f]
        assert not b[nb:].any(), f
        assert np.array_equal(b[:nb, 7], w64["boxes"][:, 7]), f
        assert b[:nb, 2:6].tobytes() == w32["boxes"][:, 2:6].tobytes(), f
        assert (np.abs(b[:nb, :2] - w64["boxes"][:, :2]) <= 3 * E24 * entering(w64["boxes"], fr["plan"], sc) * sc).all(), f
        hb = 6 * E24 * (np.abs(w64["boxes"][:, 6]) + abs(fr["plan"]["angle"]) + 3 * np.pi)
        assert (np.abs(b[:nb, 6] - w64["boxes"][:, 6]) <= hb).all(), f


# ------------------------------------------------------------------------------------------------ G19
def g19_device_runs():
    torch = torch_()
    from hvpr_amd.augment import DeviceAugmentor
    z = AC.g19()
    out = []
    for run in (0, 1):
        bank = AC.g19_bank(z, json.loads(str(z["prepare"])))
        aug = DeviceAugmentor(AC.g19_config(z, run), [str(c) for c in z["class_names"]], bank, z["range"])
        frames = AC.g19_frames(z, run)
        batch = [dict(fr, points=torch.from_numpy(fr["points"]).to("cuda:0")) for _, fr in frames]
        out.append(([f for f, _ in frames], aug(batch, rng=np.random.RandomState(int(z[f"run{run}.seed"])))))
    return z, out


@pytest.fixture(scope="module")
def g19_runs():
    return g19_device_runs()


def ulps(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / AC.ulp32(ref)


def test_g19_through_device_augmentor(g19_runs):
    """Valid masks, box counts, the kept-point set and the point order equal to the fixture's; feature columns bit-equal; z, box
    sizes, headings and the boxes' x, y within 4 fp32 ulp of the fixture."""
    z, runs = g19_runs
    for ids, r in runs:
        valid, c0 = r["valid"].cpu().numpy().astype(bool), 0
        pts, off, gt = r["points"].cpu().numpy(), r["point_frame_offsets"].cpu().numpy(), r["gt_boxes"].cpu().numpy()
        assert np.array_equal(np.diff(off), r["num_points"])
        for i, f in enumerate(ids):
            k = f"f{f}."
            nc = len(z[k + "valid"])
            assert valid[c0: c0 + nc].tolist() == z[k + "valid"].tolist(), f
            c0 += nc
            ref_p, ref_b = z[k + "out_points"], z[k + "out_boxes"]
            p, nb = pts[off[i]: off[i + 1]], int(r["num_boxes"][i])
            assert p.shape == ref_p.shape and nb == len(ref_b), f
            assert p[:, 3].tobytes() == ref_p[:, 3].tobytes(), f
            assert np.array_equal(gt[i, :nb, 7], ref_b[:, 7]) and not gt[i, nb:].any(), f
            for name, e in (("point z", ulps(p[:, 2], ref_p[:, 2])), ("boxes", ulps(gt[i, :nb, :7], ref_b[:, :7]))):
                print(f"frame {f} {name}: max error {e.max() if e.size else 0:.2f} ulp")
                assert (e <= 4).all(), (f, name)


def test_g19_point_xy_within_4_ulp_of_the_fixture(g19_runs):
    """The issue's bound against the fixture: point x, y within 4 fp32 ulp at the magnitude of the output value.  The kernel fuses
    the rotation's second product into the sum as the reference's gemm does (tests/test_augment_host.py states why and what an
    unfused sum measured).  The difference also stays within 6 * 2^-24 sqrt(2) (|x'| + |y'|), twice the derived distance of
    either side from the exact value: asserted first."""
    z, runs = g19_runs
    worst = 0.0
    for ids, r in runs:
        pts, off = r["points"].cpu().numpy(), r["point_frame_offsets"].cpu().numpy()
        for i, f in enumerate(ids):
            ref, p = z[f"f{f}.out_points"], pts[off[i]: off[i + 1]]
            mag = np.sqrt(2.0) * (np.abs(ref[:, 0:1]) + np.abs(ref[:, 1:2])).astype(np.float64)
            assert (np.abs(p[:, :2].astype(np.float64) - ref[:, :2]) <= 6 * E24 * mag).all(), f
            e = ulps(p[:, :2], ref[:, :2])
            print(f"frame {f} point x, y: max error {e.max() if e.size else 0:.2f} ulp of the value")
            worst = max(worst, e.max() if e.size else 0.0)
    assert worst <= 4, worst


# ------------------------------------------------------------------------------------------------ collisions
def collision_frames(bank):
    """Five ragged frames: existing sets of 0, 1, 63, 64, 65 boxes; groups of 0, 1 and 15 candidates, three groups each; all
    accepted, all rejected, and the chain (a candidate over a REJECTED one of an earlier group is accepted, one over an ACCEPTED
    one is rejected)."""
    slots = AC.grid_boxes(130)
    flat = AC.grid_boxes(130, heading=0.0)
    flat[:, 6] = 0.0
    on = lambda b: b + np.array([0.5, 0.3, 0, 0, 0, 0, 0.05], np.float32)            # a box on top of b
    up = lambda b, k: b + np.array([0, 1.0 * k, 0, 0, 0, 0, 0], np.float32)         # heading 0: 1 m up overlaps, 2 m up does not
    free = slots[70:]
    frames = []
    # E = 0: 7 pairs that overlap only each other + 1 free; then one candidate over a rejected one; then nothing
    g0 = np.concatenate([np.stack([free[i], on(free[i])]) for i in range(7)] + [free[7:8]])
    frames.append((0, [g0, free[0][None] + np.array([0.2, -0.2, 0, 0, 0, 0, 0.1], np.float32), np.zeros((0, 7), np.float32)]))
    frames.append((1, [on(slots[0])[None], free[:15], np.zeros((0, 7), np.float32)]))                    # rejected; all accepted
    frames.append((63, [on(slots[:15]), free[:15], on(free[:15])]))                                      # all rejected / accepted / rejected
    frames.append((64, [np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32), free[3:4]]))
    a = flat[80]
    frames.append((65, [a[None], up(a, 1)[None], up(a, 2)[None]]))                  # accepted; over it: rejected; over the rejected only
    out = []
    for ne, groups in frames:
        cb = np.concatenate(groups).astype(np.float32)
        off = np.cumsum([0] + [len(g) for g in groups])
        gcls = np.array([(i % 2) for i in range(ne)], np.int32)                     # every other ground truth is of a hidden class
        out.append({"points": np.zeros((0, 4), np.float32), "gt_boxes": slots[:ne].copy(), "gt_cls": gcls,
                    "plan": AC.make_plan(np.arange(len(cb)) % len(bank), cb, off, cand_cls=1 + np.arange(len(cb)) % 3)})
    return out


@pytest.mark.parametrize("batched", [False, True])
def test_collision_kernel_against_the_restatement(bank, batched):
    frames = collision_frames(bank)
    want = [AC.collide(f["gt_boxes"], f["plan"]["cand_box"], f["plan"]["group_off"]) for f in frames]     # asserts the margins
    assert want[0].sum() == 2 and want[1].sum() == 15 and want[2].sum() == 15 and want[3].all() and want[4].tolist() == [1, 0, 1]
    if batched:
        got = run_device(frames, [], bank)
        assert got["valid"].tolist() == np.concatenate(want).tolist()
        assert got["nbox"].tolist() == [int((f["gt_cls"] > 0).sum() + w.sum()) for f, w in zip(frames, want)]
    else:
        for f, w in zip(frames, want):
            assert run_device([f], [], bank)["valid"].tolist() == w.tolist()


# ------------------------------------------------------------------------------------------------ points
def point_frames(bank, blk, seed=11, wide=False):
    """Frames of 0, 1, blk - 1, blk, blk + 1 and 3 blk + 7 scene points; 0 or 20 accepted boxes; every point removed, none
    removed, a mix; a frame whose output is candidate points only (no scene point at all).  wide: two frames of 40 blk + 3 and
    30 blk + 1 points, a mix — 2 x 41 block counts, more than the 64 lanes of the scan's first wave."""
    r = np.random.RandomState(seed)
    boxes = AC.grid_boxes(20, x0=6.0, y0=-30.0)
    arena_off = bank.host_points()[1]
    full = [i for i in range(len(bank)) if arena_off[i + 1] > arena_off[i]]

    def inside(n):
        b = boxes[r.randint(0, 20, n)]
        l = r.uniform(-0.4, 0.4, (n, 3)) * b[:, 3:6]
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        return np.stack([l[:, 0] * c - l[:, 1] * s + b[:, 0], l[:, 0] * s + l[:, 1] * c + b[:, 1], l[:, 2] + b[:, 2], r.uniform(0, 1, n)], 1)

    def outside(n):
        p = inside(n)
        p[:, 2] += 5.0
        return p

    mix = lambda n: np.concatenate([inside(n // 2), outside(n - n // 2)])[r.permutation(n)]
    specs = [(0, True, None), (1, True, inside), (blk - 1, False, inside), (blk, True, outside), (blk + 1, True, inside),
             (3 * blk + 7, True, mix)]
    if wide:
        specs = [(40 * blk + 3, True, mix), (30 * blk + 1, True, mix)]
    frames = []
    for n, with_boxes, make in specs:
        pts = make(n).astype(np.float32) if n else np.zeros((0, 4), np.float32)
        cb = boxes if with_boxes else np.zeros((0, 7), np.float32)
        ids = [0] + [full[i % len(full)] for i in range(1, len(cb))] if len(cb) else []          # object 0 is the empty one
        frames.append({"points": pts, "gt_boxes": np.zeros((0, 7), np.float32), "gt_cls": np.zeros((0,), np.int32),
                       "plan": AC.make_plan(ids, cb, [0, len(cb)], flip_x=bool(n % 2), angle=0.2 + 0.01 * len(frames), scale=1.03)})
    return frames


@pytest.mark.parametrize("extra", [(0.0, 0.0, 0.0), (0.25, 0.5, 0.125)])
def test_point_kernels_against_the_restatement(bank, extra):
    from hvpr_amd import kernels
    blk = kernels.augment_block_points()
    frames = point_frames(bank, blk)
    ops = [AC.OP_FLIP_X, AC.OP_ROTATE, AC.OP_SCALE]
    for f in frames:
        assert AC.margins_ok(f["points"], f["gt_boxes"], f["plan"], extra, np.zeros((0, 8)), RANGE)[0]
    got = run_device(frames, ops, bank, extra, remove_outside=False)
    w32, w64 = restate(frames, ops, bank, extra, remove_outside=False, dtype=np.float32), \
        restate(frames, ops, bank, extra, remove_outside=False)
    kept = [len(w["kept"]) for w in w64]
    assert kept[1] == 0 and kept[2] == blk - 1 and kept[3] == blk and kept[4] == 0 and 0 < kept[5] < 3 * blk + 7     # all / none / some removed
    assert len(w64[0]["points"]) > 0 and len(frames[0]["points"]) == 0                                               # candidate points only
    assert got["off"].tolist() == np.cumsum([0] + [len(w["points"]) for w in w64]).tolist()
    check_against_restatement(frames, ops, bank, got, w32, w64)


def test_point_kernels_with_block_counts_past_one_wave(bank):
    """Two frames whose 2 x 41 per-block counts do not fit the first wave of k_points_scan's block scan: offsets, kept sets, order
    and floats as in the restatement."""
    from hvpr_amd import kernels
    blk = kernels.augment_block_points()
    frames = point_frames(bank, blk, seed=12, wide=True)
    ops = [AC.OP_FLIP_X, AC.OP_ROTATE, AC.OP_SCALE]
    for f in frames:
        assert AC.margins_ok(f["points"], f["gt_boxes"], f["plan"], (0.0, 0.0, 0.0), np.zeros((0, 8)), RANGE)[0]
    got = run_device(frames, ops, bank, remove_outside=False)
    w32, w64 = restate(frames, ops, bank, remove_outside=False, dtype=np.float32), restate(frames, ops, bank, remove_outside=False)
    kept = [len(w["kept"]) for w in w64]
    assert 19 * blk < kept[0] < 21 * blk and 14 * blk < kept[1] < 16 * blk                # half of each frame removed
    assert got["off"].tolist() == np.cumsum([0] + [len(w["points"]) for w in w64]).tolist()
    check_against_restatement(frames, ops, bank, got, w32, w64)


# ------------------------------------------------------------------------------------------------ exact edges
def test_exact_faces_and_range_bounds_and_identity(bank):
    nx = lambda v, d: np.nextafter(np.float32(v), np.float32(d))
    cut = np.array([[10, 5, 0, 4, 2, 2, 0]], np.float32)                             # faces x 8 | 12, y 4 | 6, z -1 | 1: heading exactly 0
    pts = np.array([[12, 5, 0, .1], [8, 5, 0, .2], [10, 6, 0, .3], [10, 4, 0, .4],                    # on an x / y face: outside (<)
                    [10, 5, 1, .5], [10, 5, -1, .6], [nx(12, 0), nx(6, 0), 1, .7],                    # on a z face: inside (<=)
                    [10, 5, nx(1, 2), .8], [11, 5.5, 0.5, .9]], np.float32)
    stays = [True, True, True, True, False, False, False, True, False]
    gts = np.array([[-2, 0, 0, 4, 2, 2, 0], [72.5, 0, 0, 4, 2, 2, 0], [30, -41, 0, 4, 2, 2, 0], [30, 41, 0, 4, 2, 2, 0],
                    [30, 0, -4, 4, 2, 2, 0], [30, 0, 2, 4, 2, 2, 0]], np.float32)       # a corner exactly on each of the six bounds
    out = gts.copy()                                                                 # ... and the same boxes one ulp further out
    out[0, 0], out[1, 0], out[2, 1], out[3, 1], out[4, 2], out[5, 2] = nx(-2, -9), nx(72.5, 99), nx(-41, -99), nx(41, 99), nx(-4, -9), nx(2, 9)
    frame = {"points": pts, "gt_boxes": np.concatenate([gts, out]), "gt_cls": np.arange(12, dtype=np.int32) % 3 + 1,
             "plan": AC.make_plan([1], cut, [0, 1], cand_cls=[2])}
    ops = [AC.OP_FLIP_X, AC.OP_FLIP_Y, AC.OP_ROTATE, AC.OP_SCALE]                     # no flip drawn, angle 0, scale 1: the identity
    got = run_device([frame], ops, bank)
    assert got["valid"].tolist() == [True]
    arena, off = bank.host_points()
    n_obj = int(off[2] - off[1])
    scene = got["points"][n_obj: got["off"][1]]
    assert scene.tobytes() == pts[stays].tobytes()                                    # faces as stated, identity bit-exact
    want_obj = arena[off[1]: off[2]].copy()
    want_obj[:, :3] += bank.obj_box[1, :3]
    assert got["points"][:n_obj].tobytes() == want_obj.tobytes()
    assert int(got["nbox"][0]) == 7                                                   # six on a bound kept, six one ulp out dropped
    assert got["gt"][0, :6, :7].tobytes() == frame["gt_boxes"][:6].tobytes() and got["gt"][0, 6, :7].tobytes() == cut.tobytes()
    assert got["gt"][0, :7, 7].tolist() == [1, 2, 3, 1, 2, 3, 2]


# ------------------------------------------------------------------------------------------------ the call as a whole
def test_two_runs_give_identical_bytes(bank):
    from hvpr_amd import kernels
    frames = point_frames(bank, kernels.augment_block_points())
    ops = [AC.OP_FLIP_Y, AC.OP_ROTATE, AC.OP_SCALE]
    a, b = (run_device(frames, ops, bank, (0.1, 0.1, 0.1)) for _ in range(2))
    total = a["off"][-1]
    for k in a:
        x, y = (v[:total] if k == "points" else v for v in (a[k], b[k]))
        assert x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("n_frames", [1, 8])
def test_call_reads_the_device_once(n_frames, monkeypatch):
    torch = torch_()
    from hvpr_amd.augment import DeviceAugmentor
    z = AC.g19()
    bank = AC.g19_bank(z, json.loads(str(z["prepare"])))
    bank.on_device()                                                                  # the upload is not a read
    aug = DeviceAugmentor(AC.g19_config(z, 0), CLASSES, bank, z["range"])
    src = [fr for _, fr in AC.g19_frames(z, 0)][:2]
    batch = [dict(src[i % 2], points=torch.from_numpy(src[i % 2]["points"]).to("cuda:0")) for i in range(n_frames)]
    torch.cuda.synchronize()
    reads = []
    real_cpu, real_item, real_tolist = torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append("cpu"), real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.append("item"), real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append("tolist"), real_tolist(self))[1])
    r = aug(batch, rng=np.random.RandomState(1))
    assert reads == ["cpu"], reads
    assert len(r["num_points"]) == n_frames and r["num_boxes"].sum() > 0


def test_refusals_return_an_error_and_leave_outputs_untouched(bank):
    torch = torch_()
    from hvpr_amd import kernels
    from hvpr_amd.augment import pack_plans, plan_words
    arena, obj_box = bank.on_device()
    boxes = AC.grid_boxes(2)
    pts = np.random.RandomState(2).uniform(0, 40, (50, 4)).astype(np.float32)

    def staged(cand_obj):
        stage = torch.empty((plan_words(1, 1, 0, 2),), dtype=torch.int32).pin_memory()
        off = np.append(bank.host_points()[1], [0, 0])                                # room for an id past the bank
        n = pack_plans(stage.numpy(), [AC.make_plan(cand_obj, boxes, [0, 2])], [np.zeros((0, 7), np.float32)],
                       [np.zeros((0,), np.int32)], [50], 0, 1, off)
        return stage, stage.to("cuda:0"), n

    stage, dev, n = staged([1, 2])
    valid = torch.ones((2,), dtype=torch.int32, device="cuda:0")
    need = 50 + int(bank.host_points()[1][3] - bank.host_points()[1][1])
    sentinel = lambda *shape: torch.full(shape, -7.0, device="cuda:0")
    off = torch.full((2,), -7, dtype=torch.int32, device="cuda:0")
    cases = [("width", torch.from_numpy(np.ascontiguousarray(pts[:, :3])).to("cuda:0"), sentinel(need, 3), (stage, dev, n)),
             ("capacity", torch.from_numpy(pts).to("cuda:0"), sentinel(need - 1, 4), (stage, dev, n)),
             ("object id", torch.from_numpy(pts).to("cuda:0"), sentinel(need + 8, 4), staged([1, len(bank)]))]
    for what, p, out, (st, dv, nw) in cases:
        with pytest.raises(RuntimeError, match="hvpr_augment_points_f32"):
            kernels.augment_points(st, dv, nw, valid, p, arena, obj_box, np.zeros((3,), np.float32), out=out, out_off=off)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((off == -7).all()), what
    gt, cnt = sentinel(1, 1, 8), torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
    with pytest.raises(RuntimeError, match="hvpr_augment_boxes_f32"):                 # two candidates may be accepted: g_cap 1 is too small
        kernels.augment_boxes(stage, dev, n, valid, RANGE, True, 1, out=gt, count=cnt)
    torch.cuda.synchronize()
    assert bool((gt == -7.0).all()) and bool((cnt == -7).all())
