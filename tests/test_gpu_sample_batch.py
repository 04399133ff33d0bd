"""GPU: `sample_points` for a whole batch (hvpr_ragged_sample_count_f32 / hvpr_ragged_sample_write_f32 of csrc/collate.hip and
DeviceBatchLoader(sample_points=True)).

The count pass is held BIT FOR BIT to what existed before it: new_off to hvpr_ragged_select_count_f32 on the same input,
near_off to hvpr_point_flags_f32 mode 1 over each compacted frame (one shared expression, csrc/point_pred.h), rows of fp32 norm
exactly 40 and their neighbouring floats included.  The write pass is called with hand-made tables and compared byte for byte,
sentinel and guard rows included, with what the table names.  The loader is compared with fixture G23 (the reference's own path,
tests/golden/make_golden_sample_batch.py) and, bit for bit, with the per-frame chain of the same build."""
import numpy as np
import pytest

import test_gpu_batch_loader as TB

pytestmark = pytest.mark.gpu
DEV = TB.DEV
SENTINEL = TB.SENTINEL
RANGE, RANGE_XY = TB.RANGE, TB.RANGE_XY
NEAR = 40.0
F32 = np.float32

# x, y, z with ((x*x + y*y) + z*z) = 1600 in float32, whose root is 40 exactly, and the floats next to that edge: row 7 sums to the
# float below 1600 (its correctly rounded root is 40.0 again), row 8 to the one below that.  hvpr_point_flags_f32 takes the root
# with the hardware instruction (__fsqrt_rn is the native root in this toolchain, good to one unit in the last place), so on
# these rows it may decide otherwise than numpy does: what is held here is that the batch form decides as IT does, bit for bit.
X32 = np.nextafter(F32(32), F32(0))
EDGE = np.asarray([
    [40.0, 0.0, 0.0], [32.0, 24.0, 0.0], [32.0, -24.0, 0.0], [24.0, 32.0, 0.0], [24.0, 0.0, -32.0],
    [np.nextafter(F32(40), F32(0)), 0.0, 0.0], [np.nextafter(F32(40), F32(100)), 0.0, 0.0],
    [X32, 24.0, 0.0], [np.nextafter(X32, F32(0)), 24.0, 0.0], [np.nextafter(F32(32), F32(100)), 24.0, 0.0],
    [32.0, np.nextafter(F32(-24), F32(0)), 0.0], [32.0, np.nextafter(F32(-24), F32(-100)), 0.0],
], np.float32)


def torch_():
    import torch
    return torch


def frames_with_edges(sizes, seed, F):
    frames, calibs, shapes = TB.make_frames(sizes, "mixed", seed, F=F)
    rng = np.random.RandomState(seed + 1000)
    for p in frames:
        k = rng.rand(len(p)) < 0.15
        p[k, :3] = EDGE[rng.randint(0, len(EDGE), int(k.sum()))]
    return frames, calibs, shapes


def near_flags(points):
    from hvpr_amd import preprocess as PP
    return PP._flags(points.contiguous(), 1, near=NEAR)


SIZE_SETS = {1: [[0], [1], [63], [64], [65], [1023], [1024], [1025], [2049]],
             3: [[1023, 0, 1025], [63, 1, 64], [65, 2049, 0]],
             17: [[1024, 0, 0, 1024, 1, 63, 64, 65, 0, 1023, 1025, 2049, 1, 1, 1, 0, 5]]}


# ------------------------------------------------------------------------------------------------ 1. the count pass
def test_edge_rows_are_on_the_edge(observed):
    torch = torch_()
    sq = (EDGE[:, 0] * EDGE[:, 0] + EDGE[:, 1] * EDGE[:, 1]) + EDGE[:, 2] * EDGE[:, 2]          # IEEE float32, as the kernel sums
    lo = np.nextafter(F32(1600), F32(0))
    assert sq.dtype == np.float32 and (sq[:5] == F32(1600)).all() and sq[7] == lo and sq[8] == np.nextafter(lo, F32(0))
    assert sq[9] > F32(1600) and (np.abs(sq.astype(np.float64) - 1600.0) <= 4e-4).all(), "each within three floats of 1600"
    got = near_flags(torch.from_numpy(np.concatenate([EDGE, np.zeros((len(EDGE), 1), np.float32)], axis=1)).to(DEV)).cpu().numpy()
    assert got[:5].tolist() == [0] * 5 and got[6] == 0 and got[9] == 0, "at or above 40 whatever the last place of the root"
    observed(f"near flags of the edge rows: device {got.tolist()}, numpy {(np.sqrt(sq) < F32(NEAR)).astype(int).tolist()}")


@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("mask", [0, 2, 3])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_count_pass_matches_select_count_and_per_frame_flags(B, mask, F):
    from hvpr_amd import kernels
    torch = torch_()
    assert kernels.ragged_select_tile_rows() == 1024
    for k, sizes in enumerate(SIZE_SETS[B]):
        frames, calibs, shapes = frames_with_edges(sizes, seed=31 * B + k, F=F)
        pts, off, calib = TB.ragged(frames, calibs, shapes, capacity_rows=70, fill=[30.0, 0.5, -1.0] + [0.25] * (F - 3))
        want_off, ws0 = kernels.ragged_select_count(pts, off, mask, calib=calib, range_xy=RANGE_XY)
        kept, _ = kernels.ragged_select_write(pts, off, mask, want_off, ws0, calib=calib, range_xy=RANGE_XY)
        new_off = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
        near_off = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
        kernels.ragged_sample_count(pts, off, mask, calib=calib, range_xy=RANGE_XY, near=NEAR, new_off=new_off, near_off=near_off)
        assert torch.equal(new_off, want_off), (sizes, mask, F)
        o = want_off.cpu().numpy()
        per_frame = [int(near_flags(kept[o[b]: o[b + 1]]).sum().item()) if o[b + 1] > o[b] else 0 for b in range(B)]
        assert near_off.cpu().numpy().tolist() == np.cumsum([0] + per_frame).tolist(), (sizes, mask, F)
        if mask == 0:
            assert o.tolist() == np.cumsum([0] + sizes).tolist()


# ------------------------------------------------------------------------------------------------ 2. the write pass
def hand_made(F, seed=3):
    """Frames, counts and a table: five frames (one empty, two larger than a tile), modes 0 and 1 in one call, sources with no,
    one and two destinations, every frame's last output row named."""
    from hvpr_amd import kernels
    torch = torch_()
    T, P = kernels.ragged_select_tile_rows(), 700
    sizes, mode = [T + 37, 0, 300, 2 * T + 5, 90], np.asarray([0, 1, 1, 1, 0], np.int32)
    frames, calibs, shapes = frames_with_edges(sizes, seed=seed, F=F)
    pts, off, calib = TB.ragged(frames, calibs, shapes)
    new_off, near_off, ws = kernels.ragged_sample_count(pts, off, 2, range_xy=RANGE_XY, near=NEAR)
    sel_off, ws0 = kernels.ragged_select_count(pts, off, 2, range_xy=RANGE_XY)
    kept, _ = kernels.ragged_select_write(pts, off, 2, sel_off, ws0, range_xy=RANGE_XY)
    o = new_off.cpu().numpy()
    kept_h = kept[: o[-1]].cpu().numpy()
    near = near_flags(kept[: o[-1]]).cpu().numpy().astype(bool)
    rng = np.random.RandomState(seed)
    dest = np.full((o[-1], 2), -1, np.int32)
    rows = []                                       # (frame, source ordinal, slot, destination, kept row)
    for b in range(len(sizes)):
        n = int(o[b + 1] - o[b])
        if n == 0:
            continue
        fl = near[o[b]: o[b + 1]]
        row_of = np.arange(n) if mode[b] == 0 else np.concatenate((np.where(fl)[0], np.where(~fl)[0]))
        if mode[b] == 1:
            assert 0 < fl.sum() < n, "a mode 1 frame with near and far rows"
        m = min(P, n + n // 3)
        outs = np.r_[rng.permutation(P - 1)[: m - 1], P - 1]            # distinct, the last row among them
        first = rng.permutation(n)[: min(n - n // 5, m)]                # a fifth of the sources go nowhere
        second = rng.permutation(first)[: m - len(first)]
        for slot, srcs, ds in ((0, first, outs[: len(first)]), (1, second, outs[len(first):])):
            dest[o[b] + srcs, slot] = ds
            rows += [(b, int(s), slot, int(d), int(o[b] + row_of[s])) for s, d in zip(srcs, ds)]
    assert (dest[:, 1] >= 0).sum() > 100 and ((dest[:, 0] < 0) & (dest[:, 1] < 0)).sum() > 100
    return {"pts": pts, "off": off, "new_off": new_off, "near_off": near_off, "ws": ws, "mode": torch.from_numpy(mode).to(DEV),
            "dest": dest, "rows": rows, "kept": kept_h, "P": P, "B": len(sizes), "F": F}


def expected(h, batch_column, guard, skip=()):
    W = h["F"] + (1 if batch_column else 0)
    out = np.full((h["B"] * h["P"] + guard, W), SENTINEL, np.float32)
    for k, (b, s, slot, d, row) in enumerate(h["rows"]):
        if k in skip:
            continue
        out[b * h["P"] + d] = np.r_[F32(b), h["kept"][row]] if batch_column else h["kept"][row]
    return out


def write(h, dest, batch_column, capacity=None, guard=32):
    from hvpr_amd import kernels
    torch = torch_()
    W = h["F"] + (1 if batch_column else 0)
    rows = h["B"] * h["P"] if capacity is None else capacity
    buf = torch.full((h["B"] * h["P"] + guard, W), SENTINEL, dtype=torch.float32, device=DEV)
    _, flag = kernels.ragged_sample_write(h["pts"], h["off"], 2, h["new_off"], h["near_off"], h["mode"],
                                          torch.from_numpy(np.ascontiguousarray(dest)).to(DEV), h["P"], h["ws"], range_xy=RANGE_XY,
                                          near=NEAR, batch_column=batch_column, out=buf[:rows])
    return buf.cpu().numpy(), int(flag.item())


@pytest.mark.parametrize("F,batch_column", [(4, True), (4, False), (5, True)])
def test_write_pass_follows_the_table_byte_for_byte(F, batch_column):
    h = hand_made(F)
    want = expected(h, batch_column, 32)
    got, flag = write(h, h["dest"], batch_column)
    assert flag == 0 and got.tobytes() == want.tobytes()
    if batch_column:
        named = want[:, 0] != SENTINEL
        assert (want[named, 0] == (np.nonzero(named)[0] // h["P"]).astype(np.float32)).all() and named.sum() == len(h["rows"])
    again, flag = write(h, h["dest"], batch_column)
    assert flag == 0 and again.tobytes() == got.tobytes(), "a second run gives the same bytes"


def test_bad_destinations_and_a_short_output_flag_and_touch_nothing_else():
    h = hand_made(4)
    P, B = h["P"], h["B"]
    for value in (P, P + 5, 2 ** 31 - 1, -2, -(2 ** 31)):
        for k in (7, len(h["rows"]) - 3):                          # an entry of the first frame (mode 0), one of the last
            b, s, slot, d, row = h["rows"][k]
            bad = h["dest"].copy()
            bad[int(h["new_off"][b].item()) + s, slot] = value
            got, flag = write(h, bad, True)
            assert flag == 1 and got.tobytes() == expected(h, True, 32, skip=(k,)).tobytes(), (value, k)
    # an output one row short: the one store that names the last row is dropped
    last = [k for k, r in enumerate(h["rows"]) if r[0] == B - 1 and r[3] == P - 1]
    assert len(last) == 1
    got, flag = write(h, h["dest"], True, capacity=B * P - 1)
    assert flag == 1 and got.tobytes() == expected(h, True, 32, skip=last).tobytes()
    # a short table: the rows past it are dropped
    n_short = int(h["new_off"][B - 1].item())
    got, flag = write(h, h["dest"][:n_short], True)
    assert flag == 1 and got.tobytes() == expected(h, True, 32, skip=[k for k, r in enumerate(h["rows"]) if r[0] == B - 1]).tobytes()
    # a mode word that is neither 0 nor 1 drops its frame
    torch = torch_()
    keep = h["mode"]
    h["mode"] = torch.tensor([0, 1, 7, 1, 0], dtype=torch.int32, device=DEV)
    got, flag = write(h, h["dest"], True)
    h["mode"] = keep
    assert flag == 1 and got.tobytes() == expected(h, True, 32, skip=[k for k, r in enumerate(h["rows"]) if r[0] == 2]).tobytes()


# ------------------------------------------------------------------------------------------------ 3. DeviceBatchLoader on G23
@pytest.fixture(scope="module")
def g23():
    import batch_loader_cases as BC
    import sample_batch_cases as SC
    torch = torch_()
    z = SC.g23()
    bank = BC.g22_bank(z, device=DEV)
    bank.on_device()
    frames = BC.g22_frames(z, to_device=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return {"z": z, "bank": bank, "frames": frames, "cfg": SC.g23_config(z), "classes": [str(c) for c in z["class_names"]],
            "P": int(z["num_sample_points"])}


def make_loader(g23, training, **kw):
    from hvpr_amd.batch_loader import DeviceBatchLoader
    return DeviceBatchLoader(g23["cfg"], g23["classes"], lambda i: g23["frames"][i], len(g23["frames"]), bank=g23["bank"],
                             training=training, sample_points=True, **kw)


def check_shape(batch, B, P):
    assert batch["points"].shape == (B * P, 5) and batch["batch_size"] == B and int(batch["overflow"].item()) == 0
    assert batch["point_frame_offsets"].cpu().numpy().tolist() == (np.arange(B + 1) * P).tolist()
    assert batch["points"][:, 0].cpu().numpy().tolist() == np.repeat(np.arange(B), P).astype(np.float32).tolist()


def test_loader_reproduces_g23_train(g23, observed):
    import batch_loader_cases as BC
    import sample_batch_cases as SC
    z, P = g23["z"], g23["P"]
    loader = make_loader(g23, True, debug_choices=True)
    gens = SC.g23_generators(z, "train")
    batch = loader.prepare_batch(z["train.indices"].tolist(), gens)
    BC.assert_same_batch(z["train.points"], z["train.gt_boxes"], batch["points"].cpu().numpy(), batch["gt_boxes"].cpu().numpy(),
                         observed, "G23 device")
    check_shape(batch, 2, P)
    assert batch["redraw_index"] == {} and loader.reads == 3, "two reads and the one the debug argument costs"
    for b in range(2):
        assert np.array_equal(batch["choices"][b], z[f"train.b{b}.choice"]), ("choice", b)
        assert np.array_equal(batch["permutations"][b], z[f"train.b{b}.perm"]), ("permutation", b)
        assert SC.state_matches(gens[b], z, "train", b), ("generator state after the frame", b)
    assert batch["num_boxes"].tolist() == [int(z[f"train.b{b}.num_boxes"]) for b in range(2)]


def test_loader_reproduces_g23_test_mode(g23):
    import sample_batch_cases as SC
    z, P = g23["z"], g23["P"]
    loader = make_loader(g23, False, debug_choices=True)
    gens = SC.g23_generators(z, "test")
    batch = loader.prepare_batch(z["test.indices"].tolist(), gens)
    got = batch["points"].cpu().numpy()
    assert got.shape == z["test.points"].shape and got.tobytes() == z["test.points"].tobytes()
    gt = batch["gt_boxes"].cpu().numpy()
    assert gt.shape == z["test.gt_boxes"].shape and gt.tobytes() == z["test.gt_boxes"].tobytes()
    check_shape(batch, 4, P)
    assert batch["permutations"] == [] and loader.reads == 2
    for b in range(4):
        assert np.array_equal(batch["choices"][b], z[f"test.b{b}.choice"]), ("choice", b)
        assert SC.state_matches(gens[b], z, "test", b), ("generator state after the frame", b)


def test_choices_are_not_computed_unless_asked_for(g23):
    loader = make_loader(g23, False)
    batch = loader.prepare_batch(g23["z"]["test.indices"].tolist(), np.random.RandomState(4))
    assert "choices" not in batch and loader.reads == 1


def test_refusal_is_raised_for_a_frame_the_reference_refuses(g23):
    """Frame 5 has exactly P far rows: with P - 1 the reference refuses it."""
    import copy
    from hvpr_amd.batch_loader import DeviceBatchLoader
    cfg = copy.deepcopy(g23["cfg"])
    cfg["DATA_PROCESSOR"][1]["NUM_POINTS"]["test"] = g23["P"] - 1
    loader = DeviceBatchLoader(cfg, g23["classes"], lambda i: g23["frames"][i], 6, training=False, sample_points=True)
    with pytest.raises(ValueError):
        loader.prepare_batch([2, 5], np.random.RandomState(1))
    assert loader.prepare_batch([2, 4], np.random.RandomState(1))["points"].shape[0] == 2 * (g23["P"] - 1)


def test_single_generator_order_matches_the_restatement(g23, observed):
    """One generator for the batch: the augmentor draws of all frames, then per frame the sample draws and the permutation."""
    import batch_loader_cases as BC
    import sample_batch_cases as SC
    from hvpr_amd.augment import AugmentPlanner
    z, P, indices = g23["z"], g23["P"], [0, 1, 1, 0]
    loader = make_loader(g23, True, debug_choices=True)
    gen, ref = np.random.RandomState(2), np.random.RandomState(2)
    batch = loader.prepare_batch(indices, gen)
    host_bank = BC.g22_bank(z, device="cpu")
    planner = AugmentPlanner(g23["cfg"]["DATA_AUGMENTOR"], g23["classes"], host_bank)
    points, gt, slots = SC.prepare_batch_host(BC.g22_frames(z), indices, planner, host_bank, [ref] * 4, z["range"], 6, P)
    r64 = z["range"].astype(np.float64)
    for s in slots:                                                  # the margins the comparison leans on, in float64
        xy = s["r"]["points"][:, :2].astype(np.float64)
        assert min(np.abs(xy - r64[0:2]).min(), np.abs(xy - r64[3:5]).min()) >= 1e-3 and len(s["items"]) == 1
        assert np.abs(np.sqrt((s["kept"][:, :3].astype(np.float64) ** 2).sum(axis=1)) - NEAR).min() >= 1e-3
    BC.assert_same_batch(points, gt, batch["points"].cpu().numpy(), batch["gt_boxes"].cpu().numpy(), observed, "G23 single generator")
    for b, s in enumerate(slots):
        assert np.array_equal(batch["choices"][b], s["choice"]) and np.array_equal(batch["permutations"][b], s["perm"]), b
    assert np.array_equal(gen.get_state()[1], ref.get_state()[1]) and gen.get_state()[2] == ref.get_state()[2]
    check_shape(batch, 4, P)


def test_spliced_batch_knows_its_counts_without_a_read(g23):
    """The redraw path (no frame of G23 is redrawn, so the splice is made by hand): the spliced batch's host-known kept and near
    counts are what the fresh count pass over it finds, and it is sampled like any other."""
    loader = make_loader(g23, True)
    gen = np.random.RandomState(2)
    st = loader._augment_stage([g23["frames"][i] for i in (0, 1, 1)], [gen] * 3)
    sub = loader._augment_stage([g23["frames"][0]], [gen])
    reads = loader.reads
    spliced = loader._splice(st, {1: sub})
    assert loader.reads == reads
    for host, dev in (("new_off", "new_off_dev"), ("near_off", "near_off_dev")):
        assert spliced[host].tolist() == spliced[dev].cpu().numpy().tolist(), host
        want = [st[host][1] - st[host][0], sub[host][1] - sub[host][0], st[host][3] - st[host][2]]
        assert np.diff(spliced[host]).tolist() == want, host
    assert 0 < spliced["near_off"][-1] < spliced["new_off"][-1]
    batch = loader._finish_sampled(spliced["frames"], spliced["points"], spliced["aug_off_dev"], 2, spliced["new_off_dev"],
                                   spliced["near_off_dev"], spliced["new_off"], spliced["near_off"], spliced["ws"], [gen] * 3)
    check_shape(batch, 3, g23["P"])


# ------------------------------------------------------------------------------------------------ 4. against the per-frame chain
def chain_batch(g23, indices, rng, training):
    """compact_rows -> PointPreprocessor.sample_points -> preprocess.shuffle_points -> batch column, frame by frame."""
    from hvpr_amd import preprocess as PP
    from hvpr_amd.augment import DeviceAugmentor
    torch = torch_()
    z, P = g23["z"], g23["P"]
    pre = PP.PointPreprocessor(z["range"], num_points=P, training=training)
    frames = [dict(g23["frames"][i]) for i in indices]
    for f in frames:
        f["points"] = TB.chain_frame(f["points"], 1, f["calib"], f["image_shape"])
    if training:
        out = DeviceAugmentor(g23["cfg"]["DATA_AUGMENTOR"], g23["classes"], g23["bank"], z["range"])(frames, rng)
        off = np.cumsum([0] + out["num_points"].tolist())
        per = [out["points"][off[b]: off[b + 1]].contiguous() for b in range(len(frames))]
    else:
        per = [f["points"] for f in frames]
    parts = []
    for b, p in enumerate(per):
        kept, count = PP.compact_rows(p, PP.mask_points_by_range(p, z["range"]))
        p = pre.sample_points(kept[: int(count.item())], rng)
        if training:
            p = PP.shuffle_points(p, rng)
        parts.append(torch.cat([torch.full((p.shape[0], 1), float(b), device=DEV), p], dim=1))
    return {"points": torch.cat(parts).contiguous(), "batch_size": len(frames)}, (out["gt_boxes"] if training else None)


def test_training_batch_is_the_per_frame_chain_bit_for_bit_and_voxelizes_alike(g23):
    torch = torch_()
    indices = [0, 1, 1, 0]
    loader = make_loader(g23, True)
    batch = loader.prepare_batch(indices, np.random.RandomState(7))
    assert batch["redraw_index"] == {}
    chain, gt = chain_batch(g23, indices, np.random.RandomState(7), True)
    assert torch.equal(TB.bits(chain["points"]), TB.bits(batch["points"]))
    assert torch.equal(gt[:, : batch["gt_boxes"].shape[1]], batch["gt_boxes"])
    check_shape(batch, 4, g23["P"])
    got, want = TB.voxelize_on_device(batch, g23["z"]["range"]), TB.voxelize_on_device(chain, g23["z"]["range"])
    assert got[0].shape[0] > 100
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g.contiguous().view(torch.int32), w.contiguous().view(torch.int32))


def test_test_batch_is_the_per_frame_chain_bit_for_bit(g23):
    torch = torch_()
    indices = g23["z"]["test.indices"].tolist()
    batch = make_loader(g23, False).prepare_batch(indices, np.random.RandomState(9))
    chain, _ = chain_batch(g23, indices, np.random.RandomState(9), False)
    assert torch.equal(TB.bits(chain["points"]), TB.bits(batch["points"]))


# ------------------------------------------------------------------------------------------------ 5. reads
def test_training_batch_reads_twice_test_batch_once(g23):
    torch = torch_()
    loader = make_loader(g23, True)
    loader.prepare_batch([0, 1, 1, 0], np.random.RandomState(5))          # first use: allocations, pinned buffers
    torch.cuda.synchronize()
    reads0 = loader.reads
    batch, syncs = TB.run_counting_syncs(loader, lambda: loader.prepare_batch([0, 1, 1, 0], np.random.RandomState(2)))
    assert batch["redraw_index"] == {} and batch["points"].shape[0] == 4 * g23["P"]
    assert syncs == 2 and loader.reads - reads0 == 2
    tester = make_loader(g23, False)
    tester.prepare_batch([2, 3, 4, 5], np.random.RandomState(1))
    torch.cuda.synchronize()
    batch, syncs = TB.run_counting_syncs(tester, lambda: tester.prepare_batch([5, 4, 3, 2], np.random.RandomState(2)))
    assert syncs == 1 and tester.reads == 2 and batch["points"].shape[0] == 4 * g23["P"]
