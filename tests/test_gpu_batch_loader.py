"""GPU: the ragged select / shuffle / collate kernels (csrc/collate.hip) and DeviceBatchLoader.

The kernels are compared BIT FOR BIT with the per-frame chain that existed before them (hvpr_point_flags_f32 +
hvpr_compact_rows_f32 per frame, hvpr_gather_rows_f32 for a permutation): the keep decision is one shared expression
(csrc/point_pred.h), so the same rows must survive in the same order with the same bits, with no margin, also for points exactly
on a range bound or on the image border.  The border case uses a dyadic calibration (a pure axis permutation, focal length 512,
principal point (640, 192), image 384 x 1280): x = 4, y = 5 projects to u = (512 * -5 + 640 * 4) / 4 = 0 exactly, y = -5 to
u = 1280 = the image width exactly, z = +-1.5 to v = 0 and v = 384 exactly, so the expected decisions are known as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.5
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
RANGE = np.asarray([0.0, -39.68, -3.0, 69.12, 39.68, 1.0], np.float32)
RANGE_XY = RANGE[[0, 1, 3, 4]]


def torch_():
    import torch
    return torch


def tile_():
    from hvpr_amd import kernels
    return kernels.ragged_select_tile_rows()


def size_cases():
    T = tile_()
    rng = np.random.RandomState(5)
    return {"empty": [0], "one": [1], "tile": [T], "tile+1": [T + 1], "boundary_in_tile": [T - 1, 2],
            "boundaries_in_wave": [1, 1, 1, 0, 2], "leading_empty": [0, 0, 5], "multi_tile": [3 * T + 17, 0, T],
            "64_frames": list(rng.randint(1, 4, size=64)),
            "tiles_past_a_wave": [40 * T + 3, 30 * T + 1]}      # 72 tile counts: the scan's second wave gets live pieces


SIZE_NAMES = ["empty", "one", "tile", "tile+1", "boundary_in_tile", "boundaries_in_wave", "leading_empty", "multi_tile", "64_frames",
              "tiles_past_a_wave"]


def kitti_calib(b):
    """A KITTI-like calibration, a little different per frame (so that a row judged with its neighbour's calibration shows)."""
    P2 = np.asarray([[721.5377 + b, 0.0, 609.5593, 44.85728], [0.0, 721.5377 + b, 172.854 - b, 0.2163791],
                     [0.0, 0.0, 1.0, 0.002745884]], np.float32)
    R0 = np.asarray([[0.9999239, 0.00983776, -0.00744505], [-0.0098698, 0.9999421, -0.00427846],
                     [0.00740253, 0.00435161, 0.9999631]], np.float32)
    V2C = np.asarray([[0.00753374, -0.9999714, -0.00061660, -0.00406977], [0.01480249, 0.00072807, -0.9998902, -0.07631618],
                      [0.9998621, 0.00752379, 0.01480755, -0.2717806]], np.float32)
    return {"Tr_velo2cam": V2C, "R0": R0, "P2": P2}, (375 - (b % 3), 1242 - (b % 2))


def dyadic_calib():
    P2 = np.asarray([[512.0, 0.0, 640.0, 0.0], [0.0, 512.0, 192.0, 0.0], [0.0, 0.0, 1.0, 0.0]], np.float32)
    V2C = np.asarray([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]], np.float32)
    return {"Tr_velo2cam": V2C, "R0": np.eye(3, dtype=np.float32), "P2": P2}, (384, 1280)


BORDER = np.asarray([  # x, y, z, intensity, in range?, in image?
    [4.0, 5.0, 0.0, 0.1, 1, 1],        # u = 0: inside
    [4.0, -5.0, 0.0, 0.2, 1, 0],       # u = 1280 = width: outside
    [4.0, 0.0, 1.5, 0.3, 1, 1],        # v = 0: inside
    [4.0, 0.0, -1.5, 0.4, 1, 0],       # v = 384 = height: outside
    [0.0, 0.0, 0.0, 0.5, 1, 0],        # x on the lower bound; rect depth 0: u is 0/0, not inside
    [69.12, 1.0, 0.0, 0.6, 1, 1],      # x on the upper bound
    [8.0, -39.68, 0.0, 0.7, 1, 0],     # y on the lower bound
    [8.0, 39.68, 0.0, 0.8, 1, 0],      # y on the upper bound
    [np.nextafter(np.float32(69.12), np.float32(100)), 1.0, 0.0, 0.9, 0, 1],
    [8.0, np.nextafter(np.float32(-39.68), np.float32(-100)), 0.0, 1.0, 0, 0],
    [-4.0, 1.0, 0.0, 1.1, 0, 0],       # behind the camera
], np.float64)


def make_frames(sizes, kind, seed, F=4):
    """(frames, calibs, shapes): float32 (n, F) per frame."""
    rng = np.random.RandomState(seed)
    frames, calibs, shapes = [], [], []
    for b, n in enumerate(sizes):
        c, s = dyadic_calib() if kind == "border" else kitti_calib(b)
        p = np.zeros((n, F), np.float32)
        p[:, 3:] = rng.rand(n, F - 3)
        if kind == "mixed":
            p[:, 0], p[:, 1], p[:, 2] = rng.uniform(-10, 80, n), rng.uniform(-45, 45, n), rng.uniform(-3, 1, n)
        elif kind == "all":            # in range and well inside the image
            p[:, 0], p[:, 1], p[:, 2] = rng.uniform(20, 60, n), rng.uniform(-4, 4, n), rng.uniform(-1.5, 0.0, n)
        elif kind == "none":           # behind the sensor and out of range
            p[:, 0], p[:, 1], p[:, 2] = rng.uniform(-60, -20, n), rng.uniform(50, 60, n), rng.uniform(-3, 1, n)
        elif kind == "border":         # column 3 names the BORDER row: k / 16
            k = rng.randint(0, len(BORDER), n)
            p[:, :3], p[:, 3] = BORDER[k, :3], k / 16.0
        frames.append(p)
        calibs.append(c)
        shapes.append(s)
    return frames, calibs, shapes


def chain_frame(points, mask, calib, shape):
    """The per-frame chain: flags + stable compaction, one frame, with its host read."""
    from hvpr_amd import preprocess as PP
    torch = torch_()
    if points.shape[0] == 0:
        return points
    if mask == 2:
        flags = PP.mask_points_by_range(points, RANGE)
    elif mask == 1:
        flags = PP.get_fov_flag(points, calib, shape)
    else:
        a, p = PP.fov_matrices(calib, points.device)
        flags = PP._flags(points.contiguous(), 0, torch.from_numpy(RANGE_XY.copy()).to(points.device),
                          fov=(a, p, (int(shape[0]), int(shape[1]))))
    out, count = PP.compact_rows(points, flags)
    return out[: int(count.item())]


def ragged(frames, calibs, shapes, capacity_rows=0, fill=None):
    from hvpr_amd import eval_loop
    torch = torch_()
    F = frames[0].shape[1]
    parts = list(frames)
    if capacity_rows:
        parts.append(np.tile(np.asarray(fill, np.float32), (capacity_rows, 1)))
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts).reshape(-1, F))).to(DEV)
    off = torch.from_numpy(np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)).to(DEV)
    calib = torch.from_numpy(eval_loop.pack_calib(calibs, shapes)).to(DEV)
    return pts, off, calib


def select(pts, off, calib, mask, **kw):
    from hvpr_amd import kernels
    new_off, ws = kernels.ragged_select_count(pts, off, mask, calib=calib, range_xy=RANGE_XY)
    out, flag = kernels.ragged_select_write(pts, off, mask, new_off, ws, calib=calib, range_xy=RANGE_XY, **kw)
    return new_off, out, flag


def bits(t):
    return t.contiguous().view(torch_().int32)


# ------------------------------------------------------------------------------------------------ 1. against the per-frame chain
@pytest.mark.parametrize("case", SIZE_NAMES)
def test_select_matches_per_frame_chain_bitwise(case):
    torch = torch_()
    sizes = size_cases()[case]
    for kind in ("mixed", "all", "none", "border"):
        frames, calibs, shapes = make_frames(sizes, kind, seed=len(sizes) + sum(sizes))
        pts, off, calib = ragged(frames, calibs, shapes)
        dev_frames = [torch.from_numpy(f).to(DEV) for f in frames]
        for mask in (1, 2, 3):
            want = [chain_frame(f, mask, c, s) for f, c, s in zip(dev_frames, calibs, shapes)]
            want_off = np.cumsum([0] + [int(w.shape[0]) for w in want])
            new_off, out, flag = select(pts, off, calib, mask)
            assert new_off.cpu().numpy().tolist() == want_off.tolist(), (case, kind, mask)
            assert int(flag.item()) == 0
            got = out[: want_off[-1]]
            exp = torch.cat(want) if want else got
            assert torch.equal(bits(got), bits(exp)), (case, kind, mask)
            if kind == "all":
                assert want_off[-1] == sum(sizes)
            if kind == "none":
                assert want_off[-1] == 0
            if kind == "border" and sum(sizes):
                allp = np.concatenate(frames)
                row = np.rint(allp[:, 3] * 16).astype(int)
                keep = np.ones(len(allp), bool)
                if mask & 2:
                    keep &= BORDER[row, 4] == 1
                if mask & 1:
                    keep &= BORDER[row, 5] == 1
                assert int(want_off[-1]) == int(keep.sum()), (case, mask)


def test_select_other_row_widths_and_batch_column():
    """F = 3, 5, 8 take the scalar row copy; the batch column in front of a row is the frame index."""
    torch = torch_()
    T = tile_()
    for F in (3, 5, 8):
        frames, calibs, shapes = make_frames([T + 3, 0, 70], "mixed", seed=F, F=F)
        pts, off, calib = ragged(frames, calibs, shapes)
        want = [chain_frame(torch.from_numpy(f).to(DEV), 3, c, s) for f, c, s in zip(frames, calibs, shapes)]
        new_off, out, flag = select(pts, off, calib, 3, batch_column=True)
        n = [int(w.shape[0]) for w in want]
        assert new_off.cpu().numpy().tolist() == np.cumsum([0] + n).tolist() and int(flag.item()) == 0
        got = out[: sum(n)]
        assert torch.equal(bits(got[:, 1:]), bits(torch.cat(want)))
        assert got[:, 0].cpu().numpy().tolist() == np.repeat(np.arange(3), n).astype(np.float32).tolist()


# ------------------------------------------------------------------------------------------------ 2. capacity rows
def test_capacity_rows_are_ignored():
    torch = torch_()
    T = tile_()
    frames, calibs, shapes = make_frames([T - 5, 40], "mixed", seed=2)
    inside = [30.0, 0.5, -1.0, 0.25]                       # in range and inside the image of every calibration used here
    pts0, off, calib = ragged(frames, calibs, shapes)
    pts1, _, _ = ragged(frames, calibs, shapes, capacity_rows=2 * T, fill=inside)
    for mask in (1, 2, 3):
        off0, out0, _ = select(pts0, off, calib, mask)
        n = int(off0[-1].item())
        assert 0 < n < T + 35
        out = torch.full((pts1.shape[0], 4), SENTINEL, dtype=torch.float32, device=DEV)
        off1, out1, flag = select(pts1, off, calib, mask, out=out)
        assert torch.equal(off0, off1) and int(flag.item()) == 0
        assert torch.equal(bits(out1[:n]), bits(out0[:n]))
        assert bool((out1[n:] == SENTINEL).all())
        # and the fill rows WOULD have been kept
        keep_off, _, _ = select(pts1, torch.tensor([0, pts1.shape[0]], dtype=torch.int32, device=DEV), calib[:1].contiguous(), mask)
        assert int(keep_off[-1].item()) >= 2 * T


# ------------------------------------------------------------------------------------------------ 3. inv_perm
def _perms(counts, how, seed=0):
    rng = np.random.RandomState(seed)
    if how == "identity":
        return [np.arange(m) for m in counts]
    if how == "reverse":
        return [np.arange(m)[::-1].copy() for m in counts]
    return [rng.permutation(m) for m in counts]


def _inverse(perms):
    inv = []
    for p in perms:
        q = np.empty(len(p), np.int64)
        q[p] = np.arange(len(p))
        inv.append(q)
    return np.concatenate(inv).astype(np.int32) if inv else np.zeros((0,), np.int32)


@pytest.mark.parametrize("how", ["identity", "reverse", "seeded"])
def test_inv_perm_places_rows_like_a_gather(how):
    from hvpr_amd import kernels, preprocess as PP
    torch = torch_()
    T = tile_()
    frames, calibs, shapes = make_frames([3 * T + 9, 0, 33, T], "mixed", seed=11)
    pts, off, calib = ragged(frames, calibs, shapes)
    new_off, ws = kernels.ragged_select_count(pts, off, 2, calib=calib, range_xy=RANGE_XY)
    compacted, _ = kernels.ragged_select_write(pts, off, 2, new_off, ws, calib=calib, range_xy=RANGE_XY)
    o = new_off.cpu().numpy()
    counts = np.diff(o)
    assert counts[1] == 0 and counts.min() == 0 and counts[0] > T
    perms = _perms(counts, how, seed=3)
    inv = torch.from_numpy(_inverse(perms)).to(DEV)
    out = torch.full((int(o[-1]) + 64, 5), SENTINEL, dtype=torch.float32, device=DEV)
    _, flag = kernels.ragged_select_write(pts, off, 2, new_off, ws, calib=calib, range_xy=RANGE_XY, inv_perm=inv, batch_column=True,
                                          out=out)
    assert int(flag.item()) == 0
    for b in range(4):
        seg = out[o[b]: o[b + 1]]
        want = PP.gather_rows(compacted[o[b]: o[b + 1]], torch.from_numpy(perms[b].astype(np.int32)).to(DEV)) if counts[b] else seg[:, 1:]
        assert torch.equal(bits(seg[:, 1:]), bits(want)), (how, b)
        assert bool((seg[:, 0] == float(b)).all())
    assert bool((out[o[-1]:] == SENTINEL).all())


def test_bad_inv_perm_and_small_output_flag_and_stay_inside():
    from hvpr_amd import kernels
    torch = torch_()
    T = tile_()
    frames, calibs, shapes = make_frames([T + 50, 200], "all", seed=4)
    pts, off, calib = ragged(frames, calibs, shapes)
    new_off, ws = kernels.ragged_select_count(pts, off, 2, range_xy=RANGE_XY)
    o = new_off.cpu().numpy()
    n = int(o[-1])
    assert n == T + 250
    good = _inverse(_perms(np.diff(o), "seeded", seed=8))

    def run(inv, rows):
        buf = torch.full((rows + 32, 5), SENTINEL, dtype=torch.float32, device=DEV)          # 32 guard rows behind the output
        _, flag = kernels.ragged_select_write(pts, off, 2, new_off, ws, range_xy=RANGE_XY, inv_perm=torch.from_numpy(inv).to(DEV),
                                              batch_column=True, out=buf[:rows])
        return buf, int(flag.item())

    buf, flag = run(good, n)
    assert flag == 0 and bool((buf[:n] != SENTINEL).all()) and bool((buf[n:] == SENTINEL).all())
    # an entry past its frame (frame 1 has 200 rows), a negative one, and one that would land in the other frame
    for where, value in ((T + 60, 200), (3, -1), (5, T + 50)):
        bad = good.copy()
        bad[where] = value
        buf, flag = run(bad, n)
        dest = o[0 if where < o[1] else 1] + good[where]
        assert flag == 1
        assert bool((buf[dest] == SENTINEL).all()), "the dropped row's slot stays untouched"
        assert int((buf[:n, 0] != SENTINEL).sum().item()) == n - 1 and bool((buf[n:] == SENTINEL).all())
    # an undersized output: rows past it are dropped and flagged
    buf, flag = run(good, n - 100)
    assert flag == 1 and bool((buf[n - 100:] == SENTINEL).all())
    assert int((buf[: n - 100, 0] != SENTINEL).sum().item()) == n - 100
    # a short inv_perm: ranks past it are dropped and flagged
    buf, flag = run(good[: T], n)
    assert flag == 1 and int((buf[:n, 0] != SENTINEL).sum().item()) == T


# ------------------------------------------------------------------------------------------------ 4. argument checks
def test_argument_checks_refuse_without_launching():
    from hvpr_amd import _lib, kernels
    torch = torch_()
    L = _lib.lib()
    frames, calibs, shapes = make_frames([100, 20], "mixed", seed=6)
    pts, off, calib = ragged(frames, calibs, shapes)
    rxy = RANGE_XY.copy()
    need = L.hvpr_ragged_select_workspace_bytes(120, 2)
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    new_off = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((120, 5), SENTINEL, dtype=torch.float32, device=DEV)
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def count(**o):
        a = dict(points=pts.data_ptr(), rows=120, F=4, off=off.data_ptr(), B=2, mask=3, calib=calib.data_ptr(),
                 range_xy=rxy.ctypes.data, new_off=new_off.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        assert set(o) <= set(a)
        a.update(o)
        return L.hvpr_ragged_select_count_f32(*a.values(), st)

    def write(**o):
        a = dict(points=pts.data_ptr(), rows=120, F=4, off=off.data_ptr(), B=2, mask=3, calib=calib.data_ptr(),
                 range_xy=rxy.ctypes.data, new_off=new_off.data_ptr(), inv_perm=None, n_perm=0, batch_column=1, out=out.data_ptr(),
                 cap=120, flag=flag.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        assert set(o) <= set(a)
        a.update(o)
        return L.hvpr_ragged_select_write_f32(*a.values(), st)

    for fn in (count, write):
        assert fn(rows=-1) == INVALID
        assert fn(F=2) == INVALID
        assert fn(B=0) == INVALID
        assert fn(mask=4) == INVALID and fn(mask=-1) == INVALID
        assert fn(off=None) == INVALID
        assert fn(points=None) == INVALID
        assert fn(calib=None) == INVALID and fn(range_xy=None) == INVALID
        assert fn(ws=None) == INVALID
        assert fn(ws_bytes=need - 1) == WORKSPACE
        assert fn(B=1025) == UNSUPPORTED
        assert fn(rows=2 ** 31 - 1) == UNSUPPORTED
        assert fn(new_off=None) == INVALID
    assert count(calib=None, mask=2) == 0                                  # the range alone needs no calibration
    assert write(flag=None) == INVALID and write(cap=-1) == INVALID and write(out=None) == INVALID and write(n_perm=-1) == INVALID
    torch.cuda.synchronize()
    # only the one accepted count call above (mask 2 without a calibration) wrote anything
    assert bool((out == SENTINEL).all()) and int(flag.item()) == 0
    assert new_off.cpu().numpy()[0] == 0
    assert kernels.ragged_select_tile_rows() > 0


# ------------------------------------------------------------------------------------------------ 5. DeviceBatchLoader on G22
@pytest.fixture(scope="module")
def g22():
    import batch_loader_cases as BC
    torch = torch_()
    z = BC.g22()
    bank = BC.g22_bank(z, device=DEV)
    bank.on_device()
    frames = BC.g22_frames(z, to_device=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return {"z": z, "bank": bank, "frames": frames, "cfg": BC.g22_config(z), "classes": [str(c) for c in z["class_names"]]}


def make_loader(g22, training, cfg=None):
    from hvpr_amd.batch_loader import DeviceBatchLoader
    return DeviceBatchLoader(cfg or g22["cfg"], g22["classes"], lambda i: g22["frames"][i], len(g22["frames"]), bank=g22["bank"],
                             training=training)


def test_loader_reproduces_g22_train(g22, observed):
    import batch_loader_cases as BC
    z = g22["z"]
    loader = make_loader(g22, True)
    gens = BC.g22_generators(z)
    batch = loader.prepare_batch(z["train.indices"].tolist(), gens)
    BC.assert_train_batch_is_g22(z, batch["points"].cpu().numpy(), batch["gt_boxes"].cpu().numpy(), observed, "device")
    items = [z[f"train.b{b}.items"].tolist() for b in range(4)]
    assert batch["redraw_index"] == {3: items[3][1:]}, "the redraw index"
    for b in range(4):
        assert np.array_equal(batch["permutations"][b], z[f"train.b{b}.perm"]), ("permutation", b)
        assert BC.state_matches(gens[b], z, b), ("generator state after the frame", b)
    n = [int(z[f"train.b{b}.num_points"]) for b in range(4)]
    assert batch["point_frame_offsets"].cpu().numpy().tolist() == np.cumsum([0] + n).tolist()
    assert batch["num_boxes"].tolist() == [int(z[f"train.b{b}.num_boxes"]) for b in range(4)]
    assert batch["batch_size"] == 4 and int(batch["overflow"].item()) == 0
    assert batch["frame_id"] == ["0", "1", "2", str(items[3][-1])] and len(batch["calib"]) == len(batch["image_shape"]) == 4


def test_loader_reproduces_g22_test_mode(g22):
    z = g22["z"]
    loader = make_loader(g22, False)
    state = np.random.RandomState(3)
    before = state.get_state()[1].copy()
    batch = loader.prepare_batch(z["train.indices"].tolist(), state)
    assert loader.reads == 1
    assert np.array_equal(before, state.get_state()[1]), "test mode draws nothing"
    got = batch["points"].cpu().numpy()
    assert got.shape == z["test.points"].shape and got.tobytes() == z["test.points"].tobytes()
    gt = batch["gt_boxes"].cpu().numpy()
    assert gt.shape == z["test.gt_boxes"].shape and gt.tobytes() == z["test.gt_boxes"].tobytes()
    assert np.diff(batch["point_frame_offsets"].cpu().numpy()).tolist() == z["test.num_points"].tolist()
    assert int(batch["overflow"].item()) == 0 and batch["frame_id"] == ["0", "1", "2", "3"]


# ------------------------------------------------------------------------------------------------ 6. reads
def run_counting_syncs(loader, fn):
    """fn() with every stretch between the loader's reads under sync-debug "error" and the reads themselves under "warn":
    returns (result, synchronising calls warned about)."""
    import warnings
    torch = torch_()
    seen, real = [0], loader._read

    def read(t):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                r = real(t)
            seen[0] += sum("synchroniz" in str(x.message).lower() for x in w)
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return r

    loader._read = read
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        loader._read = real
    return out, seen[0]


def test_training_batch_reads_twice_test_batch_once(g22):
    torch = torch_()
    loader = make_loader(g22, True)
    loader.prepare_batch([0, 1, 2, 1], np.random.RandomState(1))          # first use: allocations, pinned buffers
    torch.cuda.synchronize()
    reads0 = loader.reads
    batch, syncs = run_counting_syncs(loader, lambda: loader.prepare_batch([0, 1, 2, 1], np.random.RandomState(2)))
    assert batch["redraw_index"] == {} and batch["batch_size"] == 4
    assert syncs == 2 and loader.reads - reads0 == 2
    tester = make_loader(g22, False)
    tester.prepare_batch([0, 1, 2, 3])
    torch.cuda.synchronize()
    batch, syncs = run_counting_syncs(tester, lambda: tester.prepare_batch([3, 2, 1, 0]))
    assert syncs == 1 and tester.reads == 2 and batch["points"].shape[0] == int(g22["z"]["test.num_points"].sum())


# ------------------------------------------------------------------------------------------------ 7. consumption
def voxelize_on_device(batch_dict, rng6, training=True):
    """_VoxelizingDetector.voxelize_on_device on a stand-in that carries only what the method reads."""
    from types import SimpleNamespace
    from hvpr_amd import detector as D
    from hvpr_amd.config import AttrDict
    cfg = AttrDict(DATA_PROCESSOR=[{"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.8, 0.8, 4.0], "MAX_POINTS_PER_VOXEL": 5,
                                    "MAX_NUMBER_OF_VOXELS": {"train": 16000, "test": 40000}}])
    det = SimpleNamespace(training=training, _voxgen={}, dataset=SimpleNamespace(dataset_cfg=cfg, point_cloud_range=rng6))
    det._voxel_cfg = lambda: D._VoxelizingDetector._voxel_cfg(det)
    det._voxel_generator = lambda device: D._VoxelizingDetector._voxel_generator(det, device)
    det._frame_offsets = D._VoxelizingDetector._frame_offsets
    out = D._VoxelizingDetector.voxelize_on_device(det, dict(batch_dict))
    m = int(out["voxel_count_device"].item())
    return out["voxels"][:m], out["voxel_coords"][:m], out["voxel_num_points"][:m]


def test_voxelizer_consumes_the_batch_like_the_per_frame_chain(g22):
    """The same frames through what existed before: FOV flags + compaction per frame, DeviceAugmentor, range flags + compaction
    per frame, the loader's permutations through gather_rows, torch.cat with a batch column."""
    from hvpr_amd import preprocess as PP
    from hvpr_amd.augment import DeviceAugmentor
    torch = torch_()
    z, indices = g22["z"], [0, 1, 2, 1]
    loader = make_loader(g22, True)
    batch = loader.prepare_batch(indices, np.random.RandomState(7))
    assert batch["redraw_index"] == {}
    frames = [dict(g22["frames"][i]) for i in indices]
    for f in frames:
        f["points"] = chain_frame(f["points"], 1, f["calib"], f["image_shape"])
    aug = DeviceAugmentor(g22["cfg"]["DATA_AUGMENTOR"], g22["classes"], g22["bank"], z["range"])
    out = aug(frames, np.random.RandomState(7))
    off = np.cumsum([0] + out["num_points"].tolist())
    parts = []
    for b in range(4):
        p = out["points"][off[b]: off[b + 1]].contiguous()
        if p.shape[0]:
            flags = PP.mask_points_by_range(p, z["range"])
            kept, count = PP.compact_rows(p, flags)
            p = kept[: int(count.item())]
        perm = batch["permutations"][b]
        assert len(perm) == p.shape[0]
        if p.shape[0]:
            p = PP.gather_rows(p, torch.from_numpy(perm.astype(np.int32)).to(DEV))
        parts.append(torch.cat([torch.full((p.shape[0], 1), float(b), device=DEV), p], dim=1))
    chain = {"points": torch.cat(parts).contiguous(), "batch_size": 4}
    assert torch.equal(bits(chain["points"]), bits(batch["points"]))
    assert torch.equal(out["gt_boxes"][:, : batch["gt_boxes"].shape[1]], batch["gt_boxes"])
    got, want = voxelize_on_device(batch, z["range"]), voxelize_on_device(chain, z["range"])
    assert got[0].shape[0] > 500 and int(got[2].max().item()) == 5, "the 5-point cap bites: the order of the points matters"
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g.contiguous().view(torch.int32), w.contiguous().view(torch.int32))


def test_single_generator_order_and_a_redraw_in_the_first_slot(g22, observed):
    """One generator for the batch: the augmentor draws of all frames, then each empty frame's redraw chain, then the
    permutations (the order batch_loader.py documents and tests/batch_loader_cases.py restates).  The frame that loses every box
    comes FIRST here, so the spliced batch has frames behind the redrawn slot.  The seed is the first for which that frame's
    candidates all collide and the restated batch keeps G22's margins after the augmentor (asserted below): the scene's own
    margins (box pairs, points off candidate faces, the FOV borders) do not depend on the seed."""
    import augment_cases as AC
    import batch_loader_cases as BC
    from hvpr_amd.augment import AugmentPlanner
    z, indices = g22["z"], [3, 0, 2, 1]
    loader = make_loader(g22, True)
    gen = np.random.RandomState(187)
    batch = loader.prepare_batch(indices, gen)
    host_bank = BC.g22_bank(z, device="cpu")
    planner = AugmentPlanner(g22["cfg"]["DATA_AUGMENTOR"], g22["classes"], host_bank)
    ref = np.random.RandomState(187)
    points, gt, slots = BC.prepare_batch_host(BC.g22_frames(z), indices, planner, host_bank, [ref] * 4, z["range"], 4)
    assert len(slots[0]["items"]) >= 2, "the first slot is redrawn"
    r64 = z["range"].astype(np.float64)
    for s in slots:
        xy, tb = s["r"]["points"][:, :2].astype(np.float64), np.asarray(s["r"]["boxes_before_trim"], np.float64)
        assert min(np.abs(xy - r64[0:2]).min(), np.abs(xy - r64[3:5]).min()) >= 1e-3
        cn = AC.box_corners(tb[:, :7])
        assert min(np.abs(cn - r64[0:3]).min(), np.abs(cn - r64[3:6]).min()) >= 1e-3 and np.abs(np.abs(tb[:, 6]) - np.pi).min() >= 1e-3
    assert batch["redraw_index"] == {b: s["items"][1:] for b, s in enumerate(slots) if len(s["items"]) > 1}
    BC.assert_same_batch(points, gt, batch["points"].cpu().numpy(), batch["gt_boxes"].cpu().numpy(), observed, "single generator")
    for b, s in enumerate(slots):
        assert np.array_equal(batch["permutations"][b], s["perm"]), b
    assert np.array_equal(gen.get_state()[1], ref.get_state()[1]) and gen.get_state()[2] == ref.get_state()[2]
    assert batch["frame_id"] == [str(s["items"][-1]) for s in slots] and int(batch["overflow"].item()) == 0
