"""GPU: gt_database.StagedChunk, the one staged chunk of the database's count and of get_infos' count, at the shapes where a
chunk can go wrong: a frame with no box, a frame with no point behind one that has some, a frame with exactly MAX_FRAME_BOXES
boxes (one more is refused), each with its frames given as host arrays and as device tensors.

A chunk that carries BOTH optional sections (float64 centres and the calibration table) must count as a chunk that carries
centres only does under kernels.gt_database_count, and as one that carries the calibration only does under
kernels.kitti_infos_count: the sections a call does not read may not move the ones it does.  Both are held to the numpy checkers
of tests/kitti_infos_cases.py (plain_count_host, count_host).  Counts are integers and compared exactly; every cloud keeps that
module's margin rule (asserted here for every frame), so no point is left out of the comparison."""
import numpy as np
import pytest

import kitti_infos_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = {"one frame, no box": ([300], [0], 31),
         "second frame has no point": ([400, 0], [3, 2], 32),
         "exactly MAX_FRAME_BOXES boxes": ([700], [256], 33)}


@pytest.fixture(scope="module")
def cases():
    """name -> (frames, per frame the database's counts, per frame get_infos' counts): made once, never written to."""
    out = {}
    for name, (points, boxes, seed) in CASES.items():
        frames = KC.make_case(points, boxes, seed=seed)
        assert all(KC.margins_hold(f["points"], f["boxes"], f["calib"], f["image_shape"]) for f in frames)
        plain = [KC.plain_count_host(f["points"], f["boxes"]) for f in frames]
        in_view, _ = KC.counts_of(frames)
        out[name] = (frames, plain, in_view)
    return out


def chunk_of(frames, on_device, centres, calib):
    import torch
    from hvpr_amd.gt_database import StagedChunk
    pts = [torch.from_numpy(f["points"]).to(DEV) if on_device else f["points"] for f in frames]
    extra = {"calibs": [f["calib"] for f in frames], "image_shapes": [f["image_shape"] for f in frames]} if calib else {}
    return StagedChunk(pts, [f["boxes"] for f in frames], DEV, centres=centres, **extra)


def database_counts(chunk):
    from hvpr_amd import kernels
    counts, _ = kernels.gt_database_count(chunk.points, chunk.pt_off_host, chunk.pt_off, chunk.boxes, chunk.box_off_host, chunk.box_off)
    return counts.cpu().numpy()


def infos_counts(chunk):
    from hvpr_amd import kernels
    counts, _, _ = kernels.kitti_infos_count(chunk.points, chunk.pt_off_host, chunk.pt_off, chunk.boxes, chunk.box_off_host,
                                             chunk.box_off, chunk.calib_host, chunk.calib)
    return counts.cpu().numpy()


@pytest.mark.parametrize("on_device", [False, True], ids=["host frames", "device frames"])
@pytest.mark.parametrize("name", list(CASES))
def test_both_sections_count_as_either_alone(cases, name, on_device):
    frames, plain, in_view = cases[name]
    both = chunk_of(frames, on_device, centres=True, calib=True)
    centres_only, calib_only = chunk_of(frames, on_device, centres=True, calib=False), chunk_of(frames, on_device, centres=False, calib=True)
    assert both.centres is not None and both.calib is not None
    assert centres_only.calib is None and centres_only.calib_host is None and calib_only.centres is None
    assert both.n_obj == sum(len(f["boxes"]) for f in frames) and both.n_box == [len(f["boxes"]) for f in frames]
    # the sections themselves: what was staged is what arrived
    b32 = np.concatenate([np.asarray(f["boxes"], np.float64).reshape(-1, 7) for f in frames]).astype(np.float32)
    c64 = np.concatenate([np.asarray(f["boxes"], np.float64).reshape(-1, 7)[:, :3] for f in frames])
    for chunk in (both, centres_only, calib_only):
        assert np.array_equal(chunk.boxes.cpu().numpy(), b32)
        assert chunk.pt_off.cpu().numpy().tolist() == chunk.pt_off_host.numpy().tolist() == np.cumsum([0] + [len(f["points"]) for f in frames]).tolist()
        assert chunk.box_off.cpu().numpy().tolist() == chunk.box_off_host.numpy().tolist() == np.cumsum([0] + both.n_box).tolist()
        assert np.array_equal(chunk.points.cpu().numpy(), np.concatenate([f["points"] for f in frames]))
    for chunk in (both, centres_only):
        assert chunk.centres.dtype.is_floating_point and chunk.centres.element_size() == 8 and np.array_equal(chunk.centres.cpu().numpy(), c64)
    for chunk in (both, calib_only):
        assert np.array_equal(chunk.calib.cpu().numpy(), chunk.calib_host.numpy()) and tuple(chunk.calib.shape) == (len(frames), 26)
    # the database's count
    got, alone = database_counts(both), database_counts(centres_only)
    assert got.dtype == np.int32 and np.array_equal(got, alone)
    assert np.array_equal(got, np.concatenate(plain))
    # get_infos' count
    got, alone = infos_counts(both), infos_counts(calib_only)
    assert got.dtype == np.int32 and np.array_equal(got, alone)
    assert np.array_equal(got, np.concatenate(in_view))
    # and the chunk's own `count` is the call its sections name
    assert np.array_equal(centres_only.count()[0].cpu().numpy(), np.concatenate(plain)) and centres_only.count()[1] is None
    assert np.array_equal(calib_only.count()[0].cpu().numpy(), np.concatenate(in_view))


def test_the_cases_count_something(cases):
    """The comparison above is not between zeros: boxes with points, and in the full frame boxes in view and out of it."""
    _, plain, in_view = cases["second frame has no point"]
    assert int(plain[0].sum()) > 0 and plain[1].tolist() == [0, 0] and in_view[1].tolist() == [0, 0]
    _, plain, in_view = cases["exactly MAX_FRAME_BOXES boxes"]
    assert len(plain[0]) == 256 and (plain[0] > 0).sum() >= 8 and (in_view[0] > 0).sum() >= 4 and (in_view[0] < plain[0]).sum() >= 4
    _, plain, in_view = cases["one frame, no box"]
    assert len(plain[0]) == 0 and len(in_view[0]) == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host frames", "device frames"])
def test_one_box_more_than_a_frame_may_hold_is_refused(on_device):
    from hvpr_amd.gt_database import MAX_FRAME_BOXES
    assert MAX_FRAME_BOXES == 256
    big = KC.make_case([64], [MAX_FRAME_BOXES + 1], seed=34)
    for centres, calib in ((True, True), (True, False), (False, True)):
        with pytest.raises(ValueError, match="a frame may hold 256 boxes, got 257"):
            chunk_of(big, on_device, centres, calib)
