"""Point pre-processing in front of the voxelizer, on the device ("next" row f2 of SURVEY.md §8f) plus the host->device
input path (row f1).  Mirrors, with the reference's names:

  * mask_points_by_range               pcdet/utils/common_utils.py:59-62
  * DataProcessor.mask_points_and_boxes_outside_range / sample_points
                                       pcdet/datasets/processor/data_processor.py:20-30,77-108
  * KittiDataset.get_fov_flag          pcdet/datasets/kitti/kitti_dataset.py:100-116 (over Calibration.lidar_to_rect /
                                       rect_to_img, pcdet/utils/calibration_kitti.py:65-84)
  * collate_batch's `points` branch + load_data_to_gpu
                                       pcdet/datasets/dataset.py:148-180 and the absent pcdet/models/__init__.py

Flags, stable compaction and the row gather are HIP kernels (csrc/preprocess.hip).  `sample_points` draws its indices on
the host with the SAME sequence of numpy RNG calls as the reference (test.py:47 seeds numpy even at test time), from near
flags computed on the device — bit-identical post-sampling points for a given seed.
"""
import numpy as np
import torch

from . import kernels
from ._lib import call, lib
from .calibration import fov_matrices


def _flags(points, mode, range_xy=None, near=40.0, fov=None):
    n = points.shape[0]
    flags = torch.empty((n,), dtype=torch.uint8, device=points.device)
    a = p = None
    h = w = 0
    if fov is not None:
        a, p, (h, w) = fov
    call("hvpr_point_flags_f32", points, n, points.shape[1], mode, range_xy, float(near), a, p, int(h), int(w), flags, kernels._stream())
    return flags


def mask_points_by_range(points, limit_range):
    """points (N, >=3) f32 cuda -> uint8 mask (x and y inside [lo, hi], inclusive)."""
    r = torch.as_tensor(np.asarray(limit_range, np.float32)[[0, 1, 3, 4]], device=points.device)
    return _flags(points.contiguous(), 0, r)


def get_fov_flag(points, calib, img_shape):
    """uint8 mask of the points that project into the image (and lie in front of the camera)."""
    a, p = fov_matrices(calib, points.device)
    every = torch.tensor([-3.0e38, -3.0e38, 3.0e38, 3.0e38], device=points.device)
    return _flags(points.contiguous(), 0, every, fov=(a, p, (int(img_shape[0]), int(img_shape[1]))))


def compact_rows(rows, flags, count_only=False):
    """rows[flags != 0], stable.  Returns (out, count): `out` has rows.shape[0] rows of which the first `count` (device
    int32) are live — no host synchronisation; slice with int(count) when a host size is needed."""
    rows = rows.contiguous()
    n, w = rows.shape
    out = torch.empty_like(rows)
    count = torch.zeros((1,), dtype=torch.int32, device=rows.device)
    ws = torch.empty((lib().hvpr_compact_workspace_bytes(n),), dtype=torch.uint8, device=rows.device)
    call("hvpr_compact_rows_f32", rows, n, w, flags, out, n, count, ws, ws.numel(), kernels._stream())
    return out, count


def gather_rows(rows, idx):
    rows = rows.contiguous()
    idx = idx.to(torch.int32).contiguous()
    out = torch.empty((idx.shape[0], rows.shape[1]), dtype=torch.float32, device=rows.device)
    call("hvpr_gather_rows_f32", rows, rows.shape[0], rows.shape[1], idx, idx.shape[0], out, kernels._stream())
    return out


def shuffle_points(points, rng=np.random):
    """DataProcessor.shuffle_points (data_processor.py:32-39) for one frame: points[rng.permutation(N)], the permutation drawn
    on the host as the reference draws it, the rows gathered on the device.  (A whole batch at once, fused with the range mask
    and the collation: hvpr_amd.batch_loader.DeviceBatchLoader.)"""
    perm = rng.permutation(points.shape[0])
    return gather_rows(points, torch.from_numpy(np.ascontiguousarray(perm).astype(np.int32)).to(points.device))


def plan_sample_points(n, c, num_points, rng=np.random, shuffle=False):
    """DataProcessor.sample_points (data_processor.py:77-108) for a frame of n rows of which c are near, from the counts alone:
    the reference's sequence of generator calls (the draw at :91 in front of the size test included), over ordinals.  Returns a
    dict: `mode` 0 when an entry of `choice` is a row's in-frame rank, 1 when it is a near ordinal (< c) or c + a far ordinal;
    `choice`, the reference's `choice` in that form; `perm`, the following `rng.permutation` (None without `shuffle`); `order` =
    choice[perm], the source of every output row.  Raises what the reference raises."""
    n, c, P = int(n), int(c), int(num_points)
    if not 0 <= c <= n:
        raise ValueError(f"plan_sample_points: {c} near rows of {n}")
    mode = 0
    if P == -1:
        choice = np.arange(n)
    elif P < n:
        far, near_ord = n - c, np.arange(c)
        want = P - far
        drawn = rng.choice(near_ord, want, replace=False)               # :91, ValueError when more than P rows are far
        if want > 0:
            drawn = rng.choice(near_ord, want, replace=False)
            choice = np.concatenate((drawn, c + np.arange(far)), axis=0) if far > 0 else drawn
            mode = 1
        else:
            choice = rng.choice(np.arange(n), P, replace=False)
        rng.shuffle(choice)
    else:
        choice = np.arange(n)
        if P > n:                                                        # ValueError when P - n > n or the frame is empty
            choice = np.concatenate((choice, rng.choice(choice, P - n, replace=False)), axis=0)
        rng.shuffle(choice)
    perm = rng.permutation(len(choice)) if shuffle else None
    return {"mode": mode, "choice": choice, "perm": perm, "order": choice if perm is None else choice[perm]}


def resolve_sample_choice(plan, near):
    """The reference's `choice` (row indices) of a plan, given the frame's near flags."""
    if plan["mode"] == 0:
        return plan["choice"]
    near = np.asarray(near) != 0
    return np.concatenate((np.where(near)[0], np.where(~near)[0]))[plan["choice"]]


def sample_points_choice(near, num_points, rng=np.random):
    """Index selection of DataProcessor.sample_points for one frame whose near flags are on the host: the plan, resolved.  Like
    the reference, this raises ValueError when more than num_points points lie beyond 40 m."""
    near = np.asarray(near)
    return resolve_sample_choice(plan_sample_points(len(near), np.count_nonzero(near), num_points, rng), near)


class PointPreprocessor:
    """The device-side DataProcessor steps of kitti_dataset.yaml that precede `transform_points_to_voxels`
    (which MixAnchor_Memory.forward performs itself): FOV filter, range mask, sample_points."""

    def __init__(self, point_cloud_range, num_points=16384, training=False, fov_points_only=True):
        self.point_cloud_range = np.asarray(point_cloud_range, np.float32)
        self.num_points, self.training, self.fov_points_only = num_points, training, fov_points_only

    def mask_points_and_boxes_outside_range(self, points):
        out, count = compact_rows(points, mask_points_by_range(points, self.point_cloud_range))
        return out[: int(count.item())]

    def fov_filter(self, points, calib, img_shape):
        out, count = compact_rows(points, get_fov_flag(points, calib, img_shape))
        return out[: int(count.item())]

    def sample_points(self, points, rng=np.random):
        if self.num_points == -1:
            return points
        near = _flags(points.contiguous(), 1, near=40.0).cpu().numpy() if self.num_points < points.shape[0] else \
            np.ones((points.shape[0],), np.uint8)
        choice = sample_points_choice(near, self.num_points, rng)
        return gather_rows(points, torch.from_numpy(np.ascontiguousarray(choice).astype(np.int32)).to(points.device))

    def __call__(self, points, calib=None, img_shape=None, rng=np.random):
        if self.fov_points_only and calib is not None:
            points = self.fov_filter(points, calib, img_shape)
        points = self.mask_points_and_boxes_outside_range(points)
        return self.sample_points(points, rng)


# ------------------------------------------------------------------------------------------------ f1: host -> device
def to_device(array, device):
    """A host array on `device` through pinned memory: the upload does not synchronise the host."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    if torch.device(device).type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


class PinnedBuffer:
    """A grow-only pinned staging buffer: `take(n)` is its first n elements, allocated anew only when n outgrows it."""

    def __init__(self, dtype=torch.int32, floor=4096):
        self.dtype, self.floor, self._buf = dtype, int(floor), None

    def take(self, n):
        if self._buf is None or self._buf.numel() < n:
            self._buf = torch.empty((max(int(n), self.floor),), dtype=self.dtype).pin_memory()
        return self._buf[:n]


class InputPipeline:
    """collate_batch's `points` branch (dataset.py:161-166: a batch-index column in front of every frame's rows) and
    load_data_to_gpu, as a double-buffered pinned-memory upload on its own HIP stream: frame k+1 is copied while frame k
    computes.  `put(frames)` stages a list of (N_i, C) float32 arrays; `get()` returns the batch_dict of the OLDEST staged
    batch with device tensors `points` (sum N_i, C+1) and `point_frame_offsets` (B+1,) int32."""

    def __init__(self, max_points, n_feat=4, max_batch=1, device="cuda:0", depth=2):
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device)
        self.slots = [{"host": torch.empty((max_points, n_feat + 1), dtype=torch.float32).pin_memory(),
                       "dev": torch.empty((max_points, n_feat + 1), dtype=torch.float32, device=self.device),
                       "off_host": torch.zeros((max_batch + 1,), dtype=torch.int32).pin_memory(),
                       "off_dev": torch.zeros((max_batch + 1,), dtype=torch.int32, device=self.device),
                       "ready": torch.cuda.Event(), "free": torch.cuda.Event(), "n": 0, "b": 0} for _ in range(depth)]
        self.head = self.tail = 0

    def put(self, frames):
        s = self.slots[self.head % len(self.slots)]
        s["free"].synchronize()                    # the batch that used this slot has been consumed by the GPU
        n = 0
        for b, f in enumerate(frames):
            m = len(f)
            s["host"][n:n + m, 0] = float(b)
            s["host"][n:n + m, 1:] = torch.from_numpy(np.ascontiguousarray(f, np.float32))
            s["off_host"][b] = n
            n += m
        s["off_host"][len(frames)] = n
        s["n"], s["b"] = n, len(frames)
        with torch.cuda.stream(self.stream):
            s["dev"][:n].copy_(s["host"][:n], non_blocking=True)
            s["off_dev"][: len(frames) + 1].copy_(s["off_host"][: len(frames) + 1], non_blocking=True)
            s["ready"].record(self.stream)
        self.head += 1

    def get(self):
        assert self.tail < self.head, "InputPipeline.get() without a staged batch"
        s = self.slots[self.tail % len(self.slots)]
        self.tail += 1
        torch.cuda.current_stream(self.device).wait_event(s["ready"])
        return {"points": s["dev"][: s["n"]], "point_frame_offsets": s["off_dev"][: s["b"] + 1], "batch_size": s["b"]}, s

    @staticmethod
    def release(slot):
        """Call after the consumer's kernels that read the slot are enqueued."""
        slot["free"].record(torch.cuda.current_stream())
