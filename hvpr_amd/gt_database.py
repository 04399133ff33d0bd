"""The GT-sampling database built on the device from raw frames: the reference's KittiDataset.create_groundtruth_database
(pcdet/datasets/kitti/kitti_dataset.py:193-243), whose native points_in_boxes_cpu is absent from the reference.

  count_points_in_boxes        per frame and box how many of the frame's points lie inside: the count-only mode.
  DatabaseBuilder              takes `infos` in the reference's layout and a `get_lidar`, a chunk of frames per library call
                               (csrc/gt_database.hip): one pinned upload, the count call, ONE host read (the counts, which are
                               the records' num_points_in_gt), the arena grown, the extract call.  Every object's points stay in
                               one device arena.
  builder.db_infos()           {name: [record]} with the reference's keys, value types and order.
  builder.object_bank(...)     an augment.ObjectBank whose points never left the device.
  create_groundtruth_database  the reference's method: gt_database[_<split>]/<idx>_<name>_<i>.bin and kitti_dbinfos_<split>.pkl,
                               after one device-to-host copy of the arena.

A point is inside a box as hvpr_amd.gt_sampling.points_in_boxes_cpu decides (fp32); an object's points are moved into its own
frame as numpy does at :226, float32 minus float64 rounded once.
"""
import os
import pickle

import numpy as np
import torch

from . import kernels
from .augment import ObjectBank
from .calibration import CALIB_WORDS, pack_calib
from .preprocess import PinnedBuffer

MAX_FRAME_BOXES = 256


def _align(n, a=256):
    return (n + a - 1) // a * a


def chunk_layout(B, n_boxes, n_points, F, centres=False, calib=False, points=False):
    """({section: byte offset}, total bytes) of a chunk of B frames in its staging buffer, every section 256-byte aligned.  pt_off
    and box_off (int32, B + 1 each) and boxes (float32, 7 a box) are always there; centres (float64, 3 a box), calib (float32,
    CALIB_WORDS a frame) and points (float32, F a point) where asked for: a section that is not takes no bytes."""
    sizes = [("pt_off", 4 * (B + 1)), ("box_off", 4 * (B + 1))] + ([("calib", 4 * CALIB_WORDS * B)] if calib else []) \
        + [("boxes", 28 * n_boxes)] + ([("centres", 24 * n_boxes)] if centres else []) + ([("points", 4 * F * n_points)] if points else [])
    offsets, total = {}, 0
    for name, size in sizes:
        offsets[name], total = total, total + _align(size)
    return offsets, total


def _view(buf, offset, dtype, *shape):
    """`shape` elements of `dtype` at byte `offset` of the uint8 tensor `buf`: the staging buffer or its device copy."""
    return buf[offset: offset + int(np.prod(shape)) * dtype.itemsize].view(dtype).view(*shape)


class StagedChunk:
    """A chunk's inputs in one pinned staging buffer (`stage`, a preprocess.PinnedBuffer of uint8 that may be shared by the chunks
    of a run), uploaded with one copy: pt_off, box_off (int32), boxes (float32); with `centres` the float64 box centres the
    database's extract call takes; with `calibs` and `image_shapes` the calibration table (calibration.pack_calib) of get_infos'
    count; and, where the frames came from the host, the points.  Frames that are on the device already stay there.  The host
    views stay valid for the library's checks."""

    def __init__(self, points_list, boxes_list, device, stage=None, centres=False, calibs=None, image_shapes=None):
        dev = torch.device(device)
        B = len(points_list)
        F = {int(p.shape[1]) for p in points_list}
        if len(F) != 1:
            raise ValueError("frames of one chunk must share a point feature width")
        self.F = F = F.pop()
        n_pts = [int(p.shape[0]) for p in points_list]
        n_box = [int(b.shape[0]) for b in boxes_list]
        if max(n_box) > MAX_FRAME_BOXES:
            raise ValueError(f"a frame may hold {MAX_FRAME_BOXES} boxes, got {max(n_box)}")
        N, M = sum(n_pts), sum(n_box)
        on_host = all(isinstance(p, np.ndarray) for p in points_list)
        at, total = chunk_layout(B, M, N, F, centres=centres, calib=calibs is not None, points=on_host)
        host = (stage if stage is not None else PinnedBuffer(torch.uint8, 1 << 16)).take(total)

        def sections(buf):
            return {"pt_off": _view(buf, at["pt_off"], torch.int32, B + 1), "box_off": _view(buf, at["box_off"], torch.int32, B + 1),
                    "boxes": _view(buf, at["boxes"], torch.float32, M, 7),
                    "centres": _view(buf, at["centres"], torch.float64, M, 3) if centres else None,
                    "calib": _view(buf, at["calib"], torch.float32, B, CALIB_WORDS) if calibs is not None else None,
                    "points": _view(buf, at["points"], torch.float32, N, F) if on_host else None}

        h = sections(host)
        self.pt_off_host, self.box_off_host, self.calib_host = h["pt_off"], h["box_off"], h["calib"]
        self.pt_off_host.numpy()[:] = np.concatenate([[0], np.cumsum(n_pts)])
        self.box_off_host.numpy()[:] = np.concatenate([[0], np.cumsum(n_box)])
        if calibs is not None:
            self.calib_host.numpy()[:] = pack_calib(calibs, image_shapes)
        if M:
            b64 = np.concatenate([np.asarray(b, np.float64).reshape(-1, b.shape[1])[:, :7] for b in boxes_list if b.shape[0]], axis=0)
            h["boxes"].numpy()[:] = b64.astype(np.float32)
            if centres:
                h["centres"].numpy()[:] = b64[:, :3]
        if on_host and N:
            np.concatenate([np.asarray(p, np.float32) for p in points_list], axis=0, out=h["points"].numpy())
        d = sections(host.to(dev, non_blocking=True))                            # the one upload of the chunk
        self.pt_off, self.box_off, self.boxes, self.centres, self.calib = d["pt_off"], d["box_off"], d["boxes"], d["centres"], d["calib"]
        if on_host:
            self.points = d["points"]
        else:                                                                    # frames that are on the device already stay there
            per = [torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev) if isinstance(p, np.ndarray)
                   else p.to(dev, torch.float32) for p in points_list]
            self.points = (per[0] if B == 1 else torch.cat(per, dim=0)).contiguous()
        self.n_obj, self.n_box = M, n_box

    def count(self, workspace=None, want_fov=False):
        """(obj_count, fov_count, workspace).  With a calibration table get_infos' count: per box the points in the camera's view
        and inside it, and with `want_fov` per frame the points in view.  Without one the database's: every point of the frame
        counts, fov_count is None, and the workspace goes to gt_database_extract."""
        chunk = (self.points, self.pt_off_host, self.pt_off, self.boxes, self.box_off_host, self.box_off)
        if self.calib is None:
            obj_count, workspace = kernels.gt_database_count(*chunk, workspace=workspace)
            return obj_count, None, workspace
        return kernels.kitti_infos_count(*chunk, self.calib_host, self.calib, want_fov=want_fov, workspace=workspace)


class CountReader:
    """The grown pinned stage of a chunk's counts and the chunk's ONE synchronising read; `reads` counts them."""

    def __init__(self):
        self._stage, self.reads = PinnedBuffer(torch.int32, 1024), 0

    def __call__(self, counts_dev):
        """The int32 host tensor of `counts_dev`, valid until the next call."""
        host = self._stage.take(counts_dev.numel())
        host.copy_(counts_dev)                                                   # the one read of the chunk (synchronises)
        self.reads += 1
        return host


def _boxes_of(b):
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    return b.reshape(-1, 7) if b.size == 0 else b


def _points_of(p):
    return p if hasattr(p, "detach") else np.asarray(p)


def count_points_in_boxes(points_list, boxes_list, device="cuda:0", frames_per_call=32):
    """Per frame i an (n_i,) int32 array: how many of points_list[i] (N_i, F) lie inside each of boxes_list[i] (n_i, 7+).  The
    box test of the database, without the database; NOT get_infos' num_points_in_gt (kitti_dataset.py:171-184), which is a hull
    test over the points in the camera's view: that count is hvpr_amd.kitti_dataset's (InfoCounter, KittiDataset.get_infos)."""
    if len(points_list) != len(boxes_list):
        raise ValueError("count_points_in_boxes: one box array per frame")
    out, stage, read, ws = [], PinnedBuffer(torch.uint8, 1 << 16), CountReader(), None
    for c0 in range(0, len(points_list), int(frames_per_call)):
        chunk = StagedChunk([_points_of(p) for p in points_list[c0: c0 + frames_per_call]],
                            [_boxes_of(b) for b in boxes_list[c0: c0 + frames_per_call]], device, stage)
        counts, _, ws = chunk.count(ws)
        counts = read(counts).numpy()
        off = chunk.box_off_host.numpy()
        out.extend(counts[off[f]: off[f + 1]].copy() for f in range(len(chunk.n_box)))
    return out


class DatabaseBuilder:
    """add_frames(infos, get_lidar): `infos` as the reference's kitti_infos_*.pkl holds them (the keys read at
    kitti_dataset.py:207-214: point_cloud.lidar_idx; annos.name, difficulty, bbox, score, gt_boxes_lidar as float64, which has
    fewer rows than `name` when DontCare rows trail), `get_lidar(sample_idx)` an (N, F) float32 array or device tensor.
    `used_classes` filters the records, not the objects: the reference writes a file for every object (:221-238)."""

    def __init__(self, class_names=None, used_classes=None, num_point_features=4, frames_per_call=32, device="cuda:0", split="train"):
        self.class_names = None if class_names is None else list(class_names)
        self.used_classes = None if used_classes is None else list(used_classes)
        self.num_point_features = int(num_point_features)
        self.frames_per_call = max(1, int(frames_per_call))
        self.device = torch.device(device)
        self.split = split
        self.database_dir = "gt_database" if split == "train" else "gt_database_%s" % split
        self.objects = []                     # every object in the reference's order: (record, used, first row, rows)
        self._arena = torch.empty((0, self.num_point_features), dtype=torch.float32, device=self.device)
        self._rows = 0
        self._stage, self._read, self._ws = PinnedBuffer(torch.uint8, 1 << 16), CountReader(), None

    def _reserve(self, rows):
        if self._rows + rows > self._arena.shape[0]:
            grown = torch.empty((max(self._rows + rows, 2 * self._arena.shape[0]), self.num_point_features), dtype=torch.float32,
                                device=self.device)
            grown[: self._rows] = self._arena[: self._rows]
            self._arena = grown

    def add_frames(self, infos, get_lidar):
        for c0 in range(0, len(infos), self.frames_per_call):
            self._add_chunk(infos[c0: c0 + self.frames_per_call], get_lidar)
        return self

    def _add_chunk(self, infos, get_lidar):
        pts = [_points_of(get_lidar(info["point_cloud"]["lidar_idx"])) for info in infos]
        if any(int(p.shape[1]) != self.num_point_features for p in pts):
            raise ValueError(f"get_lidar must return (N, {self.num_point_features}) points")
        chunk = StagedChunk(pts, [np.asarray(info["annos"]["gt_boxes_lidar"]) for info in infos], self.device, self._stage, centres=True)
        if chunk.n_obj == 0:
            return
        counts_dev, _, self._ws = chunk.count(self._ws)
        counts_host = self._read(counts_dev)
        counts = counts_host.numpy()
        rows = int(counts.sum(dtype=np.int64))
        self._reserve(rows)
        kernels.gt_database_extract(chunk.points, chunk.pt_off_host, chunk.pt_off, chunk.boxes, chunk.box_off_host, chunk.box_off,
                                    chunk.centres, counts_host, counts_dev, self._arena[self._rows:], self._ws)
        k, start = 0, self._rows
        for info in infos:                                                       # kitti_dataset.py:207-238
            sample_idx, annos = info["point_cloud"]["lidar_idx"], info["annos"]
            names, difficulty, bbox, gt_boxes = annos["name"], annos["difficulty"], annos["bbox"], annos["gt_boxes_lidar"]
            for i in range(gt_boxes.shape[0]):
                n = int(counts[k])
                rec = {"name": names[i], "path": "%s/%s_%s_%d.bin" % (self.database_dir, sample_idx, names[i], i),
                       "image_idx": sample_idx, "gt_idx": i, "box3d_lidar": gt_boxes[i], "num_points_in_gt": n,
                       "difficulty": difficulty[i], "bbox": bbox[i], "score": annos["score"][i]}
                self.objects.append((rec, self.used_classes is None or names[i] in self.used_classes, start, n))
                k, start = k + 1, start + n
        self._rows = start           # no wait: the read above came after the upload, and the extract call reads the device only

    def arena(self):
        """(rows, F) device tensor: every object's points, in the order of `objects`."""
        return self._arena[: self._rows]

    def db_infos(self):
        out = {}
        for rec, used, _, _ in self.objects:
            if used:
                out.setdefault(rec["name"], []).append(rec)
        return out

    def object_bank(self, class_names=None, prepare=None):
        class_names = self.class_names if class_names is None else list(class_names)
        if class_names is None:
            raise ValueError("object_bank needs class_names")
        rows_of = {id(rec): (start, n) for rec, _, start, n in self.objects}
        return ObjectBank.from_device(self.db_infos(), self.arena(), rows_of, class_names, prepare=prepare,
                                      num_point_features=self.num_point_features, device=self.device)

    def write(self, root_path):
        """The files of kitti_dataset.py:196-243 under `root_path`; one device-to-host copy of the arena."""
        root = str(root_path)
        os.makedirs(os.path.join(root, self.database_dir), exist_ok=True)
        host = self.arena().cpu().numpy()
        for rec, _, start, n in self.objects:
            with open(os.path.join(root, rec["path"]), "w") as f:
                host[start: start + n].tofile(f)                                # no points: a zero-byte file, as the reference's
        with open(os.path.join(root, "kitti_dbinfos_%s.pkl" % self.split), "wb") as f:
            pickle.dump(self.db_infos(), f)


def create_groundtruth_database(root_path, infos_or_info_path, get_lidar, used_classes=None, split="train", **builder_args):
    """KittiDataset.create_groundtruth_database(info_path, used_classes, split) for a dataset rooted at `root_path`; returns the
    builder, whose `object_bank` gives the same database without reading the files back."""
    infos = infos_or_info_path
    if isinstance(infos, (str, os.PathLike)):
        with open(infos, "rb") as f:
            infos = pickle.load(f)
    builder = DatabaseBuilder(used_classes=used_classes, split=split, **builder_args)
    builder.add_frames(infos, get_lidar)
    builder.write(root_path)
    return builder
