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

MAX_FRAME_BOXES = 256


def _align(n, a=256):
    return (n + a - 1) // a * a


class _Chunk:
    """A chunk's inputs in one pinned staging buffer, uploaded with one copy: pt_off, box_off (int32), boxes (float32), centres
    (float64) and, where the frames came from the host, the points.  The host views stay valid for the library's checks."""

    def __init__(self, points_list, boxes_list, device, stage):
        dev = torch.device(device)
        B = len(points_list)
        F = {int(p.shape[1]) for p in points_list}
        if len(F) != 1:
            raise ValueError("frames of one chunk must share a point feature width")
        self.F = F.pop()
        n_pts = [int(p.shape[0]) for p in points_list]
        n_box = [int(b.shape[0]) for b in boxes_list]
        if max(n_box) > MAX_FRAME_BOXES:
            raise ValueError(f"a frame may hold {MAX_FRAME_BOXES} boxes, got {max(n_box)}")
        N, M = sum(n_pts), sum(n_box)
        on_host = all(isinstance(p, np.ndarray) for p in points_list)
        o_pt, o_box = 0, _align(4 * (B + 1))
        o_boxes = o_box + _align(4 * (B + 1))
        o_ctr = o_boxes + _align(28 * M)
        o_pts = o_ctr + _align(24 * M)
        total = o_pts + (_align(4 * self.F * N) if on_host else 0)
        if stage[0] is None or stage[0].numel() < total:
            stage[0] = torch.empty((max(total, 1 << 16),), dtype=torch.uint8).pin_memory()
        host = stage[0][:total]

        def hv(o, count, tdtype, width):
            return host[o: o + count * width].view(tdtype)

        self.pt_off_host, self.box_off_host = hv(o_pt, B + 1, torch.int32, 4), hv(o_box, B + 1, torch.int32, 4)
        boxes_h, ctr_h = hv(o_boxes, 7 * M, torch.float32, 4).view(M, 7), hv(o_ctr, 3 * M, torch.float64, 8).view(M, 3)
        self.pt_off_host.numpy()[:] = np.concatenate([[0], np.cumsum(n_pts)])
        self.box_off_host.numpy()[:] = np.concatenate([[0], np.cumsum(n_box)])
        if M:
            b64 = np.concatenate([np.asarray(b, np.float64).reshape(-1, b.shape[1])[:, :7] for b in boxes_list if b.shape[0]], axis=0)
            boxes_h.numpy()[:] = b64.astype(np.float32)
            ctr_h.numpy()[:] = b64[:, :3]
        if on_host and N:
            pts_h = hv(o_pts, self.F * N, torch.float32, 4).view(N, self.F)
            np.concatenate([np.asarray(p, np.float32) for p in points_list], axis=0, out=pts_h.numpy())
        d = host.to(dev, non_blocking=True)                                      # the one upload of the chunk

        def dv(o, count, tdtype, width):
            return d[o: o + count * width].view(tdtype)

        self.pt_off, self.box_off = dv(o_pt, B + 1, torch.int32, 4), dv(o_box, B + 1, torch.int32, 4)
        self.boxes, self.centres = dv(o_boxes, 7 * M, torch.float32, 4).view(M, 7), dv(o_ctr, 3 * M, torch.float64, 8).view(M, 3)
        if on_host:
            self.points = dv(o_pts, self.F * N, torch.float32, 4).view(N, self.F)
        else:                                                                    # frames that are on the device already stay there
            per = [torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev) if isinstance(p, np.ndarray)
                   else p.to(dev, torch.float32) for p in points_list]
            self.points = (per[0] if B == 1 else torch.cat(per, dim=0)).contiguous()
        self.n_obj, self.n_box = M, n_box

    def count(self, workspace=None):
        return kernels.gt_database_count(self.points, self.pt_off_host, self.pt_off, self.boxes, self.box_off_host, self.box_off,
                                         workspace=workspace)


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
    out, stage, ws = [], [None], None
    for c0 in range(0, len(points_list), int(frames_per_call)):
        chunk = _Chunk([_points_of(p) for p in points_list[c0: c0 + frames_per_call]],
                       [_boxes_of(b) for b in boxes_list[c0: c0 + frames_per_call]], device, stage)
        counts, ws = chunk.count(ws)
        counts = counts.cpu().numpy()
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
        self._stage, self._count_stage, self._ws = [None], None, None

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
        chunk = _Chunk(pts, [np.asarray(info["annos"]["gt_boxes_lidar"]) for info in infos], self.device, self._stage)
        if chunk.n_obj == 0:
            return
        counts_dev, self._ws = chunk.count(self._ws)
        if self._count_stage is None or self._count_stage.numel() < chunk.n_obj:
            self._count_stage = torch.empty((max(chunk.n_obj, 1024),), dtype=torch.int32).pin_memory()
        counts_host = self._count_stage[: chunk.n_obj]
        counts_host.copy_(counts_dev)                                            # the one read of the chunk (synchronises)
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
