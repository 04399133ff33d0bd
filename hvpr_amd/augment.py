"""Training augmentation on the device, a whole batch per call: the reference's DataAugmentor (pcdet/datasets/augmentor/) and the
training-only box trim of `mask_points_and_boxes_outside_range` (data_processor.py:24-28).

  ObjectBank       the GT-sampling database (database_sampler.py:10-77): records and per-class lists on the host, every
                   surviving object's points ONCE in one device arena.
  AugmentPlanner   the host RNG protocol: exactly the reference's `np.random` draws in exactly its order, one small plan per
                   frame (candidate objects per sample group, flip flags, rotation, scale).  A seeded run stays comparable.
  DeviceAugmentor  plans a batch, uploads all plans in one pinned buffer with one copy, runs the HIP kernels of
                   csrc/augment.hip (collision test, boxes, points) for all frames at once, and reads the device ONCE.

The reference redraws a frame that ends up with no box (dataset.py:127-129).  That redraw stays the caller's: the box counts
come back on the host for it.

A quirk of the reference that is kept, not fixed: `SAMPLE_GROUPS` entries of classes outside `class_names` are skipped
(database_sampler.py:33-34), so with CLASS_NAMES ['Car'] and the groups of hvpr.yaml (Pedestrian, Cyclist) nothing is sampled.
"""
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch

from . import kernels, preprocess
from .calibration import lidar_to_rect, rect_to_lidar
from .config import _get

OP_FLIP_X, OP_FLIP_Y, OP_ROTATE, OP_SCALE = 1, 2, 3, 4
PLAN_MAGIC = 0x31475541
PLAN_HEADER = 8


# ------------------------------------------------------------------------------------------------ the database
class ObjectBank:
    """db_infos: {class: [record]} with the reference's record keys (name, path, box3d_lidar, num_points_in_gt, difficulty);
    a record may carry its points inline under 'points' instead of a path (from_arrays).  `prepare` is the PREPARE dict of the
    gt_sampling config, applied in its order as database_sampler.py:25-26 does.  Objects are numbered class by class in
    `class_names` order; `class_ids[name][k]` is the object the reference calls db_infos[name][k]."""

    def __init__(self, db_infos, root_path, class_names, prepare=None, num_point_features=4, device="cuda:0"):
        self.root_path = None if root_path is None else str(root_path)
        self.class_names = list(class_names)
        self.num_point_features = int(num_point_features)
        self.device = torch.device(device)
        infos = {c: list(db_infos.get(c, [])) for c in self.class_names}
        for func_name, val in (prepare or {}).items():
            infos = getattr(self, func_name)(infos, val)
        self.records, self.class_ids = [], OrderedDict()
        for c in self.class_names:
            self.class_ids[c] = np.arange(len(self.records), len(self.records) + len(infos[c]), dtype=np.int64)
            self.records.extend(infos[c])
        self.obj_box = np.zeros((len(self.records), 7), np.float32)
        for i, r in enumerate(self.records):
            self.obj_box[i] = np.asarray(r["box3d_lidar"])[:7]
        self._host = None
        self._dev = None

    @classmethod
    def from_db_info_files(cls, root_path, db_info_paths, class_names, **kw):
        """database_sampler.py:19-23: the pickles of DB_INFO_PATH, concatenated per class."""
        infos = {c: [] for c in class_names}
        for p in db_info_paths:
            with open(os.path.join(str(root_path), p), "rb") as f:
                d = pickle.load(f)
            for c in class_names:
                infos[c].extend(d.get(c, []))
        return cls(infos, root_path, class_names, **kw)

    @classmethod
    def from_arrays(cls, names, boxes, points, class_names, num_points_in_gt=None, difficulty=None, **kw):
        """names (n,), boxes (n, 7), points: n arrays (p_i, F) in the object's own frame (box centre at the origin)."""
        infos = {}
        for i, name in enumerate(names):
            pts = np.ascontiguousarray(points[i], np.float32)
            infos.setdefault(str(name), []).append({
                "name": str(name), "path": None, "points": pts, "box3d_lidar": np.asarray(boxes[i]),
                "num_points_in_gt": int(pts.shape[0] if num_points_in_gt is None else num_points_in_gt[i]),
                "difficulty": int(0 if difficulty is None else difficulty[i])})
        kw.setdefault("num_point_features", int(points[0].shape[1]) if len(points) else 4)
        return cls(infos, None, class_names, **kw)

    @classmethod
    def from_device(cls, db_infos, arena, rows_of, class_names, **kw):
        """A bank over points that are already on the device (hvpr_amd.gt_database.DatabaseBuilder).  `arena` (rows, F) float32
        device tensor; `rows_of[id(record)]` = (first row, rows) of that record's points in it.  The PREPARE filters run on the
        records as ever; the survivors' segments are gathered into the bank's order on the device, and the host copy
        (`host_points`) is made from that only when someone asks."""
        kw.setdefault("num_point_features", int(arena.shape[1]))
        kw.setdefault("device", arena.device)
        bank = cls(db_infos, None, class_names, **kw)
        seg = np.asarray([rows_of[id(r)] for r in bank.records], np.int64).reshape(-1, 2)
        off = np.zeros((len(bank.records) + 1,), np.int64)
        off[1:] = np.cumsum(seg[:, 1])
        idx = np.arange(off[-1], dtype=np.int64) + np.repeat(seg[:, 0] - off[:-1], seg[:, 1])     # bank row -> arena row
        if off[-1] > 0:
            pts = preprocess.gather_rows(arena, torch.from_numpy(idx.astype(np.int32)).to(arena.device))
        else:
            pts = torch.zeros((0, bank.num_point_features), dtype=torch.float32, device=arena.device)
        bank._dev = (pts, torch.from_numpy(bank.obj_box).to(arena.device))
        bank._dev_off = off
        return bank

    @staticmethod
    def filter_by_difficulty(db_infos, removed_difficulty):
        return {k: [i for i in v if i["difficulty"] not in removed_difficulty] for k, v in db_infos.items()}

    @staticmethod
    def filter_by_min_points(db_infos, min_gt_points_list):
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(":")
            min_num = int(min_num)
            if min_num > 0 and name in db_infos:
                db_infos[name] = [i for i in db_infos[name] if i["num_points_in_gt"] >= min_num]
        return db_infos

    def __len__(self):
        return len(self.records)

    def host_points(self):
        """(arena (P_total, F) f32, obj_off (n+1) i64): every object's points, loaded once (database_sampler.py:132-134)."""
        if self._host is None and getattr(self, "_dev_off", None) is not None:       # from_device: the arena is the source
            self._host = (np.ascontiguousarray(self._dev[0].cpu().numpy(), np.float32), self._dev_off)
        if self._host is None:
            F, parts = self.num_point_features, []
            for r in self.records:
                if r.get("points") is not None:
                    parts.append(np.asarray(r["points"], np.float32).reshape(-1, F))
                else:
                    parts.append(np.fromfile(os.path.join(self.root_path, r["path"]), dtype=np.float32).reshape(-1, F))
            off = np.zeros((len(parts) + 1,), np.int64)
            off[1:] = np.cumsum([p.shape[0] for p in parts])
            arena = np.concatenate(parts, axis=0) if parts else np.zeros((0, F), np.float32)
            self._host = (np.ascontiguousarray(arena, np.float32), off)
        return self._host

    def on_device(self):
        """(arena, obj_box) as device tensors, made on first use."""
        if self._dev is None:
            arena, _ = self.host_points()
            self._dev = (torch.from_numpy(arena).to(self.device), torch.from_numpy(self.obj_box).to(self.device))
        return self._dev


# ------------------------------------------------------------------------------------------------ road plane
def put_boxes_on_road_planes(gt_boxes, road_plane, calib):
    """database_sampler.py:99-116.  Row-wise, so it may run over every candidate before the collision test decides."""
    a, b, c, d = road_plane
    center_cam = lidar_to_rect(gt_boxes[:, 0:3], calib)
    cur_height_cam = (-d - a * center_cam[:, 0] - c * center_cam[:, 2]) / b
    center_cam[:, 1] = cur_height_cam
    cur_lidar_height = rect_to_lidar(center_cam, calib)[:, 2]
    mv_height = gt_boxes[:, 2] - gt_boxes[:, 5] / 2 - cur_lidar_height
    gt_boxes[:, 2] -= mv_height
    return gt_boxes, mv_height


def fakelidar_to_lidar(boxes):
    """box_utils.py:108-119."""
    w, l, h, r = boxes[:, 3:4], boxes[:, 4:5], boxes[:, 5:6], boxes[:, 6:7]
    boxes[:, 2] += h[:, 0] / 2
    return np.concatenate([boxes[:, 0:3], l, w, h, -(r + np.pi / 2)], axis=-1)


# ------------------------------------------------------------------------------------------------ the RNG protocol
class AugmentPlanner:
    """Needs the bank's host side only (records, per-class lists): no GPU."""

    def __init__(self, augmentor_cfg, class_names, bank):
        self.class_names, self.bank = list(class_names), bank
        cfgs = augmentor_cfg if isinstance(augmentor_cfg, list) else augmentor_cfg["AUG_CONFIG_LIST"]
        disabled = [] if isinstance(augmentor_cfg, list) else _get(augmentor_cfg, "DISABLE_AUG_LIST", [])
        self.queue = [c for c in cfgs if c["NAME"] not in disabled]              # data_augmentor.py:19-24
        self.sampler_cfg, self.groups, self.sample_class_num, ops = None, OrderedDict(), {}, []
        for k, c in enumerate(self.queue):
            name = c["NAME"]
            if name == "gt_sampling":
                if self.sampler_cfg is not None or ops:
                    raise ValueError("gt_sampling must come once, before the world transforms (pasted objects take them too)")
                self.sampler_cfg = c
                for x in c["SAMPLE_GROUPS"]:                                     # database_sampler.py:31-40
                    cname, num = x.split(":")
                    if cname not in self.class_names:
                        continue
                    n = len(bank.class_ids[cname])
                    if n == 0:
                        raise ValueError(f"gt_sampling: no {cname} object survives the PREPARE filters")
                    self.sample_class_num[cname] = num
                    self.groups[cname] = {"sample_num": num, "pointer": n, "indices": np.arange(n)}
            elif name == "random_world_flip":
                for ax in c["ALONG_AXIS_LIST"]:
                    assert ax in ("x", "y")
                    ops.append(OP_FLIP_X if ax == "x" else OP_FLIP_Y)
            elif name == "random_world_rotation":
                ops.append(OP_ROTATE)
            elif name == "random_world_scaling":
                r = c["WORLD_SCALE_RANGE"]
                if not r[1] - r[0] < 1e-3:                                       # augmentor_utils.py:73-74: no draw, no change
                    ops.append(OP_SCALE)
            else:
                raise ValueError(f"unknown augmentor {name}")
        if len(set(ops)) != len(ops) or len(ops) > 8:
            raise ValueError("each world transform (flip x, flip y, rotation, scaling) may be configured once")
        self.ops = ops
        self.ops_word = sum(op << (4 * k) for k, op in enumerate(ops))
        s = self.sampler_cfg or {}
        self.limit_whole_scene = bool(_get(s, "LIMIT_WHOLE_SCENE", False))
        self.use_road_plane = bool(_get(s, "USE_ROAD_PLANE", False))
        self.fakelidar = bool(_get(s, "DATABASE_WITH_FAKELIDAR", False))
        self.extra_width = np.asarray(_get(s, "REMOVE_EXTRA_WIDTH", [0.0, 0.0, 0.0]), np.float32)

    @property
    def num_groups(self):
        return len(self.groups)

    def reset(self):
        """The sampler's per-class state as the constructor leaves it (database_sampler.py:31-40): what a freshly forked worker
        of the reference starts an epoch with."""
        for cname, grp in self.groups.items():
            n = len(self.bank.class_ids[cname])
            grp.update(sample_num=self.sample_class_num[cname], pointer=n, indices=np.arange(n))

    def _sample_with_fixed_number(self, class_name, grp, rng):
        """database_sampler.py:79-96, returning indices into the class list."""
        sample_num, pointer, indices = int(grp["sample_num"]), grp["pointer"], grp["indices"]
        n = len(self.bank.class_ids[class_name])
        if pointer >= n:
            indices = rng.permutation(n)
            pointer = 0
        picked = indices[pointer: pointer + sample_num]
        grp["pointer"], grp["indices"] = pointer + sample_num, indices
        return picked

    def plan_frame(self, gt_names, calib=None, road_plane=None, rng=np.random):
        """The draws of one DataAugmentor.forward, in queue order."""
        gt_names = np.asarray(gt_names).astype(str)
        NG = self.num_groups
        plan = {"cand_obj": np.zeros((0,), np.int64), "group_off": np.zeros((NG + 1,), np.int64),
                "cand_box": np.zeros((0, 7), np.float32), "cand_mv": np.zeros((0,), np.float32),
                "cand_cls": np.zeros((0,), np.int32), "group_idx": [np.zeros((0,), np.int64)] * NG,
                "flip_x": False, "flip_y": False, "angle": 0.0, "cos": np.float32(1.0), "sin": np.float32(0.0),
                "scale": np.float32(1.0)}
        for c in self.queue:
            name = c["NAME"]
            if name == "gt_sampling":
                objs, boxes, cls, idxs, off = [], [], [], [], [0]
                for cname, grp in self.groups.items():
                    picked = np.zeros((0,), np.int64)
                    if self.limit_whole_scene:
                        grp["sample_num"] = str(int(self.sample_class_num[cname]) - int(np.sum(cname == gt_names)))
                    if int(grp["sample_num"]) > 0:
                        picked = np.asarray(self._sample_with_fixed_number(cname, grp, rng), np.int64)
                        ids = self.bank.class_ids[cname][picked]
                        b = np.stack([self.bank.records[i]["box3d_lidar"] for i in ids], axis=0).astype(np.float32)
                        if self.fakelidar:
                            b = fakelidar_to_lidar(b)
                        objs.append(ids)
                        boxes.append(b[:, 0:7].astype(np.float32))
                        cls.append(np.full((len(ids),), self.class_names.index(cname) + 1, np.int32))
                    idxs.append(picked)
                    off.append(off[-1] + len(picked))
                plan["group_idx"], plan["group_off"] = idxs, np.asarray(off, np.int64)
                if objs:
                    plan["cand_obj"], plan["cand_cls"] = np.concatenate(objs), np.concatenate(cls)
                    cb = np.ascontiguousarray(np.concatenate(boxes, axis=0))
                    mv = np.zeros((cb.shape[0],), np.float32)
                    if self.use_road_plane and road_plane is not None:
                        cb, mv = put_boxes_on_road_planes(cb, road_plane, calib)
                    plan["cand_box"], plan["cand_mv"] = cb.astype(np.float32), np.asarray(mv, np.float32)
            elif name == "random_world_flip":
                for ax in c["ALONG_AXIS_LIST"]:
                    plan["flip_" + ax] = bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))
            elif name == "random_world_rotation":
                r = c["WORLD_ROT_ANGLE"]
                r = r if isinstance(r, list) else [-r, r]
                plan["angle"] = rng.uniform(r[0], r[1])
                a = torch.from_numpy(np.array([plan["angle"]])).float()          # common_utils.rotate_points_along_z
                plan["cos"], plan["sin"] = torch.cos(a).numpy()[0], torch.sin(a).numpy()[0]
            elif name == "random_world_scaling" and OP_SCALE in self.ops:
                r = c["WORLD_SCALE_RANGE"]
                plan["scale"] = np.float32(rng.uniform(r[0], r[1]))
        return plan


# ------------------------------------------------------------------------------------------------ the packed plan
def plan_words(B, NG, G, C):
    return PLAN_HEADER + (B + 1) + (B * NG + 1) + (B + 1) + G + 5 * C + 7 * G + 7 * C + C + 8 * B


def pack_plans(buf, plans, gt_boxes, gt_cls, point_counts, ops_word, NG, obj_off):
    """Fills `buf` (int32 numpy view of the staging buffer; layout: csrc/augment.hip) and returns the words used."""
    B = len(plans)
    G = int(sum(len(g) for g in gt_boxes))
    C = int(sum(len(p["cand_obj"]) for p in plans))
    n = plan_words(B, NG, G, C)
    if n > buf.shape[0]:
        raise ValueError("augment plan does not fit its staging buffer")
    w = buf[:n]
    w[:PLAN_HEADER] = [PLAN_MAGIC, B, NG, G, C, ops_word, 0, 0]
    pos = [PLAN_HEADER]

    def take(k, dtype=np.int32):
        v = w[pos[0]: pos[0] + k].view(dtype)
        pos[0] += k
        return v

    gt_off, grp_off, pt_off = take(B + 1), take(B * NG + 1), take(B + 1)
    gcls, cobj, ccls, cfrm, cstart, cn = take(G), take(C), take(C), take(C), take(C), take(C)
    gbox, cbox, cmv, xf = take(7 * G, np.float32), take(7 * C, np.float32), take(C, np.float32), take(8 * B, np.float32)
    gt_off[0] = grp_off[0] = pt_off[0] = 0
    g = c = 0
    for f, p in enumerate(plans):
        ng, nc = len(gt_boxes[f]), len(p["cand_obj"])
        gbox[7 * g: 7 * (g + ng)] = np.asarray(gt_boxes[f], np.float32).reshape(-1)
        gcls[g: g + ng] = gt_cls[f]
        cbox[7 * c: 7 * (c + nc)] = p["cand_box"].reshape(-1)
        cobj[c: c + nc], ccls[c: c + nc], cfrm[c: c + nc], cmv[c: c + nc] = p["cand_obj"], p["cand_cls"], f, p["cand_mv"]
        cstart[c: c + nc] = obj_off[p["cand_obj"]]
        cn[c: c + nc] = obj_off[p["cand_obj"] + 1] - obj_off[p["cand_obj"]]
        grp_off[f * NG + 1: (f + 1) * NG + 1] = c + p["group_off"][1:]
        g, c = g + ng, c + nc
        gt_off[f + 1], pt_off[f + 1] = g, pt_off[f] + int(point_counts[f])
        xf[8 * f: 8 * f + 8] = [float(p["flip_x"]), float(p["flip_y"]), p["cos"], p["sin"], np.float32(p["angle"]), p["scale"], 0, 0]
    return n


# ------------------------------------------------------------------------------------------------ the public class
class DeviceAugmentor:
    """augmentor_cfg: the DATA_AUGMENTOR block (or a bare AUG_CONFIG_LIST).  `__call__(frames, rng)` takes a list of frames,
    each a dict with device `points` (N_i, F) float32, host `gt_boxes` (G_i, 7), host `gt_names` (G_i,), optional `calib`
    (dict of Tr_velo2cam / R0 / P2) and `road_plane`; or, with `points=` and `point_counts=`, one ragged device array
    (sum N_i, F) whose frames lie end to end with the host-known sizes `point_counts`.

    Returns a dict: `points` (sum M_i, F) and `point_frame_offsets` (B+1,) int32 on the device, `gt_boxes` (B, G_cap, 8) on the
    device (zero-padded, column 7 = class index + 1: what the target assigner reads), and after the ONE host read of the call
    `num_points` (B,) and `num_boxes` (B,) as numpy, plus `valid` (device, per candidate) and `plans` (the host draws).
    A frame with num_boxes == 0 is the caller's to redraw (dataset.py:127-129)."""

    def __init__(self, augmentor_cfg, class_names, bank, point_cloud_range, remove_outside_boxes=True):
        self.class_names, self.bank = list(class_names), bank
        self.planner = AugmentPlanner(augmentor_cfg, class_names, bank)
        self.point_cloud_range = np.ascontiguousarray(point_cloud_range, np.float32)
        self.remove_outside_boxes = bool(remove_outside_boxes)
        self._stage = preprocess.PinnedBuffer()

    def __call__(self, frames, rng=np.random, points=None, point_counts=None):
        dev = self.bank.device
        B, NG = len(frames), self.planner.num_groups
        if points is None:
            per = [f["points"] for f in frames]
            point_counts = [int(p.shape[0]) for p in per]
            if len({int(p.shape[1]) for p in per}) != 1:
                raise ValueError("frames of one batch must share a point feature width")
            points = per[0] if B == 1 else torch.cat(per, dim=0)
        points = points.contiguous()
        gt_boxes = [np.asarray(f["gt_boxes"], np.float32) for f in frames]
        gt_boxes = [b.reshape(-1, 7) if b.size == 0 else b[:, :7] for b in gt_boxes]
        gt_cls = [np.asarray([self.class_names.index(n) + 1 if n in self.class_names else 0
                              for n in np.asarray(f["gt_names"]).astype(str)], np.int32) for f in frames]
        plans = [self.planner.plan_frame(f["gt_names"], f.get("calib"), f.get("road_plane"), rng) for f in frames]
        _, obj_off = self.bank.host_points()
        G = sum(len(g) for g in gt_boxes)
        C = sum(len(p["cand_obj"]) for p in plans)
        stage = self._stage.take(plan_words(B, NG, G, C))
        words = pack_plans(stage.numpy(), plans, gt_boxes, gt_cls, point_counts, self.planner.ops_word, NG, obj_off)
        plan_dev = stage[:words].to(dev, non_blocking=True)                      # the one upload of the call
        g_cap = max(1, max(int((gt_cls[f] > 0).sum()) + len(plans[f]["cand_obj"]) for f in range(B)))
        out = kernels.augment_batch(stage, plan_dev, words, points, self.bank, self.planner.extra_width, self.point_cloud_range,
                                    self.remove_outside_boxes, g_cap)
        counts = out.pop("counts").cpu().numpy()                                 # the one read of the call
        off = counts[: B + 1]
        out["points"] = out["points"][: int(off[B])]
        out["num_points"], out["num_boxes"], out["plans"] = np.diff(off), counts[B + 1:].copy(), plans
        return out
