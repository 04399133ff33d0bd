"""Training (and test) batches on the device: everything between a frame's raw data and the `batch_dict` the detector reads, for
a whole batch at once.  Covers, with the reference's names,

  * KittiDataset.__getitem__ from the FOV filter on     pcdet/datasets/kitti/kitti_dataset.py:377-400
  * DatasetTemplate.prepare_data                        pcdet/datasets/dataset.py:95-146 (augmentor, redraw of a frame that ends
                                                        with no box, class filter, class column)
  * DataProcessor.mask_points_and_boxes_outside_range,
    shuffle_points                                      pcdet/datasets/processor/data_processor.py:20-39
  * DatasetTemplate.collate_batch                       dataset.py:148-180 (`points` with the batch column, `gt_boxes` padded to
                                                        the largest count of the batch)

`DataProcessor.sample_points` (data_processor.py:77-108) is opt-in (`sample_points=True`), see below.
`transform_points_to_voxels` stays the detector's.  The point work is csrc/collate.hip (select / shuffle / collate over one ragged
array with device-resident offsets) around the untouched kernels of csrc/augment.hip; every random number is numpy's, drawn on
the host in the reference's order.

Host reads.  A training batch without a redraw makes exactly TWO reads of the device (`DeviceBatchLoader._read`), whatever its
size: (1) the per-frame point counts after the FOV filter, which the augment plan needs; (2) one buffer with the augmented
offsets, the box counts, the per-frame sums of accepted candidates and the offsets after the range mask.  A test batch makes
ONE.  Every upload is a non-blocking copy from pinned memory.

The redraw test is the reference's: `len(data_dict['gt_boxes']) == 0` after DataAugmentor.forward, before the class filter and
the trim.  With a GT sampler in the queue that is the class-trained ground truths plus the accepted candidates when something
was pasted, but EVERY ground truth, trained class or not, when nothing was (the sampler pops `gt_boxes_mask`,
database_sampler.py:189, so forward's own filter never runs): a quirk kept, not fixed.  A frame whose boxes all fall to the trim
stays in the batch with zero boxes.  Redrawn slots are prepared one frame at a time after the batch and spliced in: extra reads
and a device copy on that rare path only.  The sampler's pointers advance in the order the frames are planned (the whole batch,
then the redrawn frames), so a redraw in the middle of a batch gives the frames behind it other objects than the reference's
frame-by-frame order would; with the redraw in the last slot the two orders are the same.

Order of the draws in `prepare_batch(indices, rng)`.  With a list of B generators, frame b consumes rng[b] exactly as one
`__getitem__` of the reference consumes `np.random`: the augmentor's draws; then, while the frame ends with no box,
`randint(num_frames)` and the new frame's augmentor draws; then `permutation(M)`.  With ONE generator the order is: the
augmentor draws of all frames, in frame order; then each empty frame's redraw chain, in frame order; then the permutations, in
frame order.  (The reference's single-process loader would interleave them per frame; a seeded run that must match it frame for
frame passes one generator per frame.)

`sample_points` (with `sample_points=True`, between the range mask and the shuffle).  The reference's draws depend on a frame
only through n, the rows the mask keeps, c, how many of them are near (||xyz|| < 40), and P = NUM_POINTS[mode]:
`rng.choice(a, k, replace=False)` is `a[rng.choice(np.arange(len(a)), k, replace=False)]`, and `rng.shuffle` moves positions
whatever the values.  So `plan_sample_points` draws over ORDINALS (a near row's position among the frame's near kept rows, a far
row's among the far ones, or the plain in-frame rank) from the two counts, call for call as the reference
does, composes the following permutation, and the write pass of csrc/collate.hip turns each kept row's two ranks into its ordinal
and scatters it through the resulting table.  The near counts ride in read 2 of a training batch and in the one read of a test
batch (which samples too): no read is added.  A frame the reference refuses (more far rows than P, P - n > n, an empty frame)
raises the reference's ValueError before the write pass is launched.  Every frame then has exactly P rows.  With one generator
per frame the frame's draws go on: ..., `sample_points`' draws, `permutation(P)`; with ONE generator the third phase is, per
frame in frame order, the sample draws followed by the permutation.  NUM_POINTS -1 is the reference's no-op.
"""
import numpy as np
import torch

from . import augment as AUG
from . import calibration, kernels, preprocess
from .config import _get
from .preprocess import PinnedBuffer, plan_sample_points, resolve_sample_choice, to_device

NEAR = 40.0                # data_processor.py:88

SUPPORTED_PROCESSORS = ("mask_points_and_boxes_outside_range", "shuffle_points", "transform_points_to_voxels")


def sample_destinations(order, n):
    """(n, 2) int32: for every source ordinal the output rows it goes to, -1 for none (two only where a frame is padded)."""
    dest = np.full((n, 2), -1, np.int32)
    order = np.asarray(order)
    rows = np.arange(len(order), dtype=np.int32)
    dest[order[::-1], 0] = rows[::-1]               # a repeated index keeps the last value assigned: the first output row
    again = dest[order, 0] != rows                  # the second output row of a source that has two
    dest[order[again], 1] = rows[again]
    return dest


class DeviceBatchLoader:
    """dataset_cfg: the DATA_CONFIG block (POINT_CLOUD_RANGE, FOV_POINTS_ONLY, DATA_PROCESSOR and, for training,
    DATA_AUGMENTOR).  `frame_source(index)` returns what `__getitem__` holds before the FOV filter, as a dict: `points`
    (N, F) float32 on the device, `gt_boxes` (G, 7) lidar boxes and `gt_names` (G,) on the host (optional in test mode), `calib`
    (a dict of Tr_velo2cam / R0 / P2 or the reference's Calibration), `image_shape`, `frame_id`, optionally `road_plane`.
    `num_frames` is the dataset's length (the redraw draws `randint(num_frames)`); `bank` the ObjectBank of the GT sampler.

    `prepare_batch(indices, rng)` returns the batch_dict: `points` (sum M, 1 + F) and `point_frame_offsets` (B + 1,) int32 on the
    device, `gt_boxes` (B, max_gt, 8) on the device, `batch_size`, and the host lists `frame_id`, `calib`, `image_shape`;
    `overflow` is a device word that stays 0 (never read here).  With `sample_points=True` a `sample_points` step between the
    range mask and the shuffle is taken: every frame has NUM_POINTS rows.  `debug_choices=True` adds `choices`, each frame's
    resolved `choice` of the reference, at the price of one more read."""

    def __init__(self, dataset_cfg, class_names, frame_source, num_frames, bank=None, training=True, device="cuda:0",
                 sample_points=False, debug_choices=False):
        self.class_names, self.frame_source, self.num_frames = list(class_names), frame_source, int(num_frames)
        self.training, self.bank = bool(training), bank
        self.device = torch.device(device) if bank is None else bank.device
        self.point_cloud_range = np.ascontiguousarray(dataset_cfg["POINT_CLOUD_RANGE"], np.float32)
        self.range_xy = np.ascontiguousarray(self.point_cloud_range[[0, 1, 3, 4]])
        self.fov_points_only = bool(_get(dataset_cfg, "FOV_POINTS_ONLY", False))
        self.mask_range = self.remove_outside_boxes = self.shuffle = False
        self.num_points, self.debug_choices = None, bool(debug_choices)
        for p in dataset_cfg["DATA_PROCESSOR"]:
            name = p["NAME"]
            if name == "sample_points" and sample_points:
                if not self.mask_range or self.shuffle:
                    raise NotImplementedError("DeviceBatchLoader: sample_points is taken behind "
                                              "mask_points_and_boxes_outside_range and in front of shuffle_points only")
                if self.num_points is not None:
                    raise NotImplementedError("DeviceBatchLoader: sample_points twice")
                self.num_points = int(p["NUM_POINTS"]["train" if self.training else "test"])
                continue
            if name not in SUPPORTED_PROCESSORS:
                raise NotImplementedError(f"DeviceBatchLoader: DATA_PROCESSOR step '{name}' is not handled here "
                                          f"(sample_points is taken with the keyword sample_points=True only)")
            if name == "mask_points_and_boxes_outside_range":
                if self.shuffle or self.num_points is not None:
                    raise NotImplementedError("DeviceBatchLoader: shuffle_points or sample_points in front of "
                                              "mask_points_and_boxes_outside_range")
                if _get(p, "min_num_corners", 1) != 1:
                    raise NotImplementedError("DeviceBatchLoader: min_num_corners other than 1")
                self.mask_range = True
                self.remove_outside_boxes = bool(_get(p, "REMOVE_OUTSIDE_BOXES", False)) and self.training
            elif name == "shuffle_points":
                self.shuffle = bool(p["SHUFFLE_ENABLED"]["train" if self.training else "test"])
        if self.num_points == -1:                                                # the reference's no-op
            self.num_points = None
        elif self.num_points is not None and self.num_points < 0:
            raise ValueError("DeviceBatchLoader: NUM_POINTS must be -1 or a count")
        self.planner = None
        if self.training:
            if bank is None:
                raise ValueError("DeviceBatchLoader: training needs the ObjectBank of the GT sampler")
            self.planner = AUG.AugmentPlanner(dataset_cfg["DATA_AUGMENTOR"], self.class_names, bank)
        self._stage = PinnedBuffer()
        # the destination table and the mode words of a sampled batch: the upload of batch k is enqueued before the reads of
        # batch k + 1, and the buffer is written again only after them
        self._table = PinnedBuffer()
        self.reads = 0

    # -------------------------------------------------------------------------------------------- the only host reads
    def _read(self, tensor):
        self.reads += 1
        return tensor.cpu().numpy()

    def _up(self, array):
        return to_device(array, self.device)

    # -------------------------------------------------------------------------------------------- pieces
    def _count(self, points, off, mask, calib=None):
        """(new_off, near_off or None, workspace): the count pass, with the near counts when the batch is sampled."""
        if self.num_points is None:
            new_off, ws = kernels.ragged_select_count(points, off, mask, calib=calib, range_xy=self.range_xy)
            return new_off, None, ws
        return kernels.ragged_sample_count(points, off, mask, calib=calib, range_xy=self.range_xy, near=NEAR)

    def _ragged(self, frames):
        per = [f["points"] for f in frames]
        if len({int(p.shape[1]) for p in per}) != 1:
            raise ValueError("frames of one batch must share a point feature width")
        counts = [int(p.shape[0]) for p in per]
        points = per[0].contiguous() if len(per) == 1 else torch.cat(per, dim=0)
        off = self._up(np.cumsum([0] + counts).astype(np.int32))
        return points, off, counts

    def _calib(self, frames):
        return self._up(calibration.pack_calib([f["calib"] for f in frames], [f["image_shape"] for f in frames]))

    @staticmethod
    def _batch(frames, points, offsets, flag, perms):
        """The batch dict without the boxes: the device fields as given, the host fields from the frames."""
        return {"points": points, "point_frame_offsets": offsets, "batch_size": len(frames), "overflow": flag,
                "frame_id": [f.get("frame_id") for f in frames], "calib": [f.get("calib") for f in frames],
                "image_shape": [f.get("image_shape") for f in frames], "permutations": perms}

    def _augment_stage(self, frames, rngs):
        """FOV select, read 1, the augmentor's draws, the augment kernels, the range count, read 2: the frames as ragged
        augmented points with everything the host has to know about them."""
        B, NG = len(frames), self.planner.num_groups
        points, off, counts = self._ragged(frames)
        if self.fov_points_only:
            calib = self._calib(frames)
            fov_off, ws = kernels.ragged_select_count(points, off, 1, calib=calib)
            points, _ = kernels.ragged_select_write(points, off, 1, fov_off, ws, calib=calib)
            fov_off = self._read(fov_off)                                        # read 1
            counts = np.diff(fov_off).tolist()
            points = points[: int(fov_off[B])]
        gt_boxes = [np.asarray(f["gt_boxes"], np.float32) for f in frames]
        gt_boxes = [b.reshape(-1, 7) if b.size == 0 else b[:, :7] for b in gt_boxes]
        gt_cls = [np.asarray([self.class_names.index(n) + 1 if n in self.class_names else 0
                              for n in np.asarray(f["gt_names"]).astype(str)], np.int32) for f in frames]
        plans = [self.planner.plan_frame(f["gt_names"], calibration.as_dict(f.get("calib")), f.get("road_plane"), r) for f, r in zip(frames, rngs)]
        _, obj_off = self.bank.host_points()
        G = sum(len(g) for g in gt_boxes)
        C = sum(len(p["cand_obj"]) for p in plans)
        stage = self._stage.take(AUG.plan_words(B, NG, G, C))
        words = AUG.pack_plans(stage.numpy(), plans, gt_boxes, gt_cls, counts, self.planner.ops_word, NG, obj_off)
        plan_dev = stage[:words].to(self.device, non_blocking=True)
        n_gt = np.asarray([int((c > 0).sum()) for c in gt_cls], np.int64)
        g_cap = max(1, max(int(n_gt[f]) + len(plans[f]["cand_obj"]) for f in range(B)))
        out = kernels.augment_batch(stage, plan_dev, words, points, self.bank, self.planner.extra_width, self.point_cloud_range,
                                    self.remove_outside_boxes, g_cap)
        aug_off = out["counts"][: B + 1]
        new_off, near_off, ws = self._count(out["points"], aug_off, 2 if self.mask_range else 0)
        # accepted candidates per frame: the prefix sums of `valid` at the host-known candidate offsets
        cand_off = np.cumsum([0] + [len(p["cand_obj"]) for p in plans]).astype(np.int64)
        prefix = torch.cat([torch.zeros((1,), dtype=torch.int32, device=self.device),
                            torch.cumsum(out["valid"], 0, dtype=torch.int32)])
        at = prefix.index_select(0, self._up(cand_off))
        accepted = at[1:] - at[:-1]
        host = self._read(torch.cat([out["counts"], accepted, new_off] + ([] if near_off is None else [near_off])))   # read 2
        n_accepted = host[2 * B + 1: 3 * B + 1].astype(np.int64)
        n_all = np.asarray([len(c) for c in gt_cls], np.int64)
        # what `len(data_dict['gt_boxes'])` is after DataAugmentor.forward (see the module docstring)
        after_augmentor = np.where((n_accepted > 0) | (self.planner.sampler_cfg is None), n_gt + n_accepted, n_all)
        st = {"frames": list(frames), "points": out["points"], "aug_off_dev": aug_off, "aug_off": host[: B + 1].astype(np.int64),
              "num_boxes": host[B + 1: 2 * B + 1].astype(np.int64), "boxes_before_trim": after_augmentor,
              "new_off_dev": new_off, "new_off": host[3 * B + 1: 4 * B + 2].astype(np.int64), "gt_boxes": out["gt_boxes"], "ws": ws,
              "plans": plans, "near_off_dev": near_off, "near_off": host[4 * B + 2:].astype(np.int64)}
        return st

    def _splice(self, st, redrawn):
        """The batch with the redrawn slots put in: a device copy of the points and boxes, a fresh count pass over host-known
        offsets, no read."""
        B = len(st["frames"])
        seg, gts, rows, kept, frames, nb, near = [], [], [], [], [], [], []
        for f in range(B):
            s, k = (redrawn[f], 0) if f in redrawn else (st, f)
            seg.append(s["points"][int(s["aug_off"][k]): int(s["aug_off"][k + 1])])
            rows.append(int(s["aug_off"][k + 1] - s["aug_off"][k]))
            kept.append(int(s["new_off"][k + 1] - s["new_off"][k]))
            near.append(int(s["near_off"][k + 1] - s["near_off"][k]) if self.num_points is not None else 0)
            gts.append(s["gt_boxes"][k])
            nb.append(int(s["num_boxes"][k]))
            frames.append(s["frames"][k])
        g_cap = max(g.shape[0] for g in gts)
        gt = torch.zeros((B, g_cap, 8), dtype=torch.float32, device=self.device)
        for f, g in enumerate(gts):
            gt[f, : g.shape[0]] = g
        points = torch.cat(seg, dim=0)
        aug_off = np.cumsum([0] + rows).astype(np.int32)
        aug_off_dev = self._up(aug_off)
        new_off_dev, near_off_dev, ws = self._count(points, aug_off_dev, 2 if self.mask_range else 0)
        return {"frames": frames, "points": points, "aug_off_dev": aug_off_dev, "aug_off": aug_off.astype(np.int64),
                "num_boxes": np.asarray(nb, np.int64), "new_off_dev": new_off_dev, "new_off": np.cumsum([0] + kept).astype(np.int64),
                "gt_boxes": gt, "ws": ws, "near_off_dev": near_off_dev, "near_off": np.cumsum([0] + near).astype(np.int64)}

    def _finish(self, frames, points, off_dev, mask, new_off_dev, new_off, ws, rngs, calib=None):
        """The permutations (host) and the write pass with the batch column."""
        total = int(new_off[-1])
        inv = None
        perms = []
        if self.shuffle:
            flat = np.empty((total,), np.int32)
            for b, r in enumerate(rngs):
                m = int(new_off[b + 1] - new_off[b])
                perm = r.permutation(m)
                flat[int(new_off[b]) + perm] = np.arange(m, dtype=np.int32)     # the inverse: where each kept row goes
                perms.append(perm)
            inv = self._up(flat) if total else None
        out = torch.empty((total, points.shape[1] + 1), dtype=torch.float32, device=self.device)
        flag = torch.zeros((1,), dtype=torch.int32, device=self.device)
        kernels.ragged_select_write(points, off_dev, mask, new_off_dev, ws, calib=calib, range_xy=self.range_xy, inv_perm=inv,
                                    batch_column=True, out=out, flag=flag)
        return self._batch(frames, out, new_off_dev, flag, perms)

    def _finish_sampled(self, frames, points, off_dev, mask, new_off_dev, near_off_dev, new_off, near_off, ws, rngs, calib=None):
        """sample_points' draws and the permutations (host), then the write pass through the destination table: every frame
        gets exactly NUM_POINTS rows."""
        B, P, total = len(frames), self.num_points, int(new_off[-1])
        stage = self._table.take(2 * total + B)                                 # pinned, kept from batch to batch
        dest, mode = stage.numpy()[: 2 * total].reshape(total, 2), stage.numpy()[2 * total: 2 * total + B]
        perms, plans = [], []
        for b, r in enumerate(rngs):                                             # raises before the write pass is launched
            n, c = int(new_off[b + 1] - new_off[b]), int(near_off[b + 1] - near_off[b])
            plan = plan_sample_points(n, c, P, r, shuffle=self.shuffle)
            dest[int(new_off[b]): int(new_off[b + 1])] = sample_destinations(plan["order"], n)
            mode[b] = plan["mode"]
            plans.append(plan)
            if self.shuffle:
                perms.append(plan["perm"])
        table = stage[: 2 * total + B].to(self.device, non_blocking=True)
        out = torch.empty((B * P, points.shape[1] + 1), dtype=torch.float32, device=self.device)
        flag = torch.zeros((1,), dtype=torch.int32, device=self.device)
        kernels.ragged_sample_write(points, off_dev, mask, new_off_dev, near_off_dev, table[2 * total:],
                                    table[: 2 * total].view(total, 2), P, ws, calib=calib, range_xy=self.range_xy, near=NEAR,
                                    batch_column=True, out=out, flag=flag)
        batch = self._batch(frames, out, self._up(np.arange(B + 1, dtype=np.int32) * P), flag, perms)
        if self.debug_choices:                                                   # the near flags of the kept rows: one more read
            # the workspace of the sample count begins with the layout the select write reads (csrc/collate.hip, carve)
            kept, _ = kernels.ragged_select_write(points, off_dev, mask, new_off_dev, ws, calib=calib, range_xy=self.range_xy)
            near = self._read(preprocess._flags(kept[:total].contiguous(), 1, near=NEAR)) if total else np.zeros((0,), np.uint8)
            batch["choices"] = [resolve_sample_choice(p, near[int(new_off[b]): int(new_off[b + 1])]) for b, p in enumerate(plans)]
        return batch

    # -------------------------------------------------------------------------------------------- the entry point
    def prepare_batch(self, indices, rng=np.random):
        indices = [int(i) for i in indices]
        B = len(indices)
        rngs = list(rng) if isinstance(rng, (list, tuple)) else [rng] * B
        if len(rngs) != B:
            raise ValueError("one generator, or one per frame of the batch")
        frames = [self.frame_source(i) for i in indices]
        if not self.training:
            return self._test_batch(frames, rngs)
        st = self._augment_stage(frames, rngs)
        redrawn, redraw_index = {}, {}
        for f in np.nonzero(st["boxes_before_trim"] == 0)[0].tolist():           # dataset.py:127-129, rare
            redraw_index[f] = []
            while True:
                new_index = int(rngs[f].randint(self.num_frames))
                redraw_index[f].append(new_index)
                sub = self._augment_stage([self.frame_source(new_index)], [rngs[f]])
                if sub["boxes_before_trim"][0] > 0:
                    break
            redrawn[f] = sub
        if redrawn:
            st = self._splice(st, redrawn)
        if self.num_points is None:
            batch = self._finish(st["frames"], st["points"], st["aug_off_dev"], 2 if self.mask_range else 0, st["new_off_dev"],
                                 st["new_off"], st["ws"], rngs)
        else:
            batch = self._finish_sampled(st["frames"], st["points"], st["aug_off_dev"], 2 if self.mask_range else 0,
                                         st["new_off_dev"], st["near_off_dev"], st["new_off"], st["near_off"], st["ws"], rngs)
        max_gt = int(st["num_boxes"].max()) if B else 0
        batch["gt_boxes"] = st["gt_boxes"][:, :max_gt].contiguous()
        batch["num_boxes"], batch["redraw_index"] = st["num_boxes"], redraw_index
        return batch

    def _test_batch(self, frames, rngs):
        B = len(frames)
        points, off, _ = self._ragged(frames)
        mask = (1 if self.fov_points_only else 0) | (2 if self.mask_range else 0)
        calib = self._calib(frames) if mask & 1 else None
        new_off_dev, near_off_dev, ws = self._count(points, off, mask, calib=calib)
        if self.num_points is not None:
            host = self._read(torch.cat([new_off_dev, near_off_dev])).astype(np.int64)       # the one read
            batch = self._finish_sampled(frames, points, off, mask, new_off_dev, near_off_dev, host[: B + 1], host[B + 1:], ws,
                                         rngs, calib=calib)
        elif not self.shuffle:
            out, flag = kernels.ragged_select_write(points, off, mask, new_off_dev, ws, calib=calib, range_xy=self.range_xy,
                                                    batch_column=True)          # sized by the input rows: enqueued before the read
            new_off = self._read(new_off_dev)                                    # the one read
            batch = self._batch(frames, out[: int(new_off[B])], new_off_dev, flag, [])
        else:
            new_off = self._read(new_off_dev).astype(np.int64)
            batch = self._finish(frames, points, off, mask, new_off_dev, new_off, ws, rngs, calib=calib)
        if all(f.get("gt_boxes") is not None for f in frames):                   # dataset.py:131-137; no trim outside training
            rows = []
            for f in frames:
                names = np.asarray(f["gt_names"]).astype(str)
                sel = [i for i, n in enumerate(names) if n in self.class_names]
                cls = np.asarray([self.class_names.index(names[i]) + 1 for i in sel], np.float32).reshape(-1, 1)
                rows.append(np.concatenate([np.asarray(f["gt_boxes"], np.float32).reshape(-1, 7)[sel], cls], axis=1))
            gt = np.zeros((B, max(len(r) for r in rows), 8), np.float32)
            for k, r in enumerate(rows):
                gt[k, : len(r)] = r
            batch["gt_boxes"] = self._up(gt)
        return batch
