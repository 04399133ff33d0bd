"""Generate tests/golden/g23_sample_batch.npz: a training batch and a test batch through the reference's own data path with
`sample_points` in the DATA_PROCESSOR queue, between the range mask and the shuffle as in the reference's hvpr.yaml.

Runs only where the reference is.  It imports make_golden_batch.py (G22) and does not edit it: the database, the margins of the
scene points, the calibration and the augmentor configuration are G22's, and the reference code that runs is what runs there
plus DataProcessor.sample_points (pcdet/datasets/processor/data_processor.py:77-108), driven by the same kind of stand-in
subclass of DatasetTemplate.  NUM_POINTS is P = 192 in both modes.

One dataset of 6 frames.
  training batch [0, 1]
    frame 0   more than P rows behind the range mask, near and far ones (the draw over the near rows, the far rows appended)
    frame 1   P/2 <= n < P (padded by a draw without replacement: some rows twice)
  test batch [2, 3, 4, 5]: no augmentor, so the counts behind the FOV filter and the range mask are canned exactly
    frame 2   n > P          150 near + 100 far
    frame 3   n < P          90 near + 30 far
    frame 4   n == P         130 near + 62 far (no draw, the shuffle alone)
    frame 5   far == P       40 near + 192 far: `want == 0`, the draw over every row
Also stored, as booleans: the reference raises ValueError for a frame with P + 1 far rows and for one with 2 n < P.

The training seed is the first from SEED0 on for which no frame is redrawn, both frames show the above, and the margins hold,
asserted in float64: G22's (see make_golden_batch.py) and no row that reaches sample_points within 1e-3 m of norm 40.  The test
frames keep the same margins by construction.

Stored: the frames and the database; for each slot of either batch every draw in order (tags p permutation, c choice,
u uniform, r randint, s the array np.random.shuffle left), the resolved `choice`, the final permutation (training), n and c,
the numpy RNG state after the slot; the collated points and gt_boxes of both batches.
"""
import copy
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_batch as MGB  # noqa: E402

MG, MGA, AC = MGB.MG, MGB.MGA, MGB.AC
P = 192
NEAR = 40.0
SEED0 = 2300
TRAIN, TEST = [0, 1], [2, 3, 4, 5]
# kept near rows, kept far rows, rows the FOV filter or the range mask drops: before the augmentor for the training frames
COUNTS = [(150, 100, 120), (85, 45, 80), (150, 100, 200), (90, 30, 100), (130, 62, 150), (40, 192, 90)]
IMAGE_SHAPES = [[375, 1242], [370, 1224], [375, 1242], [376, 1241], [374, 1238], [375, 1242]]

DATASET_CFG = copy.deepcopy(MGB.DATASET_CFG)
DATASET_CFG["DATA_PROCESSOR"].insert(1, {"NAME": "sample_points", "NUM_POINTS": {"train": P, "test": P}})


def norm64(points):
    return np.sqrt((points[:, :3].astype(np.float64) ** 2).sum(axis=1))


def build_frames(R, get_fov_flag, db_boxes):
    """G22's scene points (with its margins) thinned to the canned counts, in a random order.  NOT G22's scene: the two
    assignments below replace, in the imported module and for this process only, the point count and the frame list its
    build_frames reads, so that it makes six frames of 2600 points with frame 0's ground truths (the file is not edited)."""
    MGB.N_SCENE, MGB.FRAMES = 2600, [dict(MGB.FRAMES[0], image_shape=s) for s in IMAGE_SHAPES]
    frames = MGB.build_frames(np.random.RandomState(230), db_boxes)
    gen = np.random.RandomState(231)
    calib = R.calibration.Calibration(dict(MGB.CALIB))
    for fr, (n_near, n_far, n_drop) in zip(frames, COUNTS):
        pts = fr["points"]
        pts = pts[np.abs(norm64(pts) - NEAR) >= 1e-2]
        xy, r64 = pts[:, :2].astype(np.float64), MGB.RANGE.astype(np.float64)
        pts = pts[np.minimum(np.abs(xy - r64[0:2]).min(axis=1), np.abs(xy - r64[3:5]).min(axis=1)) >= 1e-3]
        keep = get_fov_flag(calib.lidar_to_rect(pts[:, 0:3]), fr["image_shape"], calib)
        keep &= R.common_utils.mask_points_by_range(pts, MGB.RANGE)
        near = np.linalg.norm(pts[:, 0:3], axis=1) < NEAR
        groups = [np.where(keep & near)[0], np.where(keep & ~near)[0], np.where(~keep)[0]]
        assert all(len(g) >= k for g, k in zip(groups, (n_near, n_far, n_drop))), [len(g) for g in groups]
        pick = np.concatenate([gen.permutation(g)[:k] for g, k in zip(groups, (n_near, n_far, n_drop))])
        fr["points"] = np.ascontiguousarray(pts[np.sort(pick)][gen.permutation(len(pick))])
    return frames


def main():
    R = MGA.load_augmentor(MG.load_reference())
    MG._load("pcdet.datasets.processor.point_feature_encoder", "pcdet/datasets/processor/point_feature_encoder.py")
    ds_mod = MG._load("pcdet.datasets.dataset", "pcdet/datasets/dataset.py")
    get_fov_flag = MGB.get_fov_flag_of_reference()
    log = {"draws": [], "items": [], "groups": [], "range_in": [], "trim_in": []}

    class CannedDataset(ds_mod.DatasetTemplate):
        """KittiDataset.__getitem__ from the FOV filter on (kitti_dataset.py:377-400), over frames held in memory."""

        def __init__(self, frames, training, root):
            super().__init__(dataset_cfg=MG.EasyDict(DATASET_CFG), class_names=MGB.CLASS_NAMES, training=training, root_path=root)
            self.frames = frames

        def __len__(self):
            return len(self.frames)

        def __getitem__(self, index):
            log["items"].append(int(index))
            fr = self.frames[index]
            points, calib, img_shape = fr["points"].copy(), R.calibration.Calibration(dict(MGB.CALIB)), fr["image_shape"]
            if self.dataset_cfg.FOV_POINTS_ONLY:
                points = points[get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), img_shape, calib)]
            input_dict = {"points": points, "frame_id": str(index), "calib": calib, "gt_names": fr["gt_names"].copy(),
                          "gt_boxes": fr["gt_boxes"].copy(), "road_plane": fr["road_plane"].copy()}
            data_dict = self.prepare_data(data_dict=input_dict)
            data_dict["image_shape"] = img_shape
            return data_dict

    def spy(fn, tag):
        def w(*a, **k):
            r = fn(*a, **k)
            log["draws"].append((tag, np.atleast_1d(np.asarray(r, np.float64))))
            return r
        return w

    real_shuffle = np.random.shuffle

    def shuffle_spy(x):
        real_shuffle(x)
        log["draws"].append(("s", np.asarray(x, np.float64).copy()))

    real_mask = R.common_utils.mask_points_by_range
    real_trim = R.box_utils.mask_boxes_outside_range_numpy

    def mask_spy(points, limit_range):
        log["range_in"].append(np.array(points))
        return real_mask(points, limit_range)

    def trim_spy(boxes, limit_range, min_num_corners=1):
        log["trim_in"].append(np.array(boxes))
        return real_trim(boxes, limit_range, min_num_corners=min_num_corners)

    R.common_utils.mask_points_by_range = mask_spy
    R.box_utils.mask_boxes_outside_range_numpy = trim_spy

    tmp = Path(tempfile.mkdtemp(prefix="g23_db_"))
    db = MGB.build_database(tmp, np.random.RandomState(22))
    db_boxes = db["db.boxes"]
    frames = build_frames(R, get_fov_flag, db_boxes)
    ex = np.array(MGB.AUG_CFG["AUG_CONFIG_LIST"][0]["REMOVE_EXTRA_WIDTH"], np.float64)
    real = (np.random.permutation, np.random.choice, np.random.uniform, np.random.randint)
    r64 = MGB.RANGE.astype(np.float64)

    def run(training, indices, seed):
        """One batch under `seed`: per slot what was drawn and what reached the range mask, and the collated batch."""
        np.random.seed(seed)
        ds = CannedDataset(frames, training, tmp)
        groups = []
        if ds.training:
            sampler = ds.data_augmentor.data_augmentor_queue[0]
            real_sample = sampler.sample_with_fixed_number

            def sample(class_name, grp):
                r = real_sample(class_name, grp)
                groups.append([i["uid"] for i in r])
                return r

            sampler.sample_with_fixed_number = sample
        np.random.permutation, np.random.choice, np.random.uniform, np.random.randint = (spy(f, t) for f, t in zip(real, "pcur"))
        np.random.shuffle = shuffle_spy
        try:
            slots, items = [], []
            for b in indices:
                for k in log:
                    log[k] = []
                del groups[:]
                item = ds[b]
                st = np.random.get_state()
                kept = log["range_in"][-1][real_mask(log["range_in"][-1], MGB.RANGE)]
                slots.append({"items": list(log["items"]), "draws": list(log["draws"]), "groups": list(groups),
                              "range_in": list(log["range_in"]), "trim_in": list(log["trim_in"]), "kept": kept,
                              "state": (st[1].copy(), np.array([st[2], st[3]], np.int64), np.array(st[4], np.float64))})
                items.append(item)
        finally:
            np.random.permutation, np.random.choice, np.random.uniform, np.random.randint = real
            np.random.shuffle = real_shuffle
        batch = ds.collate_batch([{"points": i["points"], "gt_boxes": i["gt_boxes"]} for i in items])
        return slots, items, batch

    def margins(slots, training):
        for s in slots:
            assert len(s["range_in"]) == 1
            xy = s["range_in"][0][:, :2].astype(np.float64)
            if len(xy) and min(np.abs(xy - r64[0:2]).min(), np.abs(xy - r64[3:5]).min()) < 1e-3:
                return False
            if len(s["kept"]) and np.abs(norm64(s["kept"]) - NEAR).min() < 1e-3:
                return False
            if not training:
                continue
            assert len(s["trim_in"]) == 1 and len(s["groups"]) == 3 * len(s["items"])
            uid = [u for g in s["groups"] for u in g]
            cb = MGB.put_boxes_on_road_planes(db_boxes[uid].copy(), MGB.PLANE, MGB.CALIB)[0] if uid else np.zeros((0, 7), np.float32)
            fr, C = frames[s["items"][0]], R.calibration.Calibration(dict(MGB.CALIB))
            fov = get_fov_flag(C.lidar_to_rect(fr["points"][:, 0:3]), fr["image_shape"], C)
            if not AC.margins_ok(fr["points"][fov], fr["gt_boxes"], {"cand_box": cb}, ex, s["trim_in"][0], MGB.RANGE)[0]:
                return False
        return True

    def counts(s):
        return len(s["kept"]), int((np.linalg.norm(s["kept"][:, 0:3], axis=1) < NEAR).sum())

    found = None
    for seed in range(SEED0, SEED0 + 5000):
        try:
            slots, items, batch = run(True, TRAIN, seed)
        except ValueError:
            continue
        (n0, c0), (n1, c1) = counts(slots[0]), counts(slots[1])
        if any(len(s["items"]) != 1 for s in slots) or any(len(i["gt_boxes"]) == 0 for i in items):
            continue
        if not (n0 > P and 0 < n0 - c0 < P and c0 > 0 and P / 2 <= n1 < P) or not margins(slots, True):
            continue
        found = seed
        break
    assert found is not None, "no seed shows the scene"
    out = {"class_names": np.array(MGB.CLASS_NAMES), "range": MGB.RANGE, "prepare": np.array(json.dumps(MGB.PREPARE)),
           "config": np.array(json.dumps(DATASET_CFG)), "plane": MGB.PLANE, "num_frames": np.array(len(frames), np.int64),
           "num_sample_points": np.array(P, np.int64)}
    out.update(db)
    for k, v in MGB.CALIB.items():
        out["calib." + k] = v
    for i, fr in enumerate(frames):
        for k in ("points", "gt_boxes", "gt_names", "image_shape", "road_plane"):
            out[f"fr{i}.{k}"] = fr[k]

    def store(mode, seed, indices, slots, items, batch):
        out[mode + ".seed"], out[mode + ".indices"] = np.array(seed, np.int64), np.array(indices, np.int64)
        out[mode + ".points"], out[mode + ".gt_boxes"] = batch["points"], batch["gt_boxes"]
        assert batch["points"].dtype == np.float32 and batch["gt_boxes"].dtype == np.float32
        assert len(batch["points"]) == P * len(indices)
        for b, s in enumerate(slots):
            k = f"{mode}.b{b}."
            tags = "".join(t for t, _ in s["draws"])
            out[k + "items"] = np.array(s["items"], np.int64)
            out[k + "draw_tags"] = np.array(tags)
            out[k + "draw_values"] = np.concatenate([v for _, v in s["draws"]])
            out[k + "draw_sizes"] = np.array([len(v) for _, v in s["draws"]], np.int64)
            out[k + "choice"] = s["draws"][tags.rindex("s")][1].astype(np.int64)
            assert len(out[k + "choice"]) == P == len(items[b]["points"])
            if mode == "train":
                out[k + "perm"] = s["draws"][-1][1].astype(np.int64)
                assert tags.endswith("sp") and len(out[k + "perm"]) == P
            else:
                assert tags.endswith("s") and set(tags) <= set("cs")
            out[k + "rng_keys"], out[k + "rng_pos"], out[k + "rng_gauss"] = s["state"]
            out[k + "cand_uid"] = np.array([u for g in s["groups"] for u in g], np.int64)
            out[k + "n"], out[k + "c"] = (np.array(v, np.int64) for v in counts(s))
            out[k + "num_boxes"] = np.array(len(items[b]["gt_boxes"]), np.int64)
            if mode == "train":
                out[k + "boxes_before_trim"] = np.array(len(s["trim_in"][-1]), np.int64)

    store("train", found, TRAIN, slots, items, batch)
    t_slots, t_items, t_batch = run(False, TEST, found + 1)
    ds = CannedDataset(frames, False, tmp)
    assert margins(t_slots, False)
    assert [counts(s) for s in t_slots] == [(a + b, a) for a, b, _ in COUNTS[2:]], [counts(s) for s in t_slots]
    store("test", found + 1, TEST, t_slots, t_items, t_batch)

    def raises(n_near, n_far):
        """The reference's own sample_points on a frame of that many near and far rows."""
        gen = np.random.RandomState(5)
        xyz = gen.normal(size=(n_near + n_far, 3))
        xyz *= (np.r_[np.full(n_near, 10.0), np.full(n_far, 50.0)] / np.linalg.norm(xyz, axis=1))[:, None]
        pts = np.concatenate([xyz, gen.uniform(0, 1, (len(xyz), 1))], axis=1).astype(np.float32)
        step = [f for f, c in zip(ds.data_processor.data_processor_queue, DATASET_CFG["DATA_PROCESSOR"]) if c["NAME"] == "sample_points"]
        try:
            got = step[0](data_dict={"points": pts})
            assert len(got["points"]) == P
            return False
        except ValueError:
            return True

    out["raises.more_far_than_p"] = np.array(raises(10, P + 1))
    out["raises.two_n_less_than_p"] = np.array(raises(P // 2 - 1, 0))
    out["raises.empty_frame"] = np.array(raises(0, 0))
    out["raises.control_far_equals_p"] = np.array(raises(10, P))
    out["raises.control_two_n_equals_p"] = np.array(raises(P // 2, 0))
    path = os.path.join(MG.OUT, "g23_sample_batch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; seed", found, "train n, c", [counts(s) for s in slots], "tags",
          [str(out[f"train.b{b}.draw_tags"]) for b in range(2)], "test n, c", [counts(s) for s in t_slots],
          "raises", {k: bool(v) for k, v in out.items() if k.startswith("raises.")})


if __name__ == "__main__":
    main()
