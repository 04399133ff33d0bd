"""Generate tests/golden/g22_train_batch.npz: a whole training batch and a whole test batch through the reference's own
data path, from the FOV filter to the collated arrays.

Runs only where the reference is (see make_golden.py, whose loader this script imports and does not edit, as
make_golden_augment.py does).  The reference code that runs: get_fov_flag (its source taken out of kitti_dataset.py, as
g11_preprocess does), Calibration, DataAugmentor.forward, DatasetTemplate.prepare_data (with its redraw recursion),
PointFeatureEncoder, DataProcessor.mask_points_and_boxes_outside_range and shuffle_points, DatasetTemplate.collate_batch.
They are driven by a stand-in subclass of DatasetTemplate whose __getitem__ serves canned frames and follows
KittiDataset.__getitem__ from the FOV filter on.  The two natives the sampler calls are absent upstream and are stood in for by
hvpr_amd.gt_sampling, as in G19: they stay UNPINNED.

The scene: a dataset of 4 frames, batch [0, 1, 2, 3], three classes.
  frame 0   ordinary: class and non-class ground truths, objects pasted
  frame 1   a hidden Van over everything (nothing is pasted) and one Car far outside the range: one box before the trim,
            none after it; the frame stays in the batch with zero boxes
  frame 2   every scene point lies behind the camera: empty after the FOV filter, its points are the pasted objects'
  frame 3   no ground truth at all, and the sampled objects of every group overlap one another: no box after the augmentor,
            the frame is redrawn (dataset.py:127-129).  It is the LAST of the batch, so the sampler's pointers advance in the same
            order in the reference (frame by frame) and in a loader that plans a batch before it redraws.
A quirk of the reference this scene depends on, kept as it is: the sampler pops `gt_boxes_mask` (database_sampler.py:189), so
when NOTHING is pasted the redraw test counts every ground truth, trained class or not (frame 1 is not redrawn: its hidden Van
counts); when something is pasted the count is class-trained ground truths plus pasted objects.

The seed is the first from SEED0 on for which the run shows all of the above AND keeps the margins, asserted in float64: G19's
(box pairs, scene points off the faces of candidate boxes, output corners off the range bounds, headings off pi), and no point
within 1e-3 m of an x/y range bound after the augmentor, no projected pixel within 1e-3 px of the image border, no rect depth
within 1e-3 of 0.

Stored: the frames and the database; for each batch slot every draw in order (tags p permutation, c choice, u uniform,
r randint), the __getitem__ indices served, the final permutation, the numpy RNG state after the slot; the collated points
and gt_boxes of the train and the test batch.
"""
import ast
import json
import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402
import make_golden_augment as MGA  # noqa: E402
import augment_cases as AC  # noqa: E402
from hvpr_amd.augment import put_boxes_on_road_planes  # noqa: E402

CLASS_NAMES = MGA.CLASS_NAMES
RANGE = MGA.RANGE
CALIB, PLANE = MGA.CALIB, MGA.PLANE
CAR, PED, CYC = MGA.CAR, MGA.PED, MGA.CYC
SEED0 = 2200
N_SCENE = 1500

# name, x, y, z, size, heading, points, difficulty: per class one overlapping pair and two free objects
DB = [
    ("Car", 10.0, 5.0, -0.9, CAR, 0.3, 30, 0), ("Car", 11.5, 5.6, -0.8, CAR, -0.2, 25, 1),
    ("Car", 20.0, -10.0, -1.0, CAR, 1.2, 40, 0), ("Car", 30.0, 12.0, -0.7, CAR, -2.9, 12, 2),
    ("Car", 60.0, 30.0, -1.0, CAR, 0.0, 9, -1),                                                  # removed by filter_by_difficulty
    ("Pedestrian", 40.0, -5.0, -0.6, PED, 0.7, 14, 0), ("Pedestrian", 40.3, -4.8, -0.6, PED, -1.0, 9, 0),
    ("Pedestrian", 50.0, 0.0, -0.5, PED, 2.0, 20, 1), ("Pedestrian", 45.0, -20.0, -0.5, PED, 0.4, 11, 0),
    ("Pedestrian", 55.0, 15.0, -0.5, PED, 0.0, 3, 0),                                            # removed by filter_by_min_points
    ("Cyclist", 25.0, 22.0, -0.6, CYC, 0.4, 16, 0), ("Cyclist", 25.6, 22.3, -0.6, CYC, 1.9, 8, 0),
    ("Cyclist", 35.0, -30.0, -0.8, CYC, -0.6, 11, 0), ("Cyclist", 16.0, -18.0, -0.7, CYC, 0.9, 13, 0),
]
PREPARE = MGA.PREPARE
AUG_CFG = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [
    {"NAME": "gt_sampling", "USE_ROAD_PLANE": True, "DB_INFO_PATH": ["dbinfos.pkl"], "PREPARE": PREPARE,
     "SAMPLE_GROUPS": ["Car:2", "Pedestrian:2", "Cyclist:2"], "NUM_POINT_FEATURES": 4, "DATABASE_WITH_FAKELIDAR": False,
     "REMOVE_EXTRA_WIDTH": [0.2, 0.1, 0.3], "LIMIT_WHOLE_SCENE": False},
    {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
    {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
    {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]}
DATASET_CFG = {
    "DATASET": "KittiDataset", "DATA_PATH": ".", "POINT_CLOUD_RANGE": [float(v) for v in RANGE], "FOV_POINTS_ONLY": True,
    "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity"],
                               "src_feature_list": ["x", "y", "z", "intensity"]},
    "DATA_AUGMENTOR": AUG_CFG,
    "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                       {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}}]}
VAN = [90.0, 90.0, 3.0]
FRAMES = [
    {"gts": [MGA.gt("Car", 15.0, -25.0, -1.0, CAR, 0.5), MGA.gt("Van", 55.0, 25.0, -0.6, [5.0, 2.0, 2.0], 0.1),
             MGA.gt("Pedestrian", 30.0, -15.0, -0.7, PED, 0.2), MGA.gt("Car", 74.0, 10.0, -1.0, CAR, 0.2)], "behind": False,
     "image_shape": [375, 1242]},
    {"gts": [MGA.gt("Van", 35.0, 0.0, -1.0, VAN, 0.2), MGA.gt("Car", 100.0, 0.0, -1.0, CAR, 0.2)], "behind": False,
     "image_shape": [370, 1224]},
    {"gts": [MGA.gt("Car", 15.0, -25.0, -1.0, CAR, 0.5), MGA.gt("Cyclist", 50.0, 20.0, -0.6, CYC, 1.0)], "behind": True,
     "image_shape": [375, 1242]},
    {"gts": [], "behind": False, "image_shape": [376, 1241]},
]


def get_fov_flag_of_reference():
    tree = ast.parse(open(os.path.join(MG.REF, "pcdet/datasets/kitti/kitti_dataset.py")).read())
    fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "get_fov_flag"][0]
    fn.decorator_list = []
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "kitti_dataset.py", "exec"), ns)
    return ns["get_fov_flag"]


def project64(xyz):
    """(u, v, rect depth, image depth) in float64."""
    a = np.dot(CALIB["Tr_velo2cam"].astype(np.float64).T, CALIB["R0"].astype(np.float64).T)
    rect = np.hstack([xyz.astype(np.float64), np.ones((len(xyz), 1))]) @ a
    img = np.hstack([rect, np.ones((len(xyz), 1))]) @ CALIB["P2"].astype(np.float64).T
    return img[:, 0] / rect[:, 2], img[:, 1] / rect[:, 2], rect[:, 2], img[:, 2] - CALIB["P2"].astype(np.float64).T[3, 2]


def build_database(tmp, gen):
    infos, arena, off = {}, [], [0]
    for uid, (name, x, y, z, size, h, n, diff) in enumerate(DB):
        half = np.array(size, np.float32) / 2 * 0.9
        pts = np.concatenate([gen.uniform(-half, half, (n, 3)), gen.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
        pts.tofile(str(tmp / f"obj_{uid}.bin"))
        infos.setdefault(name, []).append({"name": name, "path": f"obj_{uid}.bin", "uid": uid, "difficulty": diff,
                                           "box3d_lidar": np.array([x, y, z, *size, h], np.float32), "num_points_in_gt": n})
        arena.append(pts)
        off.append(off[-1] + n)
    with open(tmp / "dbinfos.pkl", "wb") as f:
        pickle.dump(infos, f)
    boxes = np.stack([np.array([d[1], d[2], d[3], *d[4], d[5]], np.float32) for d in DB])
    return {"db.names": np.array([d[0] for d in DB]), "db.boxes": boxes, "db.points": np.concatenate(arena),
            "db.point_off": np.array(off, np.int64), "db.num_points_in_gt": np.array([d[6] for d in DB], np.int64),
            "db.difficulty": np.array([d[7] for d in DB], np.int64)}


def build_frames(gen, db_boxes):
    ex = np.array(AUG_CFG["AUG_CONFIG_LIST"][0]["REMOVE_EXTRA_WIDTH"], np.float64)
    cands = np.concatenate([db_boxes.astype(np.float64), put_boxes_on_road_planes(db_boxes.copy(), PLANE, CALIB)[0].astype(np.float64)])
    frames = []
    for fr in FRAMES:
        lo, hi = (np.array([-30.0, -45.0, -3.0]), np.array([-0.5, 45.0, 1.0])) if fr["behind"] else \
            (np.array([-10.0, -45.0, -3.0]), np.array([80.0, 45.0, 1.0]))
        pts = np.concatenate([gen.uniform(lo, hi, (N_SCENE, 3)), gen.uniform(0, 1, (N_SCENE, 1))], axis=1)
        if not fr["behind"]:
            near = [db_boxes[i, :3] + gen.uniform(-1.2, 1.2, (8, 3)) * [1.0, 1.0, 0.6] for i in range(len(DB))]
            pts = np.concatenate([pts, np.concatenate([np.concatenate(near), gen.uniform(0, 1, (8 * len(DB), 1))], axis=1)])
        pts = pts.astype(np.float32)
        ok = np.ones((len(pts),), bool)
        for b in cands:                                   # G19's margin: off the faces of every box a candidate could have
            e = b.copy()
            e[3:6] += ex
            ok &= AC.point_face_distance(pts, e)[0] >= 2e-3
        u, v, rz, depth = project64(pts[:, :3])           # the FOV margins
        h, w = fr["image_shape"]
        with np.errstate(invalid="ignore", divide="ignore"):
            ok &= (np.abs(rz) >= 1e-3) & (np.abs(depth) >= 1e-3)
            ok &= (np.abs(u) >= 1e-3) & (np.abs(u - w) >= 1e-3) & (np.abs(v) >= 1e-3) & (np.abs(v - h) >= 1e-3)
        names = np.array([g[0] for g in fr["gts"]], dtype="<U16")
        boxes = np.stack([g[1] for g in fr["gts"]]) if fr["gts"] else np.zeros((0, 7), np.float32)
        frames.append({"points": pts[ok], "gt_boxes": boxes, "gt_names": names, "image_shape": np.array(fr["image_shape"], np.int32),
                       "road_plane": PLANE.copy()})
    return frames


def main():
    R = MGA.load_augmentor(MG.load_reference())
    MG._load("pcdet.datasets.processor.point_feature_encoder", "pcdet/datasets/processor/point_feature_encoder.py")
    ds_mod = MG._load("pcdet.datasets.dataset", "pcdet/datasets/dataset.py")
    get_fov_flag = get_fov_flag_of_reference()
    log = {"draws": [], "items": [], "groups": [], "range_in": [], "trim_in": []}

    class CannedDataset(ds_mod.DatasetTemplate):
        """KittiDataset.__getitem__ from the FOV filter on (kitti_dataset.py:377-400), over frames held in memory."""

        def __init__(self, frames, training, root):
            super().__init__(dataset_cfg=MG.EasyDict(DATASET_CFG), class_names=CLASS_NAMES, training=training, root_path=root)
            self.frames = frames

        def __len__(self):
            return len(self.frames)

        def __getitem__(self, index):
            log["items"].append(int(index))
            fr = self.frames[index]
            points, calib, img_shape = fr["points"].copy(), R.calibration.Calibration(dict(CALIB)), fr["image_shape"]
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

    tmp = Path(tempfile.mkdtemp(prefix="g22_db_"))
    db = build_database(tmp, np.random.RandomState(22))
    db_boxes = db["db.boxes"]
    frames = build_frames(np.random.RandomState(220), db_boxes)
    ex = np.array(AUG_CFG["AUG_CONFIG_LIST"][0]["REMOVE_EXTRA_WIDTH"], np.float64)
    real = (np.random.permutation, np.random.choice, np.random.uniform, np.random.randint)

    def run_train(seed):
        """One batch under `seed`; None unless the scene shows what it is there for and keeps its margins."""
        np.random.seed(seed)
        ds = CannedDataset(frames, True, tmp)
        sampler = ds.data_augmentor.data_augmentor_queue[0]
        real_sample = sampler.sample_with_fixed_number

        def sample(class_name, grp):
            r = real_sample(class_name, grp)
            log["groups"].append([i["uid"] for i in r])
            return r

        sampler.sample_with_fixed_number = sample
        np.random.permutation, np.random.choice, np.random.uniform, np.random.randint = (spy(f, t) for f, t in zip(real, "pcur"))
        try:
            slots, items = [], []
            for b in range(len(frames)):
                for k in log:
                    log[k] = []
                item = ds[b]
                st = np.random.get_state()
                slots.append({"items": list(log["items"]), "draws": list(log["draws"]), "groups": list(log["groups"]),
                              "range_in": list(log["range_in"]), "trim_in": list(log["trim_in"]),
                              "state": (st[1].copy(), np.array([st[2], st[3]], np.int64), np.array(st[4], np.float64))})
                items.append(item)
        finally:
            np.random.permutation, np.random.choice, np.random.uniform, np.random.randint = real
        # what the scene is there for
        if [len(s["items"]) for s in slots[:3]] != [1, 1, 1] or len(slots[3]["items"]) < 2:
            return None
        if len(items[0]["gt_boxes"]) == 0 or len(items[1]["gt_boxes"]) != 0 or len(slots[1]["trim_in"][-1]) != 1:
            return None
        if len(items[2]["gt_boxes"]) == 0 or len(items[2]["points"]) == 0 or len(items[3]["gt_boxes"]) == 0:
            return None
        # the margins
        r64 = RANGE.astype(np.float64)
        for s in slots:
            # a redrawn frame returns before the range mask and the trim: only the last frame served reaches them
            assert len(s["range_in"]) == 1 and len(s["trim_in"]) == 1 and len(s["groups"]) == 3 * len(s["items"])
            xy = s["range_in"][0][:, :2].astype(np.float64)
            if len(xy) and min(np.abs(xy - r64[0:2]).min(), np.abs(xy - r64[3:5]).min()) < 1e-3:
                return None
            for i, served in enumerate(s["items"]):
                uid = [u for g in s["groups"][3 * i: 3 * i + 3] for u in g]
                cb = put_boxes_on_road_planes(db_boxes[uid].copy(), PLANE, CALIB)[0] if uid else np.zeros((0, 7), np.float32)
                fr, C = frames[served], R.calibration.Calibration(dict(CALIB))
                fov = get_fov_flag(C.lidar_to_rect(fr["points"][:, 0:3]), fr["image_shape"], C)
                before = s["trim_in"][0] if i == len(s["items"]) - 1 else np.zeros((0, 8), np.float32)
                okm, why = AC.margins_ok(fr["points"][fov], fr["gt_boxes"], {"cand_box": cb}, ex, before, RANGE)
                if not okm:
                    return None
        batch = ds.collate_batch([{"points": i["points"], "gt_boxes": i["gt_boxes"]} for i in items])
        return slots, items, batch

    found = None
    for seed in range(SEED0, SEED0 + 20000):
        found = run_train(seed)
        if found is not None:
            break
    assert found is not None, "no seed shows the scene"
    slots, items, batch = found
    out = {"class_names": np.array(CLASS_NAMES), "range": RANGE, "prepare": np.array(json.dumps(PREPARE)),
           "config": np.array(json.dumps(DATASET_CFG)), "plane": PLANE, "num_frames": np.array(len(frames), np.int64)}
    out.update(db)
    for k, v in CALIB.items():
        out["calib." + k] = v
    for i, fr in enumerate(frames):
        for k in ("points", "gt_boxes", "gt_names", "image_shape", "road_plane"):
            out[f"fr{i}.{k}"] = fr[k]
    out["train.seed"] = np.array(seed, np.int64)
    out["train.indices"] = np.arange(len(frames), dtype=np.int64)
    out["train.points"], out["train.gt_boxes"] = batch["points"], batch["gt_boxes"]
    assert batch["points"].dtype == np.float32 and batch["gt_boxes"].dtype == np.float32
    for b, s in enumerate(slots):
        k = f"train.b{b}."
        out[k + "items"] = np.array(s["items"], np.int64)
        out[k + "draw_tags"] = np.array("".join(t for t, _ in s["draws"]))
        out[k + "draw_values"] = np.concatenate([v for _, v in s["draws"]])
        out[k + "draw_sizes"] = np.array([len(v) for _, v in s["draws"]], np.int64)
        out[k + "perm"] = s["draws"][-1][1].astype(np.int64)
        assert s["draws"][-1][0] == "p" and len(out[k + "perm"]) == len(items[b]["points"])
        out[k + "rng_keys"], out[k + "rng_pos"], out[k + "rng_gauss"] = s["state"]
        out[k + "cand_uid"] = np.array([u for g in s["groups"] for u in g], np.int64)
        out[k + "boxes_before_trim"] = np.array(len(s["trim_in"][-1]), np.int64)
        out[k + "num_points"] = np.array(len(items[b]["points"]), np.int64)
        out[k + "num_boxes"] = np.array(len(items[b]["gt_boxes"]), np.int64)
    # the test batch: no augmentor, no trim, no shuffle
    np.random.seed(seed + 1)
    ds = CannedDataset(frames, False, tmp)
    for k in log:
        log[k] = []
    t_items = [ds[b] for b in range(len(frames))]
    st = np.random.get_state()
    np.random.seed(seed + 1)
    assert np.array_equal(st[1], np.random.get_state()[1]) and st[2] == np.random.get_state()[2], "the test path drew a number"
    r64 = RANGE.astype(np.float64)
    for pts in log["range_in"]:
        xy = pts[:, :2].astype(np.float64)
        assert not len(xy) or min(np.abs(xy - r64[0:2]).min(), np.abs(xy - r64[3:5]).min()) >= 1e-3
    t_batch = ds.collate_batch([{"points": i["points"], "gt_boxes": i["gt_boxes"]} for i in t_items])
    out["test.points"], out["test.gt_boxes"] = t_batch["points"], t_batch["gt_boxes"]
    out["test.num_points"] = np.array([len(i["points"]) for i in t_items], np.int64)
    assert out["test.num_points"][2] == 0 and out["test.num_points"].sum() > 0
    path = os.path.join(MG.OUT, "g22_train_batch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; seed", seed, "items", [s["items"] for s in slots],
          "points", [len(i["points"]) for i in items], "boxes", [len(i["gt_boxes"]) for i in items],
          "test points", out["test.num_points"].tolist())


if __name__ == "__main__":
    main()
