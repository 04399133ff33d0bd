"""Generate tests/golden/g19_augmentor.npz by running the reference's own DataAugmentor.forward and the box trim of
DataProcessor.mask_points_and_boxes_outside_range over a throw-away database (a pickle plus .bin files in a temp directory).

Runs only where the reference is (see make_golden.py, whose loader this script imports and does not edit).  What G19 pins is
the reference's PYTHON: sampling protocol, collision bookkeeping, paste order, flips, rotation, scaling, limit_period, trim.
The two natives it calls are absent upstream and are stood in for by hvpr_amd.gt_sampling (boxes_bev_iou_cpu,
points_in_boxes_cpu): they stay UNPINNED.  Zero / non-zero IoU and inside / outside are discontinuous, so the scenes keep a
margin (asserted below in float64): box pairs are >= 0.1 m apart or overlap by >= 0.01 m^2, no scene point is within 1e-3 m
of a face of an enlarged candidate box, no output corner within 1e-3 m of a range bound, no output heading within 1e-3 of pi.

Stored: inputs, the database arrays, every draw, the numpy RNG state after each frame, per group the candidate ids and the
valid mask, the output points, boxes and names.
"""
import json
import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402
import augment_cases as AC  # noqa: E402
from hvpr_amd import gt_sampling  # noqa: E402

CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]
RANGE = np.array([0, -40, -3, 70.4, 40, 1], np.float32)
CAR, PED, CYC = [3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]

# name, x, y, z, size, heading, points, difficulty
DB = [
    ("Car", 10.0, 5.0, -0.9, CAR, 0.3, 30, 0),        # 0  overlaps car 1 only: both always rejected
    ("Car", 11.5, 5.6, -0.8, CAR, -0.2, 25, 1),       # 1
    ("Car", 20.0, -10.0, -1.0, CAR, 1.2, 40, 0),      # 2  free: accepted unless a ground truth is in the way
    ("Car", 30.0, 10.0, -0.7, CAR, -2.9, 12, 2),      # 3  free
    ("Car", 40.0, -20.0, -1.1, CAR, 0.05, 0, 0),      # 4  an empty object
    ("Car", 60.0, 30.0, -1.0, CAR, 0.0, 9, -1),       # 5  removed by filter_by_difficulty
    ("Pedestrian", 9.0, 4.6, -0.6, PED, 0.7, 14, 0),  # 6  inside car 0 (a REJECTED candidate of an earlier group): accepted
    ("Pedestrian", 20.3, -9.8, -0.7, PED, -1.0, 9, 0),   # 7  inside car 2 (an ACCEPTED one): rejected with it
    ("Pedestrian", 50.0, 0.0, -0.5, PED, 2.0, 20, 1),    # 8  free
    ("Pedestrian", 55.0, 15.0, -0.5, PED, 0.0, 3, 0),    # 9  removed by filter_by_min_points
    ("Cyclist", 25.0, 20.0, -0.6, CYC, 0.4, 16, 0),      # 10 free
    ("Cyclist", 35.0, -30.0, -0.8, CYC, -0.6, 11, 0),    # 11 free
    ("Cyclist", 50.4, 0.3, -0.6, CYC, 1.9, 8, 0),        # 12 over pedestrian 8
    ("Cyclist", 45.0, 25.0, -0.6, CYC, 0.0, 30, -1),     # 13 removed by filter_by_difficulty
]

PREPARE = {"filter_by_min_points": ["Pedestrian:5", "Cyclist:5"], "filter_by_difficulty": [-1]}
RUNS = [
    {"seed": 1906, "cfg": {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": True, "DB_INFO_PATH": ["dbinfos.pkl"], "PREPARE": PREPARE,
         "SAMPLE_GROUPS": ["Car:15", "Pedestrian:10", "Van:3", "Cyclist:10"], "NUM_POINT_FEATURES": 4,
         "DATABASE_WITH_FAKELIDAR": False, "REMOVE_EXTRA_WIDTH": [0.2, 0.1, 0.3], "LIMIT_WHOLE_SCENE": False},
        {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]},
        {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
        {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]}},
    {"seed": 2024, "cfg": {"DISABLE_AUG_LIST": ["random_world_rotation"], "AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": ["dbinfos.pkl"], "PREPARE": PREPARE,
         "SAMPLE_GROUPS": ["Car:3", "Pedestrian:2", "Cyclist:2"], "NUM_POINT_FEATURES": 4,
         "DATABASE_WITH_FAKELIDAR": False, "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": True},
        {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": 0.1},
        {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [1.0, 1.0005]},
        {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]}]}},
]
CALIB = {
    "P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
    "R0": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
                    [0.007402527, 0.004351614, 0.9999631]], np.float32),
    "Tr_velo2cam": np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                             [0.9998621, 0.007523790, 0.01480755, -0.2717806]], np.float32),
}
PLANE = np.array([0.01, -0.999, 0.02, 1.68], np.float64)


def seed_of_run0(start=1906):
    """Flipping along y sends every box to x < 0, out of the range: the first seed from `start` on whose three frames draw
    flip_y = off, off, on and flip_x differently in the first two (a frame's draws: permutations of 5, 3, 3 objects, two flip
    choices, two uniforms)."""
    for seed in range(start, start + 1000):
        r, flips = np.random.RandomState(seed), []
        for _ in range(3):
            r.permutation(5), r.permutation(3), r.permutation(3)
            flips.append((bool(r.choice([False, True], replace=False, p=[0.5, 0.5])), bool(r.choice([False, True], replace=False, p=[0.5, 0.5]))))
            r.uniform(), r.uniform()
        if [f[1] for f in flips] == [False, False, True] and flips[0][0] != flips[1][0]:
            return seed
    raise RuntimeError("no seed")


def gt(name, x, y, z, size, h):
    return name, np.array([x, y, z, *size, h], np.float32)


def frames_of(run):
    """Ground truths per frame; scene points are drawn in main()."""
    if run == 0:
        return [
            {"gts": [], "plane": True},                                                       # no ground truth: iou1 := iou2
            {"gts": [gt("Car", 15.0, -25.0, -1.0, CAR, 0.5), gt("Van", 25.2, 20.1, -0.6, [5.0, 2.0, 2.0], 0.1),
                     gt("Van", 35.0, -30.2, -0.8, [5.0, 2.0, 2.0], 1.0), gt("Pedestrian", 20.5, -10.3, -0.7, PED, 0.2)],
             "plane": True},                                 # hidden Vans over cyclists 10 and 11: the Cyclist group accepts nothing
            {"gts": [gt("Van", 35.0, 0.0, -1.0, [90.0, 90.0, 3.0], 0.2), gt("Car", 5.0, 38.0, -1.0, CAR, 3.0)],
             "plane": False},                                # one hidden box over everything: nothing is pasted, no plane needed
        ]
    return [
        {"gts": [gt("Car", 15.0, -25.0, -1.0, CAR, 0.5), gt("Car", 74.0, 10.0, -1.0, CAR, 0.2)], "plane": False},   # one outside the range
        {"gts": [gt("Car", 50.0, 20.0, -1.0, CAR, -0.4), gt("Car", 60.0, -20.0, -1.0, CAR, 2.5), gt("Car", 5.0, -5.0, -1.0, CAR, 0.1),
                 gt("Pedestrian", 40.0, 5.0, -0.6, PED, 0.3), gt("Pedestrian", 42.0, 8.0, -0.6, PED, 0.3),
                 gt("Cyclist", 15.0, 30.0, -0.6, CYC, 1.0), gt("Cyclist", 18.0, 33.0, -0.6, CYC, 1.0)], "plane": False},   # nothing sampled
        {"gts": [gt("Pedestrian", 69.9, 39.5, -0.6, PED, 0.3), gt("Cyclist", 15.0, 30.0, -0.6, CYC, 1.0)], "plane": False},
        {"gts": [gt("Car", 68.0, -25.0, -1.0, CAR, 0.5), gt("Van", 30.1, 10.2, -0.7, [5.0, 2.0, 2.0], 0.3)], "plane": False},
    ]


def load_augmentor(R):
    for pkg, p in [("pcdet.datasets", "pcdet/datasets"), ("pcdet.datasets.augmentor", "pcdet/datasets/augmentor"),
                   ("pcdet.datasets.processor", "pcdet/datasets/processor")]:
        MG._stub(pkg, os.path.join(MG.REF, p))
    iou = sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"]
    roi = sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    iou.boxes_bev_iou_cpu = gt_sampling.boxes_bev_iou_cpu
    roi.points_in_boxes_cpu = lambda p, b: torch.from_numpy(gt_sampling.points_in_boxes_cpu(p, b))   # box_utils.py:86 sums a tensor
    R.box_utils.roiaware_pool3d_utils = roi
    R.augmentor_utils = MG._load("pcdet.datasets.augmentor.augmentor_utils", "pcdet/datasets/augmentor/augmentor_utils.py")
    R.database_sampler = MG._load("pcdet.datasets.augmentor.database_sampler", "pcdet/datasets/augmentor/database_sampler.py")
    R.data_augmentor = MG._load("pcdet.datasets.augmentor.data_augmentor", "pcdet/datasets/augmentor/data_augmentor.py")
    R.data_processor = MG._load("pcdet.datasets.processor.data_processor", "pcdet/datasets/processor/data_processor.py")
    R.calibration = MG._load("pcdet.utils.calibration_kitti", "pcdet/utils/calibration_kitti.py")
    return R


def main():
    R = load_augmentor(MG.load_reference())
    out = {"class_names": np.array(CLASS_NAMES), "range": RANGE, "prepare": np.array(json.dumps(PREPARE))}
    for k, v in CALIB.items():
        out["calib." + k] = v
    tmp = Path(tempfile.mkdtemp(prefix="g19_db_"))
    gen = np.random.RandomState(19)
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
    out.update({"db.names": np.array([d[0] for d in DB]), "db.boxes": np.stack([np.array([d[1], d[2], d[3], *d[4], d[5]], np.float32) for d in DB]),
                "db.points": np.concatenate(arena), "db.point_off": np.array(off, np.int64),
                "db.num_points_in_gt": np.array([d[6] for d in DB], np.int64), "db.difficulty": np.array([d[7] for d in DB], np.int64)})
    db_boxes = out["db.boxes"]

    fidx, seen = 0, {"flip_on": False, "flip_off": False, "wrap": False, "short": False}
    RUNS[0]["seed"] = seed_of_run0()
    for run, spec in enumerate(RUNS):
        cfg = MG.EasyDict(spec["cfg"])
        gcfg = spec["cfg"]["AUG_CONFIG_LIST"][0]
        np.random.seed(spec["seed"])
        aug = R.data_augmentor.DataAugmentor(tmp, cfg, CLASS_NAMES)
        sampler = aug.data_augmentor_queue[0]
        for c in CLASS_NAMES:
            out[f"run{run}.survivors.{c}"] = np.array([i["uid"] for i in sampler.db_infos[c]], np.int64)
        proc = R.data_processor.DataProcessor([MG.EasyDict(NAME="mask_points_and_boxes_outside_range", REMOVE_OUTSIDE_BOXES=True)],
                                              RANGE, training=True)
        log = {"draws": [], "groups": [], "valid": None}

        def spy(fn, tag):
            def w(*a, **k):
                r = fn(*a, **k)
                log["draws"].append((tag, np.atleast_1d(np.asarray(r, np.float64))))
                return r
            return w

        real = (np.random.permutation, np.random.choice, np.random.uniform)
        np.random.permutation, np.random.choice, np.random.uniform = (spy(f, t) for f, t in zip(real, "pcu"))
        real_sample, real_add = sampler.sample_with_fixed_number, sampler.add_sampled_boxes_to_scene

        def sample(class_name, grp):
            before, n = grp["pointer"], len(sampler.db_infos[class_name])
            r = real_sample(class_name, grp)
            seen["wrap"] |= before >= n and fidx_holder[0] > first_of_run
            seen["short"] |= len(r) < int(grp["sample_num"])
            log["groups"].append((class_name, [i["uid"] for i in r]))
            return r

        def add(data_dict, boxes, valid_dicts):
            log["valid"] = [i["uid"] for i in valid_dicts]
            return real_add(data_dict, boxes, valid_dicts)

        sampler.sample_with_fixed_number, sampler.add_sampled_boxes_to_scene = sample, add
        fidx_holder, first_of_run, frame_ids = [fidx], fidx, []
        for fr in frames_of(run):
            fidx_holder[0] = fidx
            names = np.array([g[0] for g in fr["gts"]], dtype="<U16")
            boxes = np.stack([g[1] for g in fr["gts"]]) if fr["gts"] else np.zeros((0, 7), np.float32)
            pts = np.concatenate([gen.uniform(RANGE[:3], RANGE[3:], (140, 3)), gen.uniform(0, 1, (140, 1))], axis=1)
            near = [db_boxes[i, :3] + gen.uniform(-1.2, 1.2, (8, 3)) * [1.0, 1.0, 0.6] for i in range(len(DB))]
            pts = np.concatenate([pts, np.concatenate([np.concatenate(near), gen.uniform(0, 1, (8 * len(DB), 1))], axis=1)]).astype(np.float32)
            # keep the scene off the faces of every box a candidate could have (with and without the road-plane move)
            ex = np.array(gcfg["REMOVE_EXTRA_WIDTH"], np.float64)
            cands = [db_boxes.astype(np.float64)]
            if fr["plane"]:
                from hvpr_amd.augment import put_boxes_on_road_planes
                cands.append(put_boxes_on_road_planes(db_boxes.copy(), PLANE, CALIB)[0].astype(np.float64))
            ok = np.ones((len(pts),), bool)
            for b in np.concatenate(cands):
                e = b.copy()
                e[3:6] += ex
                ok &= AC.point_face_distance(pts, e)[0] >= 2e-3
            pts = pts[ok]
            k = f"f{fidx}."
            out.update({k + "points": pts, k + "gt_boxes": boxes, k + "gt_names": names})
            d = {"points": pts.copy(), "gt_boxes": boxes.copy(), "gt_names": names.copy(),
                 "gt_boxes_mask": np.array([n in CLASS_NAMES for n in names], dtype=np.bool_)}
            if fr["plane"]:
                d["road_plane"], d["calib"] = PLANE.copy(), R.calibration.Calibration(dict(CALIB))
                out[k + "road_plane"] = PLANE
            log["draws"], log["groups"], log["valid"] = [], [], []
            d = aug.forward(d)                                                                 # the reference, as it is
            aug_points = d["points"].copy()
            sel = [i for i, n in enumerate(d["gt_names"]) if n in CLASS_NAMES]                 # dataset.py:131-137
            cls = np.array([CLASS_NAMES.index(n) + 1 for n in d["gt_names"][sel]], np.int32)
            d["gt_boxes"] = np.concatenate((d["gt_boxes"][sel], cls.reshape(-1, 1).astype(np.float32)), axis=1)
            before_trim = d["gt_boxes"].copy()
            d = proc.mask_points_and_boxes_outside_range(d, config=MG.EasyDict(REMOVE_OUTSIDE_BOXES=True))
            assert aug_points.dtype == np.float32 and d["gt_boxes"].dtype == np.float32
            flips = [bool(v[0]) for t, v in log["draws"] if t == "c"]
            seen["flip_on"] |= any(flips)
            seen["flip_off"] |= not all(flips)
            out[k + "draw_tags"] = np.array("".join(t for t, _ in log["draws"]))
            out[k + "draw_values"] = np.concatenate([v for _, v in log["draws"]]) if log["draws"] else np.zeros((0,))
            out[k + "draw_sizes"] = np.array([len(v) for _, v in log["draws"]], np.int64)
            st = np.random.get_state()
            out[k + "rng_keys"], out[k + "rng_pos"] = st[1].copy(), np.array([st[2], st[3]], np.int64)
            out[k + "rng_gauss"] = np.array(st[4], np.float64)
            out[k + "group_names"] = np.array([g[0] for g in log["groups"]], dtype="<U16")
            out[k + "group_sizes"] = np.array([len(g[1]) for g in log["groups"]], np.int64)
            cand = [u for g in log["groups"] for u in g[1]]
            out[k + "cand_uid"] = np.array(cand, np.int64)
            out[k + "valid"] = np.array([u in log["valid"] for u in cand], bool)
            out[k + "out_points"], out[k + "out_boxes"] = aug_points, d["gt_boxes"]
            out[k + "out_boxes_before_trim"] = before_trim
            out[k + "out_names"] = np.array([CLASS_NAMES[int(c) - 1] for c in d["gt_boxes"][:, 7]], dtype="<U16")
            # the margin condition, in float64
            cb = db_boxes[cand].copy() if cand else np.zeros((0, 7), np.float32)
            if fr["plane"] and len(cb):
                from hvpr_amd.augment import put_boxes_on_road_planes
                cb = put_boxes_on_road_planes(cb, PLANE, CALIB)[0]
            okm, why = AC.margins_ok(pts, boxes, {"cand_box": cb}, ex, before_trim, RANGE)
            assert okm, (fidx, why)
            frame_ids.append(fidx)
            fidx += 1
        out[f"run{run}.frames"] = np.array(frame_ids, np.int64)
        out[f"run{run}.seed"] = np.array(spec["seed"], np.int64)
        out[f"run{run}.config"] = np.array(json.dumps(spec["cfg"]))
        np.random.permutation, np.random.choice, np.random.uniform = real

    # the coverage the frames are there for
    assert all(seen.values()), seen
    v = {f: dict(zip(out[f"f{f}.cand_uid"].tolist(), out[f"f{f}.valid"].tolist())) for f in range(fidx)}
    assert not v[0][0] and not v[0][1] and v[0][2] and v[0][6] and not v[0][7] and v[0][8] and not v[0][12] and v[0][4], v[0]
    assert not v[1][10] and not v[1][11] and not v[1][12] and not v[1][2], v[1]       # the Cyclist group accepts nothing
    assert not any(v[2].values()) and len(v[2]) > 0 and len(out["f4.cand_uid"]) == 0
    assert any(0 < len(out[f"f{f}.out_boxes"]) < len(out[f"f{f}.out_boxes_before_trim"]) for f in range(fidx)), "no box is trimmed"
    assert all(len(out[f"f{f}.out_boxes"]) > 0 for f in range(fidx)), "a frame lost every box"
    path = os.path.join(MG.OUT, "g19_augmentor.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", fidx, "frames")


if __name__ == "__main__":
    main()
