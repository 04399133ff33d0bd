"""The batch loader's path with `sample_points` in it, in numpy: batch_loader_cases.py (FOV filter, augmentor, redraw, class
filter, trim, range mask) with DataProcessor.sample_points restated in this project's words
(pcdet/datasets/processor/data_processor.py:77-108) between the range mask and the shuffle.  test_sample_batch_host.py pins it
to fixture G23 (the reference's own code, tests/golden/make_golden_sample_batch.py) on the CPU; the GPU tests compare the device
against the same fixture and use `sample_points_host` as their checker.

The near flag is the reference's expression (`np.linalg.norm(points[:, 0:3], axis=1) < 40.0`, float32); the kernels square and
add left to right and take the hardware's root, good to one unit in the last place.  G23 keeps every row that reaches the step
at least 1e-3 m off norm 40, over a hundred times more than either rounding (a few units of 2^-24 * 40 = 2.4e-6), so both
decide alike."""
import json
import os

import numpy as np

import batch_loader_cases as BC

NEAR = 40.0


# ------------------------------------------------------------------------------------------------ fixture access
def g23():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_sample_batch.npz"), allow_pickle=False)


def g23_config(z):
    return json.loads(str(z["config"]))


def g23_generators(z, mode):
    """One generator per batch slot, each in the state the reference's `np.random` had when it reached that frame."""
    gens = [np.random.RandomState(int(z[mode + ".seed"]))]
    for b in range(1, len(z[mode + ".indices"])):
        k = f"{mode}.b{b - 1}."
        g = np.random.RandomState(0)
        g.set_state(("MT19937", z[k + "rng_keys"], int(z[k + "rng_pos"][0]), int(z[k + "rng_pos"][1]), float(z[k + "rng_gauss"])))
        gens.append(g)
    return gens


def state_matches(gen, z, mode, b):
    st, k = gen.get_state(), f"{mode}.b{b}."
    return bool(np.array_equal(st[1], z[k + "rng_keys"]) and [st[2], st[3]] == z[k + "rng_pos"].tolist() and
                st[4] == float(z[k + "rng_gauss"]))


# ------------------------------------------------------------------------------------------------ the step
def near_flag(points):
    return np.linalg.norm(np.asarray(points, np.float32)[:, 0:3], axis=1) < NEAR


def sample_points_host(points, num_points, rng):
    """What DataProcessor.sample_points does to one frame, restated from its three cases.  Returns (points[choice], choice).

    * more rows than wanted: every far row is kept and the room left is filled by a draw, without replacement, over the near
      rows (near ones in front, far ones behind them); the reference makes that draw once more in front of the test whether
      there is any room, and throws the first away.  With no room left it draws over all rows instead.
    * fewer rows than wanted: every row once, then a draw without replacement over the rows for what is missing.
    * -1: nothing happens.
    In the first two cases the list is shuffled in place at the end."""
    total = len(points)
    if num_points == -1:
        return points, np.arange(total)
    every = np.arange(total, dtype=np.int32)
    if total > num_points:
        flags = near_flag(points)
        close, distant = np.flatnonzero(flags), np.flatnonzero(~flags)
        room = num_points - len(distant)
        rng.choice(close, room, replace=False)                   # thrown away; raises when the far rows alone are too many
        if room > 0:
            choice = np.concatenate([rng.choice(close, room, replace=False), distant])
        else:
            choice = rng.choice(every, num_points, replace=False)
    else:
        missing = num_points - total
        choice = np.concatenate([every, rng.choice(every, missing, replace=False)]) if missing else every
    rng.shuffle(choice)
    return points[choice], choice


# ------------------------------------------------------------------------------------------------ the path
def _finish(slots, gens, rng6, num_points, shuffle):
    parts = []
    for b, s in enumerate(slots):
        pts = s["kept"]
        s["n"], s["c"] = len(pts), int(near_flag(pts).sum()) if len(pts) else 0
        pts, s["choice"] = sample_points_host(pts, num_points, gens[b])
        s["perm"] = gens[b].permutation(len(pts)) if shuffle else np.arange(len(pts))
        s["points"] = pts[s["perm"]]
        parts.append(np.concatenate([np.full((len(pts), 1), b, np.float32), s["points"]], axis=1))
    return np.concatenate(parts, axis=0)


def prepare_batch_host(frames, indices, planner, bank, gens, rng6, num_frames, num_points, shuffle=True):
    """Training, in the loader's phases: the augmentor draws of every frame, each empty frame's redraw chain, then per frame
    the sample draws followed by the permutation.  Returns the collated points (B * P, 1 + F), gt_boxes and the slots."""
    slots = [{"items": [int(i)], "r": BC._augment(frames[i], planner, bank, gens[b], rng6, True, True)} for b, i in enumerate(indices)]
    for b, s in enumerate(slots):
        while s["r"]["after_augmentor"] == 0:
            new_index = int(gens[b].randint(num_frames))
            s["items"].append(new_index)
            s["r"] = BC._augment(frames[new_index], planner, bank, gens[b], rng6, True, True)
    for s in slots:
        s["kept"] = s["r"]["points"][BC.range_flag(s["r"]["points"], rng6)]
    points = _finish(slots, gens, rng6, num_points, shuffle)
    gt = np.zeros((len(indices), max(len(s["r"]["boxes"]) for s in slots), 8), np.float32)
    for b, s in enumerate(slots):
        gt[b, : len(s["r"]["boxes"])] = s["r"]["boxes"]
    return points, gt, slots


def test_batch_host(frames, indices, class_names, gens, rng6, num_points, shuffle=False):
    """Test mode: FOV filter, range mask, sample_points (the reference seeds numpy there too), no shuffle by default."""
    slots = []
    for i in indices:
        pts = np.asarray(frames[i]["points"], np.float32)
        keep = BC.fov_flag(pts, frames[i]["calib"], frames[i]["image_shape"]) & BC.range_flag(pts, rng6)
        slots.append({"items": [int(i)], "kept": pts[keep]})
    points = _finish(slots, gens, rng6, num_points, shuffle)
    _, gt = BC.test_batch_host(frames, indices, class_names, rng6)
    return points, gt, slots


test_batch_host.__test__ = False
