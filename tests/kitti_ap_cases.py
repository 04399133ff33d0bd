"""Inputs and host-side bookkeeping shared by tests/test_kitti_ap_host.py and tests/test_gpu_kitti_ap.py.

edge_set(): 8 hand-made frames at the edges of the matching rules.  HostRun: ONE run of the host evaluator (kitti_eval.eval_class)
that also keeps what its inner calls returned — the true-positive scores of the threshold pass, n_valid, the thresholds and the
integer tp / fp / fn of every (combo, threshold) — so the device is compared with what the host computed, not with a restatement.
"""
import numpy as np

from hvpr_amd import kitti_eval

_KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y")
DIMS = {"Car": (3.9, 1.56, 1.6), "Van": (5.0, 2.2, 1.9), "Pedestrian": (0.8, 1.73, 0.6), "Person_sitting": (0.8, 1.3, 0.6),
        "Cyclist": (1.76, 1.73, 0.6), "DontCare": (-1.0, -1.0, -1.0)}


def bbox_of(loc, dims):
    u, v = 620 + 720 * loc[0] / loc[2], 180 + 720 * (loc[1] - dims[1] / 2) / loc[2]
    hw, hh = 360 * max(dims[0], dims[2]) / loc[2], 360 * dims[1] / loc[2]
    return [u - hw, v - hh, u + hw, v + hh]


class _Frame:
    def __init__(self):
        self.g = {k: [] for k in _KEYS}
        self.d = {k: [] for k in _KEYS + ("score",)}

    @staticmethod
    def _add(to, name, loc, ry, bbox, trunc, occ, dims, score=None):
        dims = np.array(DIMS[name] if dims is None else dims, np.float64)
        loc = np.array(loc, np.float64)
        to["name"].append(name); to["truncated"].append(trunc); to["occluded"].append(occ)
        to["alpha"].append(ry - np.arctan2(loc[0], loc[2])); to["bbox"].append(bbox_of(loc, np.abs(dims)) if bbox is None else list(bbox))
        to["dimensions"].append(dims); to["location"].append(loc); to["rotation_y"].append(ry)
        if score is not None:
            to["score"].append(score)

    def gt(self, name, loc=(0.0, 1.6, 20.0), ry=0.3, bbox=None, trunc=0.0, occ=0, dims=None):
        self._add(self.g, name, loc, ry, bbox, trunc, occ, dims)

    def dt(self, name, score, loc=(0.0, 1.6, 20.0), ry=0.3, bbox=None, dims=None):
        self._add(self.d, name, loc, ry, bbox, 0.0, 0, dims, score)

    def pack(self):
        def one(a, with_score):
            out = {"name": np.array(a["name"], dtype="<U16"), "truncated": np.array(a["truncated"], np.float64),
                   "occluded": np.array(a["occluded"], np.int64), "alpha": np.array(a["alpha"], np.float64),
                   "bbox": np.array(a["bbox"], np.float64).reshape(-1, 4), "dimensions": np.array(a["dimensions"], np.float64).reshape(-1, 3),
                   "location": np.array(a["location"], np.float64).reshape(-1, 3), "rotation_y": np.array(a["rotation_y"], np.float64)}
            if with_score:
                out["score"] = np.array(a["score"], np.float64)
            return out
        return one(self.g, False), one(self.d, True)


def edge_set():
    """-> (gt_annos, dt_annos), 8 frames:
    0  130 detections on 3 cars: the wave walks three chunks of 64, and the best candidate of each car (an exact copy, the largest
       overlap; the highest score elsewhere) lies in another chunk;
    1  duplicated detections: equal overlap and equal score (the lowest index must win), on a car and on a pedestrian;
    2  detections with a 2-D height of exactly 40 and of 39.99 (ignored at `easy`): an ignored detection FIRST with the larger
       overlap, an evaluated one after it; a car whose only detection is an ignored one; truncation exactly 0.15 / 0.3 / 0.5;
    3  two DontCare boxes over the same unmatched detection, one detection outside both;
    4  only DontCare ground truth;
    5  cyclist detections — a class no ground truth of the set has;
    6  an empty frame;
    7  ground truth (pedestrian, person_sitting, van) without detections."""
    rng = np.random.default_rng(20)
    frames = [_Frame() for _ in range(8)]
    f = frames[0]
    cars = [((-6.0, 1.6, 12.0), 0.2), ((1.0, 1.7, 15.0), -1.1), ((7.0, 1.5, 18.0), 2.0)]
    for loc, ry in cars:
        f.gt("Car", loc, ry)
    exact = {3: 0, 67: 1, 128: 2}
    for j in range(130):
        i = exact.get(j, j % 3)
        loc, ry = cars[i]
        if j in exact:
            f.dt("Car", 0.5, loc, ry)
        else:
            jit = rng.normal(0, 1, 3) * np.array([0.08, 0.02, 0.1]) * rng.choice([1, 1, 3])
            dl = np.array(loc) + jit
            f.dt("Car", float(np.round(rng.uniform(0.1, 1.0), 2)), dl, ry + rng.normal(0, 0.03),
                 bbox=(np.array(bbox_of(loc, DIMS["Car"])) + rng.normal(0, 3, 4)).tolist())
    f = frames[1]
    f.gt("Car", (2.0, 1.6, 14.0), 0.4)
    f.gt("Pedestrian", (-3.0, 1.7, 9.0), 1.0)
    for _ in range(2):
        f.dt("Car", 0.8, (2.05, 1.6, 14.05), 0.41)
    f.dt("Car", 0.8, (2.0, 1.6, 14.0), 0.4)                  # same score, larger overlap, later
    for _ in range(2):
        f.dt("Pedestrian", 0.6, (-3.02, 1.7, 9.01), 1.0)
    f = frames[2]
    f.gt("Car", (0.0, 1.6, 20.0), 0.0, bbox=(100.0, 100.0, 200.0, 142.0))
    f.dt("Car", 0.9, (0.0, 1.6, 20.0), 0.0, bbox=(100.0, 100.0, 200.0, 139.99))          # ignored at easy, the larger overlap
    f.dt("Car", 0.7, (0.1, 1.6, 20.1), 0.0, bbox=(100.0, 100.0, 190.0, 140.0))           # height exactly 40: evaluated
    f.gt("Car", (8.0, 1.6, 25.0), 0.5, bbox=(400.0, 100.0, 500.0, 141.0))
    f.dt("Car", 0.6, (8.0, 1.6, 25.0), 0.5, bbox=(400.0, 100.0, 500.0, 139.99))          # its only detection is an ignored one
    for x, trunc in ((-9.0, 0.15), (-5.0, 0.3), (4.0, 0.5)):
        f.gt("Car", (x, 1.6, 11.0), 0.1, trunc=trunc)
        f.dt("Car", 0.55 + trunc, (x + 0.03, 1.6, 11.02), 0.1)
    f = frames[3]
    f.gt("DontCare", bbox=(300.0, 100.0, 700.0, 300.0))
    f.gt("DontCare", bbox=(350.0, 120.0, 800.0, 320.0))
    f.gt("Car", (-8.0, 1.6, 16.0), 0.7)
    f.dt("Car", 0.75, (-8.0, 1.6, 16.0), 0.7)
    f.dt("Car", 0.65, (0.0, 1.6, 30.0), 0.0, bbox=(400.0, 150.0, 600.0, 250.0))          # inside both DontCare boxes
    f.dt("Car", 0.45, (10.0, 1.6, 30.0), 0.0, bbox=(900.0, 150.0, 1100.0, 250.0))        # outside: a false positive
    f = frames[4]
    f.gt("DontCare", bbox=(0.0, 100.0, 500.0, 300.0))
    f.dt("Pedestrian", 0.5, (-4.0, 1.7, 12.0), 0.0, bbox=(100.0, 120.0, 160.0, 280.0))
    f.dt("Car", 0.35, (5.0, 1.6, 22.0), 0.0, bbox=(700.0, 150.0, 900.0, 250.0))
    f = frames[5]
    f.gt("Car", (3.0, 1.6, 13.0), -0.4, occ=1)
    f.dt("Cyclist", 0.9, (3.0, 1.6, 13.0), -0.4, dims=DIMS["Cyclist"])
    f.dt("Cyclist", 0.4, (-6.0, 1.7, 19.0), 0.9)
    f = frames[7]
    f.gt("Pedestrian", (1.0, 1.7, 8.0), 0.0)
    f.gt("Person_sitting", (2.5, 1.7, 8.5), 0.0)
    f.gt("Van", (-7.0, 1.8, 17.0), 1.2, occ=2)
    gts, dts = zip(*(fr.pack() for fr in frames))
    return list(gts), list(dts)


def with_empty_ends(gts, dts):
    """The same frames between two empty ones."""
    g0, d0 = _Frame().pack()
    return [g0] + list(gts) + [g0], [d0] + list(dts) + [d0]


class HostRun:
    """kitti_eval.eval_class(gts, dts, classes, metric, min_overlaps, compute_aos, rotated_intersection), recorded.

    result: what eval_class returned; tp_scores[combo]: sorted scores of the threshold pass's true positives; n_valid [C, 3];
    thresholds[combo]: the array get_thresholds returned; counts[combo]: int [n_thresholds, 3] sums of _frame_stats' tp, fp, fn;
    sim[combo]: [n_thresholds] the similarity sums.  combo = (m * 3 + l) * K + k, the order eval_class walks."""

    def __init__(self, gts, dts, classes, metric, min_overlaps, compute_aos, rotated_intersection=None):
        events = []
        real = kitti_eval._match, kitti_eval._frame_stats, kitti_eval.get_thresholds

        def match(overlap, gflag, dflag, dscore, min_overlap, thresh, with_fp):
            out = real[0](overlap, gflag, dflag, dscore, min_overlap, thresh, with_fp)
            if not with_fp:
                events.append(("m", [float(dscore[j]) for _, j in out[2]]))
            return out

        def frame_stats(*a):
            out = real[1](*a)
            events.append(("s", out))
            return out

        def get_thresholds(scores, num_gt, *a, **k):
            out = real[2](scores, num_gt, *a, **k)
            events.append(("t", int(num_gt), out))
            return out

        kitti_eval._match, kitti_eval._frame_stats, kitti_eval.get_thresholds = match, frame_stats, get_thresholds
        try:
            kw = {} if rotated_intersection is None else {"rotated_intersection": rotated_intersection}
            self.result = kitti_eval.eval_class(gts, dts, classes, metric, min_overlaps, compute_aos, **kw)
        finally:
            kitti_eval._match, kitti_eval._frame_stats, kitti_eval.get_thresholds = real
        F, C, K = len(gts), len(classes), len(min_overlaps)
        self.tp_scores, self.thresholds, self.counts, self.sim = [], [], [], []
        self.n_valid = np.zeros((C, 3), np.int64)
        pos = 0
        for combo in range(C * 3 * K):
            scores = []
            for _ in range(F):
                assert events[pos][0] == "m"
                scores += events[pos][1]
                pos += 1
            _, num_gt, th = events[pos]
            pos += 1
            self.n_valid[combo // K // 3, combo // K % 3] = num_gt
            cnt, sim = np.zeros((len(th), 3), np.int64), np.zeros(len(th))
            for _ in range(F):
                for t in range(len(th)):
                    tp, fp, fn, s = events[pos][1]
                    pos += 1
                    cnt[t] += (tp, fp, fn)
                    if s != -1:
                        sim[t] += s
            self.tp_scores.append(np.sort(np.array(scores, np.float64)))
            self.thresholds.append(th); self.counts.append(cnt); self.sim.append(sim)
        assert pos == len(events)
