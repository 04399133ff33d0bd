"""GPU: the device KITTI AP evaluator (hvpr_amd/kitti_eval_device.py, csrc/kitti_ap.hip, hvpr_boxes_pairwise_ragged_f32) against the
host evaluator hvpr_amd/kitti_eval.py run on the same annotations with the same HIP intersection kernel: overlaps bit-equal, the
true-positive scores, n_valid and every integer tp / fp / fn equal, precision and recall equal, orientation within 1e-9 (the bar
tests/test_kitti_eval.py sets for these curves: only cos and the order of a double sum differ)."""
import numpy as np
import pytest

from hvpr_amd import kitti_eval, kitti_eval_device as KD
from kitti_ap_cases import HostRun, edge_set, with_empty_ends
from make_golden import synthetic_kitti_annos

pytestmark = pytest.mark.gpu

CLASSES = [0, 1, 2]
MO = kitti_eval._OVERLAPS[:, :, CLASSES]
_SETS, _RUNS = {}, {}


def annos(name):
    if name not in _SETS:
        if name == "edge":
            gd = edge_set()
        elif name == "ends":
            gd = with_empty_ends(*synthetic_kitti_annos(7, 5))
        elif name == "noaos":
            gd = synthetic_kitti_annos(1212, 24)
            for d in gd[1]:
                d["alpha"] = np.full_like(d["alpha"], -10.0)
        else:
            gd = synthetic_kitti_annos(int(name[3:]), 24)
        _SETS[name] = (gd[0], gd[1], KD.AnnoTables(*gd))
    return _SETS[name]


def host_run(name, metric):
    """The host evaluator's run on a set, once per session (read-only afterwards)."""
    if (name, metric) not in _RUNS:
        g, d, _ = annos(name)
        _RUNS[name, metric] = HostRun(g, d, CLASSES, metric, MO, metric == 0)
    return _RUNS[name, metric]


def device_stats(name, metric):
    if ("dev", name, metric) not in _RUNS:
        _RUNS["dev", name, metric] = KD.match_statistics(annos(name)[2], CLASSES, metric, MO, metric == 0)
    return _RUNS["dev", name, metric]


@pytest.mark.parametrize("name", ["syn1212", "edge", "ends"])
def test_ragged_pairwise_is_the_per_frame_kernel_bit_for_bit(name):
    import torch
    from hvpr_amd import kernels
    _, _, t = annos(name)
    got = KD._read(KD.rotated_intersections(t))
    assert got.dtype == np.float32 and got.shape == (t.n_pairs,) and t.n_pairs > 0
    n_checked = 0
    for f in range(t.n_frames):
        a, b = t.dt_box7[t.dt_off[f]:t.dt_off[f + 1]], t.gt_box7[t.gt_off[f]:t.gt_off[f + 1]]
        if len(a) == 0 or len(b) == 0:
            assert t.pair_off[f] == t.pair_off[f + 1]
            continue
        want = kernels.boxes_pairwise(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 0).cpu().numpy()
        assert np.array_equal(got[t.pair_off[f]:t.pair_off[f + 1]].reshape(len(a), len(b)), want), f
        n_checked += (want > 0).sum()
    assert n_checked > 0
    if name == "ends":
        assert t.pair_off[0] == t.pair_off[1] and t.pair_off[-1] == t.pair_off[-2]


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", ["syn1212", "edge", "ends"])
def test_overlaps_are_the_hosts_bit_for_bit(name, metric):
    g, d, t = annos(name)
    got = KD._read(KD.overlaps(t, metric))
    assert got.dtype == np.float64 and got.shape == (t.n_pairs,)
    n_pos = 0
    for f in range(t.n_frames):
        want = kitti_eval.frame_overlap(g[f], d[f], metric, kitti_eval.hip_rotated_intersection)
        assert np.array_equal(got[t.pair_off[f]:t.pair_off[f + 1]].reshape(want.shape), want), (f, metric)
        n_pos += (want > 0).sum()
    assert n_pos > 0


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", ["syn1212", "edge"])
def test_threshold_pass(name, metric):
    host, dev = host_run(name, metric), device_stats(name, metric)
    assert np.array_equal(dev["n_valid"], host.n_valid)
    for combo in range(18):
        s = dev["tp_score"][combo]
        assert np.array_equal(np.sort(s[~np.isnan(s)]), host.tp_scores[combo]), combo
        n = len(host.thresholds[combo])
        assert dev["thresh_count"][combo] == n and np.array_equal(dev["thresholds"][combo, :n], host.thresholds[combo])
    assert sum(len(s) for s in host.tp_scores) > 0


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", ["syn1212", "edge"])
def test_counting_pass_integers_equal_the_hosts(name, metric, observed):
    host, dev = host_run(name, metric), device_stats(name, metric)
    total = np.zeros(3, np.int64)
    for combo in range(18):
        n = len(host.thresholds[combo])
        assert np.array_equal(dev["counts"][combo, :n], host.counts[combo]), (combo, dev["counts"][combo, :n], host.counts[combo])
        assert (dev["counts"][combo, n:] == 0).all() and (dev["sim"][combo, n:] == 0).all()
        total += host.counts[combo].sum(axis=0)
        if metric == 0:
            np.testing.assert_allclose(dev["sim"][combo, :n], host.sim[combo], rtol=0, atol=1e-9)
    assert (total > 0).all()                                       # true positives, false positives and misses all occur
    observed(f"kitti AP {name} metric {metric}: tp/fp/fn sums {total.tolist()} equal the host's")


@pytest.mark.parametrize("name", ["syn1212", "syn7"])
def test_curves_equal_the_hosts(name):
    _, _, t = annos(name)
    for metric in (0, 1, 2):
        host = host_run(name, metric).result
        dev = KD.eval_class(t, CLASSES, metric, MO, metric == 0)
        assert np.array_equal(dev["precision"], host["precision"]) and np.array_equal(dev["recall"], host["recall"]), metric
        np.testing.assert_allclose(dev["orientation"], host["orientation"], rtol=0, atol=1e-9)
        assert host["precision"].max() > 0 and (metric != 0 or host["orientation"].max() > 0)


@pytest.mark.parametrize("classes", [["Car", "Pedestrian", "Cyclist"], ["Car"]])
@pytest.mark.parametrize("name", ["syn1212", "syn7", "noaos"])
def test_official_result_equals_the_hosts(name, classes):
    g, d, _ = annos(name)
    text_h, ret_h = kitti_eval.get_official_eval_result(g, d, classes)
    text_d, ret_d = KD.get_official_eval_result(g, d, classes)
    assert sorted(ret_d) == sorted(ret_h) and len(ret_h) == len(classes) * 3 * (3 if name == "noaos" else 4)
    for k, v in ret_h.items():
        assert abs(ret_d[k] - v) < 1e-9, (k, ret_d[k], v)
    assert text_d.splitlines() == text_h.splitlines()
    assert ("aos" in text_h) == (name != "noaos")


def test_empty_cases_follow_the_host():
    text_h, ret_h = kitti_eval.get_official_eval_result([], [], ["Car"])
    text_d, ret_d = KD.get_official_eval_result([], [], ["Car"])
    assert ret_d == ret_h and text_d == text_h
    g, d = with_empty_ends([], [])                                 # frames, but not one box
    r = KD.eval_class(KD.AnnoTables(g, d), CLASSES, 0, MO, True)
    assert all((v == 0).all() and v.shape == (3, 3, 2, 41) for v in r.values())
    g, d, _ = annos("edge")                                        # ground truth without detections, and the reverse
    none_d, none_g = with_empty_ends([], [])[1][:1] * len(g), with_empty_ends([], [])[0][:1] * len(g)
    for gg, dd in ((g, none_d), (none_g, d)):
        for metric in (0, 2):
            host = kitti_eval.eval_class(gg, dd, CLASSES, metric, MO, metric == 0)
            dev = KD.eval_class(KD.AnnoTables(gg, dd), CLASSES, metric, MO, metric == 0)
            for k in host:
                assert np.array_equal(dev[k], host[k]), (k, metric)


def test_two_runs_give_identical_buffers():
    _, _, t = annos("syn1212")
    for metric in (0, 1):
        a, b = (KD.match_statistics(t, CLASSES, metric, MO, metric == 0) for _ in range(2))
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (metric, k)     # bytes: NaN placeholders and the similarity sums included
        o1, o2 = (KD._read(KD.overlaps(t, metric)) for _ in range(2))
        assert o1.tobytes() == o2.tobytes()
    assert np.abs(a["sim"]).sum() == 0 and np.abs(KD.match_statistics(t, CLASSES, 0, MO, True)["sim"]).sum() > 0


@pytest.mark.parametrize("n_frames", [24, 96])
def test_eval_class_reads_the_device_twice_at_most(n_frames, monkeypatch):
    import torch
    g, d = synthetic_kitti_annos(1212, 24)
    reps = n_frames // 24
    t = KD.AnnoTables(g * reps, d * reps)
    t.dev                                                          # the upload is not a read
    torch.cuda.synchronize()
    reads = []
    real_cpu, real_item, real_tolist = torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append("cpu"), real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.append("item"), real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append("tolist"), real_tolist(self))[1])
    for metric in (0, 2):
        del reads[:]
        r = KD.eval_class(t, CLASSES, metric, MO, metric == 0)
        assert reads == ["cpu", "cpu"], reads
        assert r["precision"].max() > 0
