"""Fixture G27 (tests/golden/g27_atss.npz): the reference's own ATSSTargetAssigner (atss_target_assigner.py).

Runs ONLY in the build container (needs /root/reference; CPU torch), like make_golden.py, whose in-memory loader it uses.  The
reference calls iou3d_nms_utils.boxes_iou_bev / boxes_iou3d_gpu, a native module its snapshot does not ship: the build's CPU oracle
(oracle.hvpr_oracle.boxes_iou_bev / boxes_iou3d, the fp32 sequence of hvpr_amd/csrc/iou_geom.h) stands in for it.  Everything else —
the trim, the distances and their topk, mean + std, the inside test, the scatter, the arg-maxes, the forced matches, the box code —
is the reference's own code.  The reference's head cannot construct the class (anchor_head_template.py:54-71 passes a
`use_multihead` the constructor does not take): the maker executes that constructor line, records the TypeError's text, and drives
ATSSTargetAssigner directly, on G18's 40 x 32 grid and two class configurations, TOPK 8 with MATCH_HEIGHT off and on and TOPK 1,
on G18's frames, tests/assign3d_cases.extra_frames and tests/atss_cases.atss_frames.

A frame is PINNED for a run when the reference's outcome cannot hang on what is not specified: the host form of tests/atss_cases.py
meets no tie at the cut of the TOPK nearest (torch.topk decides ties its own way) and margins of at least 1e-5 — relative for the
distances, absolute for |iou - thresh|, for the gap between IoUs that a maximum compares (the device's table differs from the
oracle's in the last bits, and G27 is also run on the device) and, in metres, for the inside test.  With TOPK 1 the threshold is
NaN and no candidate is positive: only the maxima's margin (the forced matches) counts there.  A pinned frame is asserted equal to
the host form here (labels and weights exactly, targets 1e-5).

The frames made for G27 (atss_cases.atss_frames, built from boxes searched for to be well conditioned on all three anchor sets)
are ASSERTED to meet every margin in every run on both heads; a failure there means: fix the frame.  A class value outside
0 .. n_classes in one of them (other_class_on_car_anchor on the one-class head) is mapped to label 0 in the reference's rows before
they are stored: deviation (f), applied here as the test applies (b).  The frames taken over from G18 and G26 are what those
fixtures define and are not this file's to move; they carry the flag, and an unpinned one stores its ground truths only.  On the
three-class head few of them can be pinned at ANY TOPK, and rightly: a car over the pedestrian anchors (or a pedestrian under the
car anchors) has every nearby anchor wholly inside (around) it, its IoUs with them are one value up to rounding, so `iou >= mean +
std + 1e-6` sits 1e-6 from equality and the ground truth's best anchor — the forced match, TOPK 1 included — is decided by the
last bit: the reference's own outcome is rounding noise there.  Three sets in one head order are pinned by the frames made here.
The one exception to the inside margin is the case `face6` of atss_cases.face6_case, six anchors of its own with one centre
exactly on a face (its docstring says why G18's grid has no such frame at TOPK 8): the reference's labels for it and for its
nudged twin are stored under face6.* / face6_nudged.*.  Only arrays and names are
written: G18's grid / class keys, <cfg>.<frame>.gt, <cfg>.runs, and per run and pinned frame and anchor set the reference's rows
in the set's own order: labels (int8), pos_idx, pos_targets (every other target row is exactly zero and the weights are
labels > 0, asserted here).  All frames of a configuration padded to 50 rows are one batch; the reference gives for it, frame by
frame, what it gives for the frames alone (asserted here).

Usage:  python tests/golden/make_golden_atss.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_golden as G  # noqa: E402
from make_golden import G18_CLASSES, G18_PAD, G18_ROTATIONS, _g18_head_cfg, g18_frames  # noqa: E402

import assign3d_cases as A3  # noqa: E402
import atss_cases as AT  # noqa: E402

RUNS = [(8, 0), (8, 1), (1, 0)]
BAR = 1e-5
NEW = ["other_class_on_car_anchor", "class0_in_the_middle", "all_zero_table", "shared_best_anchor", "out_of_range_and_near", "spread12"]


def tie_rules_of_this_torch():
    """Items 5 and 6: first maximum along both axes, last write of an indexed assignment with repeated indices."""
    t = torch.tensor([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [1.0, 0.5, 2.0]])
    assert t.max(dim=1)[1].tolist() == [0, 1, 2] and t.max(dim=0)[1].tolist() == [0, 1, 1]
    big = torch.zeros(5000, 3)
    big[[7, 4100], 1] = 1.0
    assert big.max(dim=0)[1].tolist() == [0, 7, 0]
    v = torch.zeros(4)
    v[torch.tensor([2, 1, 2])] = torch.tensor([5.0, 6.0, 7.0])
    assert v.tolist() == [0.0, 6.0, 7.0, 0.0]


def main():
    R = G.load_reference()
    O = G._import_oracle()
    calls = {"bev": 0, "3d": 0}

    def stand_in(kind, fn):
        def f(a, b):
            calls[kind] += 1
            return torch.from_numpy(fn(np.ascontiguousarray(a.numpy()), np.ascontiguousarray(b.numpy())))
        return f
    R.atss.iou3d_nms_utils.boxes_iou_bev = stand_in("bev", O.boxes_iou_bev)
    R.atss.iou3d_nms_utils.boxes_iou3d_gpu = stand_in("3d", O.boxes_iou3d)
    tie_rules_of_this_torch()
    nx, ny = 40, 32
    rng = np.array([0, -2.56, -2.5, 6.4, 2.56, 0.5], dtype=np.float32)     # as G18
    out = dict(nx=nx, ny=ny, point_cloud_range=rng, anchor_rotations=np.array(G18_ROTATIONS, np.float64), pad_rows=G18_PAD,
               configs=np.array(list(G18_CLASSES)))
    for which, (names, sizes, heights, matched, unmatched) in G18_CLASSES.items():
        torch.manual_seed(1800)
        head = R.head_single.AnchorHeadSingle(model_cfg=_g18_head_cfg(which), input_channels=8, num_class=len(names), class_names=names,
                                              grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
        cfg = _g18_head_cfg(which)
        cfg.TARGET_ASSIGNER_CONFIG.NAME = "ATSS"
        cfg.TARGET_ASSIGNER_CONFIG.TOPK = 8
        try:                                                              # deviation (a): the head's own constructor line
            R.head_single.AnchorHeadSingle(model_cfg=cfg, input_channels=8, num_class=len(names), class_names=names,
                                           grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
            raise AssertionError("the reference's head constructed ATSSTargetAssigner")
        except TypeError as e:
            assert "use_multihead" in str(e), e
            out["head_constructor_error"] = np.array(str(e))
        anchors = [a.clone() for a in head.anchors]
        flat = [a.reshape(-1, 7).numpy().astype(np.float32) for a in anchors]
        sets = [(a, len(G18_ROTATIONS)) for a in flat]
        frames, _ = g18_frames(which, head.anchors, R.box_utils.boxes3d_nearest_bev_iou)
        for more in (A3.extra_frames(which), AT.atss_frames(which, anchors[0][0, :, :, 0].numpy())):
            assert not set(frames) & set(more)
            frames.update(more)
        out.update({f"{which}.class_names": np.array(names), f"{which}.anchor_sizes": np.array(sizes, np.float64),
                    f"{which}.anchor_bottom_heights": np.array(heights, np.float64), f"{which}.matched": np.array(matched, np.float64),
                    f"{which}.unmatched": np.array(unmatched, np.float64), f"{which}.cases": np.array(list(frames)),
                    f"{which}.runs": np.array(RUNS, np.int32), f"{which}.n_sets": len(sets)})
        for name, gt in frames.items():
            out[f"{which}.{name}.gt"] = gt
        batch = np.zeros((len(frames), G18_PAD, 8), np.float32)
        for i, gt in enumerate(frames.values()):
            batch[i, :len(gt)] = gt
        cuts = np.cumsum([0] + [a.shape[0] for a in flat])
        for topk, mh in RUNS:
            ref = R.atss.ATSSTargetAssigner(topk=topk, box_coder=head.box_coder, match_height=bool(mh))
            iou = AT.oracle_iou(mh)
            whole = ref.assign_targets([a.clone() for a in anchors], torch.from_numpy(batch.copy()))
            n_pinned, why = 0, {}
            for i, (name, gt) in enumerate(frames.items()):
                t = ref.assign_targets([a.clone() for a in anchors], torch.from_numpy(gt.copy())[None])
                got = tuple(t[k][0].numpy() for k in ("box_cls_labels", "box_reg_targets", "reg_weights"))
                for k, key in enumerate(("box_cls_labels", "box_reg_targets", "reg_weights")):
                    assert np.array_equal(whole[key][i].numpy(), got[k]), (which, topk, mh, name, key)
                lab, tgt, w = got
                assert np.isfinite(tgt).all() and np.isfinite(lab).all() and np.array_equal(lab, np.round(lab))
                assert not tgt[lab <= 0].any() and np.array_equal(w, (lab > 0).astype(np.float32))
                n = AT.trim_rows(gt)
                cls_ok = bool(((gt[:n, 7] >= 0) & (gt[:n, 7] <= len(names))).all())
                per_set, mg = [], AT.new_margins()
                for a, _ in sets:
                    h = AT.host_atss_set(a, gt, len(names), topk, iou)
                    per_set.append(h[:3])
                    mg = AT.merge_margins(mg, h[3])
                bad = []
                if topk > 1:
                    bad += ["tie at the cut"] if mg["ties"] else []
                    bad += ["distance margin"] if mg["nearest"] < BAR else []
                    bad += ["threshold margin"] if mg["thresh"] < BAR else []
                    bad += ["inside margin"] if mg["inside"] < BAR else []
                    bad += ["centre on a face"] if mg["on_face"] else []
                bad += ["maxima margin"] if mg["maxima"] < BAR else []
                bad += ["class out of range"] if not cls_ok and name not in NEW else []
                if not cls_ok and name in NEW:                            # deviation (f), applied to the reference's rows
                    out_of = lab > len(names)
                    assert out_of.any()
                    lab, tgt = np.where(out_of, 0, lab).astype(lab.dtype), np.where(out_of[:, None], 0, tgt).astype(tgt.dtype)
                key = f"{which}.k{topk}.mh{mh}.{name}."
                out[key + "pinned"] = np.array(not bad)
                if bad:
                    why[name] = bad
                    assert name not in NEW, (which, topk, mh, name, bad, mg)     # fix the frame; the bar stays
                    continue
                n_pinned += 1
                for s, (hl, ht, hw) in enumerate(per_set):
                    rl, rt = lab[cuts[s]:cuts[s + 1]], tgt[cuts[s]:cuts[s + 1]]
                    AT.check_equal((hl, ht, hw), (rl.astype(np.int32), rt, (rl > 0).astype(np.float32)), f"{key}s{s}")
                    pos = np.nonzero(rl > 0)[0]
                    assert rl.min() >= 0 and rl.max() <= len(names)
                    out.update({key + f"s{s}.labels": rl.astype(np.int8), key + f"s{s}.pos_idx": pos.astype(np.int32),
                                key + f"s{s}.pos_targets": rt[pos]})
            print(f"g27 {which} topk {topk} match_height {mh}: {n_pinned} of {len(frames)} frames pinned; unpinned:", why)
    for tag, nudge in (("face6", False), ("face6_nudged", True)):
        anchors, gt, topk = AT.face6_case(nudge)
        for mh in (0, 1):
            ref = R.atss.ATSSTargetAssigner(topk=topk, box_coder=head.box_coder, match_height=bool(mh))
            t = ref.assign_targets([torch.from_numpy(anchors.copy())], torch.from_numpy(gt.copy())[None])
            lab, tgt = t["box_cls_labels"][0].numpy(), t["box_reg_targets"][0].numpy()
            hl, ht, hw, mg = AT.host_atss_set(anchors, gt, 1, topk, AT.oracle_iou(mh))
            assert mg["on_face"] == (0 if nudge else 1) and mg["thresh"] >= BAR and mg["ties"] == 0, mg
            assert mg["inside"] >= (1e-8 if nudge else BAR), mg            # the nudged twin is one fp32 step (6e-8 m) outside, on purpose
            assert lab.tolist() == ([1, 0, 0, 0, 0, 0] if nudge else [1, 1, 0, 0, 0, 0]), lab
            AT.check_equal((hl, ht, hw), (lab.astype(np.int32), tgt, (lab > 0).astype(np.float32)), f"{tag} mh{mh}")
            out.update({f"{tag}.mh{mh}.labels": lab.astype(np.int8), f"{tag}.mh{mh}.targets": tgt})
    assert calls["bev"] and calls["3d"], calls
    path = os.path.join(G.OUT, "g27_atss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", calls, "calls of the stand-ins")


if __name__ == "__main__":
    main()
