"""Fixture G26 (tests/golden/g26_assigner_match_height.npz): the reference's own AxisAlignedTargetAssigner with MATCH_HEIGHT True,
NORM_BY_NUM_EXAMPLES False and True.

Runs ONLY in the build container (needs /root/reference; CPU torch), like make_golden.py, whose in-memory loader it uses.  The
reference's MATCH_HEIGHT branch calls iou3d_nms_utils.boxes_iou3d_gpu, a native module its snapshot does not ship: the build's
CPU oracle (oracle.hvpr_oracle.boxes_iou3d, the fp32 sequence of hvpr_amd/csrc/iou_geom.h) stands in for it.  Everything else —
the trim of padded rows, the class masks, the arg-maxes, the forced matches, the box code, NORM_BY_NUM_EXAMPLES — is the
reference's own code, run through AnchorHeadSingle.assign_targets on G18's 40 x 32 grid for G18's two class configurations
(car only, three classes), on G18's edge frames and on tests/assign3d_cases.extra_frames.  Only arrays and key names are written:
G18's grid / class keys, and per configuration and frame  <cfg>.<frame>.gt, .labels (int8), .pos_idx, .pos_targets (every other
target row is exactly zero, asserted here), .reg_weights (NORM_BY_NUM_EXAMPLES False) and .reg_weights_norm (True; labels and
targets do not depend on that flag, asserted here).  All frames of a configuration padded to 50 rows are one mixed batch; the
reference gives for it, frame by frame, what it gives for the frames alone (asserted here).

Usage:  python tests/golden/make_golden_assign3d.py
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


def main():
    R = G.load_reference()
    O = G._import_oracle()
    calls = []

    def iou3d(a, b):
        calls.append(tuple(a.shape) + tuple(b.shape))
        return torch.from_numpy(O.boxes_iou3d(a.numpy(), b.numpy()))
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"].boxes_iou3d_gpu = iou3d
    nx, ny = 40, 32
    rng = np.array([0, -2.56, -2.5, 6.4, 2.56, 0.5], dtype=np.float32)     # as G18
    out = dict(nx=nx, ny=ny, point_cloud_range=rng, anchor_rotations=np.array(G18_ROTATIONS, np.float64), pad_rows=G18_PAD,
               configs=np.array(list(G18_CLASSES)))
    for which, (names, sizes, heights, matched, unmatched) in G18_CLASSES.items():
        heads = {}
        for norm in (False, True):
            cfg = _g18_head_cfg(which)
            cfg.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT = True
            cfg.TARGET_ASSIGNER_CONFIG.NORM_BY_NUM_EXAMPLES = norm
            torch.manual_seed(1800)
            heads[norm] = R.head_single.AnchorHeadSingle(model_cfg=cfg, input_channels=8, num_class=len(names), class_names=names,
                                                         grid_size=np.array([nx, ny, 1]), point_cloud_range=rng)
            assert heads[norm].target_assigner.match_height is True and heads[norm].target_assigner.norm_by_num_examples is norm
        frames, _ = g18_frames(which, heads[False].anchors, R.box_utils.boxes3d_nearest_bev_iou)
        extra = A3.extra_frames(which)
        assert not set(frames) & set(extra)
        frames.update(extra)
        out.update({f"{which}.class_names": np.array(names), f"{which}.anchor_sizes": np.array(sizes, np.float64),
                    f"{which}.anchor_bottom_heights": np.array(heights, np.float64), f"{which}.matched": np.array(matched, np.float64),
                    f"{which}.unmatched": np.array(unmatched, np.float64), f"{which}.cases": np.array(list(frames))})
        res = {}
        for name, gt in frames.items():
            per = {}
            for norm in (False, True):
                t = heads[norm].assign_targets(gt_boxes=torch.from_numpy(gt.copy())[None])
                per[norm] = tuple(t[k][0].numpy() for k in ("box_cls_labels", "box_reg_targets", "reg_weights"))
            lab, tgt, w = per[False]
            assert np.array_equal(lab, per[True][0]) and np.array_equal(tgt, per[True][1])
            pos = np.nonzero(lab > 0)[0]
            assert not tgt[lab <= 0].any() and np.isfinite(tgt).all() and lab.min() >= -1 and lab.max() <= len(names)
            assert np.array_equal(w, (lab > 0).astype(np.float32)) and np.array_equal(per[True][2] > 0, lab > 0)
            res[name] = per
            out.update({f"{which}.{name}.gt": gt, f"{which}.{name}.labels": lab.astype(np.int8), f"{which}.{name}.reg_weights": w,
                        f"{which}.{name}.reg_weights_norm": per[True][2], f"{which}.{name}.pos_idx": pos.astype(np.int32),
                        f"{which}.{name}.pos_targets": tgt[pos]})
        npos = {k: int((v[False][0] > 0).sum()) for k, v in res.items()}
        # the cases do what they are for
        assert npos["z_disjoint_only"] == 0 and npos["z_sliver"] > 0, npos                   # IoU exactly 0: no forced match
        assert np.array_equal(res["z_disjoint_and_near"][False][0] > 0,
                              heads[False].assign_targets(gt_boxes=torch.from_numpy(frames["z_disjoint_and_near"][1:].copy())[None])
                              ["box_cls_labels"][0].numpy() > 0)
        assert np.array_equal(res["far_and_near"][False][0], res["near_only"][False][0]) and npos["near_only"] > 0
        assert npos["only_padding"] == npos["g1_all_zero"] == 0 and npos["g1_real"] > 0 and npos["zero_row0"] > 0
        assert npos["twins_real_first"] == npos["twins_same_class"] > 0 and npos["twins_class0_first"] == 0
        assert npos["on_anchor_exact"] >= 1 and npos["corner_reach"] >= 1 and npos["stacked10"] >= 1 and npos["headings"] >= 6
        k = 1 if which == "3c" else 0
        flat = heads[False].anchors[k].reshape(-1, 7).numpy()
        self_iou = O.boxes_iou3d(flat, frames["on_anchor_exact"][:, :7])[:, 0]
        hit = int(self_iou.argmax())
        # the anchor itself: IoU 1 to the rounding of the clipped polygon's area (the oracle gives 1.0 for the car, 1.0000005 for the pedestrian)
        assert abs(float(self_iou[hit]) - 1.0) <= 2e-6 and np.array_equal(flat[hit], frames["on_anchor_exact"][0, :7]), self_iou[hit]
        car = heads[False].anchors[0].reshape(-1, 7).numpy()
        wg = A3.pairs_per_workgroup(car, frames["corner_reach"], 0, len(names))
        assert (wg == 1).any(), wg[wg > 0]                                                   # a workgroup with a single surviving pair
        wg = A3.pairs_per_workgroup(car, frames["stacked10"], 0, len(names))
        assert wg.max() >= 8 * 64, wg.max()                                                  # ... and one with many rounds of 64
        # the three label bands of the random frame, and NORM_BY_NUM_EXAMPLES per frame and anchor set
        lab = res["random50"][False][0]
        assert (lab > 0).sum() >= 25 and (lab == -1).sum() > 0 and (lab == 0).sum() > 0
        w = res["random50"][True][2].reshape(ny, nx, len(names), -1)
        lab4 = lab.reshape(ny, nx, len(names), -1)
        for c in range(len(names)):
            n = max(int((lab4[:, :, c] >= 0).sum()), 1)
            assert np.array_equal(w[:, :, c], np.where(lab4[:, :, c] > 0, np.float32(1) / np.float32(n), np.float32(0)))
        # the mixed batch: every frame padded to 50 rows; the reference treats frames independently
        batch = np.zeros((len(frames), G18_PAD, 8), np.float32)
        for i, gt in enumerate(frames.values()):
            batch[i, :len(gt)] = gt
        for norm in (False, True):
            t = heads[norm].assign_targets(gt_boxes=torch.from_numpy(batch))
            for i, name in enumerate(frames):
                for key, v in zip(("box_cls_labels", "box_reg_targets", "reg_weights"), res[name][norm]):
                    assert np.array_equal(t[key][i].numpy(), v), (which, name, key)
        print(f"g26 {which}: positives per case", npos)
    assert calls, "the reference never took its MATCH_HEIGHT branch"
    path = os.path.join(G.OUT, "g26_assigner_match_height.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(calls), "calls of the stand-in")


if __name__ == "__main__":
    main()
