"""CPU: the ATSS target assigner without a device.  The numpy host form of tests/atss_cases.py over the build's CPU oracle of the
rotated BEV / 3-D IoU reproduces fixture G27 — the reference's own ATSSTargetAssigner (tests/golden/make_golden_atss.py) — on every
pinned frame, so the GPU suite may use that form, fed with any IoU table, as its statement of the semantics; the two ATSS entry
points are exported, bound from include/hvpr_amd.h and sized on the host; hvpr_car_atss.yaml loads and the head picks the class."""
import ctypes

import numpy as np
import pytest

import atss_cases as AT


@pytest.fixture(scope="module")
def g27(golden_dir):
    return AT.load_g27(golden_dir)


@pytest.mark.parametrize("which", ["car", "3c"])
def test_host_form_over_the_oracle_reproduces_g27(g27, which):
    """Every pinned frame of G27 alone, TOPK 8 with MATCH_HEIGHT off and on and TOPK 1: labels and reg_weights exactly the
    reference's, reg_targets within 1e-5, the reference's per-set rows mapped into the head's order; then all frames padded to 50
    rows as one batch, frame by frame the same arrays.  The six frames made for G27 (atss_cases.atss_frames) are pinned in every
    run on both heads.  Of G18's and G26's frames the one-class head pins 22 of 29 at TOPK 8, the three-class head 7 or 8 of 32 (a
    car over the pedestrian anchors has one IoU with all anchors under it, up to rounding: neither the candidates' threshold nor
    the ground truth's best anchor is then more than noise, at any TOPK — the maker's docstring)."""
    sets, names = AT.g27_anchor_sets(g27, which)
    cases = [str(c) for c in g27[which + ".cases"]]
    assert len(cases) == {"car": 35, "3c": 38}[which]
    assert AT.g27_runs(g27, which) == [(8, 0), (8, 1), (1, 0)]
    batch = np.zeros((len(cases), int(g27["pad_rows"]), 8), np.float32)
    for i, name in enumerate(cases):
        gt = g27[f"{which}.{name}.gt"]
        batch[i, :len(gt)] = gt
    n_pinned = {}
    for topk, mh in AT.g27_runs(g27, which):
        iou = AT.oracle_iou(mh)
        whole = AT.host_atss(sets, batch, len(names), topk, iou)
        n_pinned[topk, mh] = 0
        for i, name in enumerate(cases):
            gt, pinned, per_set = AT.g27_case(g27, which, topk, mh, name)
            got = tuple(x[0] for x in AT.host_atss(sets, gt[None], len(names), topk, iou)[:3])
            for k in range(3):
                assert np.array_equal(whole[k][i], got[k]), (which, topk, mh, name, k)
            assert pinned or name not in AT.atss_frames(which), (which, topk, mh, name)      # the frames made for G27 are pinned everywhere
            if pinned:
                n_pinned[topk, mh] += 1
                AT.check_equal(got, AT.g27_head_order(sets, per_set), f"{which} topk {topk} mh {mh} {name}")
            if name == "spread12" and topk == 8:                  # the candidate path at large: positives beyond the forced ones (ATSS at TOPK 8 passes one or two anchors a box, mostly the forced one)
                assert (got[0] > 0).sum() >= 12 * len(sets) + 2, (got[0] > 0).sum()
    want = {"car": {(8, 0): 28, (8, 1): 28, (1, 0): 30}, "3c": {(8, 0): 13, (8, 1): 14, (1, 0): 14}}[which]
    assert n_pinned == want


def test_g27_cases_do_what_they_are_for(g27):
    """No class mask (a class-2 row labels car anchors 2 on the three-class head, 0 on the one-class head), a class-0 row in the
    middle labels nothing, an all-zero table gives no positive and forces anchor 0, twins share their best anchor and the higher row
    takes it, TOPK 1 gives forced matches only, and the reference's head cannot construct the class."""
    assert "use_multihead" in str(g27["head_constructor_error"])
    sets3, names3 = AT.g27_anchor_sets(g27, "3c")
    sets1, _ = AT.g27_anchor_sets(g27, "car")
    iou = AT.oracle_iou(0)
    gt = g27["3c.other_class_on_car_anchor.gt"]
    lab3 = AT.host_atss_set(sets3[0][0], gt, 3, 1, iou)[0]
    assert (lab3 == 2).sum() == 1 and (lab3 != 0).sum() == 1                      # on the CAR set, TOPK 1: the forced match
    assert not AT.host_atss_set(sets1[0][0], gt, 1, 8, iou)[0].any()              # class 2 of 1: label 0 (deviation (f))
    lab, _, _, mg = AT.host_atss_set(sets1[0][0], g27["car.class0_in_the_middle.gt"], 1, 8, iou)
    only = AT.host_atss_set(sets1[0][0], g27["car.class0_in_the_middle.gt"][[0, 2]], 1, 8, iou)[0]
    assert (lab > 0).sum() >= 2 and (lab > 0).sum() <= (only > 0).sum()           # the class-0 row takes anchors, never gives any
    lab, tgt, w, mg = AT.host_atss_set(sets1[0][0], g27["car.all_zero_table.gt"], 1, 8, iou)
    assert lab[0] == 1 and (lab > 0).sum() == 1 and w[0] == 1 and mg["thresh"] == AT.INF
    labels = g27["car.k8.mh0.all_zero_table.s0.labels"]
    assert labels[0] == 1 and (labels > 0).sum() == 1                             # ... as in the reference: no `> 0` guard
    lab = AT.host_atss_set(sets3[0][0], g27["3c.shared_best_anchor.gt"], 3, 1, iou)[0]
    assert (lab == 3).sum() == 1 and (lab == 1).sum() == 0                        # the last write: the higher row
    for name in ("random50", "stacked10"):
        lab = AT.host_atss_set(sets1[0][0], g27[f"car.{name}.gt"], 1, 1, iou)[0]
        assert 1 <= (lab > 0).sum() <= AT.trim_rows(g27[f"car.{name}.gt"])
    lab = g27["car.k8.mh0.out_of_range_and_near.s0.labels"]
    assert lab[0] == 1 and (lab > 0).sum() >= 2


def test_a_centre_exactly_on_a_face_is_inside(g27):
    """face6 (atss_cases.face6_case): anchor 1 is positive only through the closed inside test; one fp32 step further out it is not.
    The reference's labels for both, MATCH_HEIGHT off and on."""
    for tag, nudge, want in (("face6", False, [1, 1, 0, 0, 0, 0]), ("face6_nudged", True, [1, 0, 0, 0, 0, 0])):
        anchors, gt, topk = AT.face6_case(nudge)
        for mh in (0, 1):
            lab, tgt, w, mg = AT.host_atss_set(anchors, gt, 1, topk, AT.oracle_iou(mh))
            assert lab.tolist() == want and mg["on_face"] == (0 if nudge else 1) and mg["thresh"] >= 1e-3
            ref = g27[f"{tag}.mh{mh}.labels"].astype(np.int32)
            AT.check_equal((lab, tgt, w), (ref, g27[f"{tag}.mh{mh}.targets"], (ref > 0).astype(np.float32)), f"{tag} mh {mh}")


@pytest.mark.parametrize("topk", [1, 9, 63])
def test_odd_topk_and_ties_run_through_the_host_form_alone(g27, topk):
    """UNPINNED: the two rotations of a location are at one distance, so an odd TOPK on a two-rotation set cuts inside a tie, which
    the product decides by the anchor index (the lower index, rotation 0, stays) and torch.topk in its own way; the same holds for
    a ground truth on an anchor centre (G18's on_anchor_* frames: the neighbours left and right tie).  The host form alone: the tie
    is counted, the candidates are the lowest keys, the outputs are consistent, and G27 does not pin such a frame."""
    sets, _ = AT.g27_anchor_sets(g27, "car")
    anchors = sets[0][0]
    iou = AT.oracle_iou(0)
    gt = g27["car.random50.gt"]
    lab, tgt, w, mg = AT.host_atss_set(anchors, gt, 1, topk, iou)
    assert mg["ties"] == AT.trim_rows(gt)                                         # every ground truth cuts inside a rotation pair
    assert lab.min() >= 0 and lab.max() == 1 and np.array_equal(w, (lab > 0).astype(np.float32)) and not tgt[lab == 0].any()
    assert np.isfinite(tgt).all() and (lab > 0).sum() >= 1
    keys, d = AT.distance_keys(anchors, gt[0])
    order = np.argsort(keys, kind="stable")
    assert d[order[topk - 1]] == d[order[topk]] and order[topk - 1] + 1 == order[topk] and order[topk - 1] % 2 == 0
    for name in ("on_anchor_exact", "on_anchor_square"):
        assert not bool(g27[f"car.k8.mh0.{name}.pinned"])


def test_atss_entry_points_are_exported_and_bound_from_the_header():
    """A name declared twice and a missing header: test_capi_symbols.py (the parser's duplicate case, test_missing_header_is_named)."""
    from hvpr_amd import _lib, build
    L = ctypes.CDLL(build.build())
    atss = ["hvpr_assign_targets_atss_f32", "hvpr_assign_targets_atss_workspace_bytes"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hvpr_assign_targets_atss_")) == atss
    for n in atss:
        assert hasattr(L, n) and n in _lib.PARAMS, n
    res, args = _lib.SIGNATURES["hvpr_assign_targets_atss_f32"]
    i, ll, p, z = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_size_t
    assert res is i and args == [p, i, p, i, i, i, i, i, i, i, i, ll, p, p, p, p, p, z, p]
    import torch
    kinds = _lib.PARAMS["hvpr_assign_targets_atss_f32"]
    assert [n for n, _ in kinds] == ["anchors", "n_anchors", "gt_boxes", "batch", "n_gt", "n_classes", "topk", "match_height", "per_loc",
                                     "loc_stride", "loc_offset", "anchors_total", "labels", "reg_targets", "reg_weights", "pos_count",
                                     "workspace", "workspace_bytes", "stream"]
    assert {n: k for n, k in kinds if k is not None} == {"anchors": torch.float32, "gt_boxes": torch.float32, "labels": torch.int32,
                                                         "reg_targets": torch.float32, "reg_weights": torch.float32,
                                                         "pos_count": torch.int32, "workspace": _lib.ANY}
    assert _lib.SIGNATURES["hvpr_assign_targets_atss_workspace_bytes"] == (z, [i, i, i, i])
    assert _lib.lib().hvpr_abi_version() == 8
    assert "hvpr_assign_targets_atss_f32" in _lib._calls


def test_atss_workspace_query_needs_no_gpu():
    from hvpr_amd import _lib
    q = _lib.lib().hvpr_assign_targets_atss_workspace_bytes
    for B, G, A, k in ((1, 0, 960, 9), (1, 4, 64, 64), (16, 50, 107136, 9), (3, 256, 2049, 1)):
        need = q(B, G, A, k)
        chunks = (A + 2047) // 2048
        assert need % 256 == 0 and need >= 4 * B + 8 * B * max(G, 1) + 8 * B * A + 8 * B * max(G, 1) * chunks * k
        assert need <= 4 * 256 + 4 * B + 8 * B * max(G, 1) + 8 * B * A + 8 * B * max(G, 1) * chunks * k
    assert q(16, 50, 107136, 9) > q(16, 50, 107136, 8) > q(15, 50, 107136, 8)
    for bad in ((0, 4, 960, 9), (1, -1, 960, 9), (1, 4, 0, 9), (1, 4, 960, 0), (1, 4, 960, 65)):
        assert q(*bad) == 0, bad


def _head(cfg):
    from hvpr_amd import anchor_head
    return anchor_head.AnchorHeadSingle(model_cfg=cfg, input_channels=64, num_class=1, class_names=["Car"], grid_size=np.array([16, 16, 1]),
                                        point_cloud_range=np.array([0, -1.28, -3, 2.56, 1.28, 1], np.float32))


def test_the_shipped_yaml_loads_and_the_head_picks_the_atss_class():
    import torch
    from hvpr_amd import config, target_assigner
    base, cfg = config.hvpr_car_cfg(), config.hvpr_car_atss_cfg()
    t = cfg.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG
    assert t.NAME == "ATSS" and t.TOPK == 9 and t.MATCH_HEIGHT is False and t.BOX_CODER == "ResidualCoder"
    assert base.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.NAME == "AxisAlignedTargetAssigner" and "TOPK" not in base.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG
    t.pop("TOPK"), cfg.pop("_BASE_CONFIG_")
    t.NAME = "AxisAlignedTargetAssigner"
    assert cfg == base                                                            # everything else is hvpr_car.yaml, its includes resolved
    cfg = config.hvpr_car_atss_cfg().MODEL.DENSE_HEAD
    cfg.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT = True
    head = _head(cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # the class is picked; the CPU is still refused
        head.assign_targets(torch.zeros(1, 2, 8))
    a = head.target_assigner
    assert isinstance(a, target_assigner.ATSSTargetAssigner) and a.topk == 9 and a.match_height is True and a.n_classes == 1
    assert a.box_coder is head.box_coder
    head = _head(base.MODEL.DENSE_HEAD)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.assign_targets(torch.zeros(1, 2, 8))
    assert isinstance(head.target_assigner, target_assigner.AxisAlignedTargetAssigner)


def test_a_missing_topk_and_an_unknown_name_raise():
    import torch
    from hvpr_amd import config, target_assigner
    cfg = config.hvpr_car_atss_cfg().MODEL.DENSE_HEAD
    cfg.TARGET_ASSIGNER_CONFIG.pop("TOPK")
    with pytest.raises(KeyError, match="TOPK"):
        _head(cfg).assign_targets(torch.zeros(1, 2, 8))
    cfg = config.hvpr_car_atss_cfg().MODEL.DENSE_HEAD
    cfg.TARGET_ASSIGNER_CONFIG.NAME = "SomethingElse"
    with pytest.raises(NotImplementedError, match="SomethingElse"):
        _head(cfg).assign_targets(torch.zeros(1, 2, 8))
    for topk in (0, 65):
        with pytest.raises(ValueError, match="TOPK"):
            target_assigner.ATSSTargetAssigner(topk, None)
    cfg = config.hvpr_car_atss_cfg().MODEL.DENSE_HEAD
    cfg.USE_MULTIHEAD = True
    with pytest.raises(AssertionError, match="single head"):                      # USE_MULTIHEAD still raises
        _head(cfg)


def test_a_base_config_that_includes_files_itself_is_resolved_at_any_depth(tmp_path):
    """hvpr_car_atss.yaml bases itself on a model yaml whose DATA_CONFIG has an include of its own; an include two levels down in
    the base resolves too, and a base without includes is taken as it always was."""
    from hvpr_amd import config
    d = tmp_path / "cfgs"
    d.mkdir()
    (d / "leaf.yaml").write_text("P: 1\nQ: [1, 2]\n")
    (d / "mid.yaml").write_text("A:\n    B:\n        _BASE_CONFIG_: %s\n        P: 2\n    C: 3\nD: 4\n" % (d / "leaf.yaml"))
    (d / "top.yaml").write_text("_BASE_CONFIG_: %s\nA:\n    C: 5\nE: 6\n" % (d / "mid.yaml"))
    (d / "plain.yaml").write_text("_BASE_CONFIG_: %s\nP: 7\n" % (d / "leaf.yaml"))
    top = config.cfg_from_yaml_file(str(d / "top.yaml"))
    assert top.A.B.P == 2 and top.A.B.Q == [1, 2] and top.A.C == 5 and top.D == 4 and top.E == 6
    mid = config.cfg_from_yaml_file(str(d / "mid.yaml"))
    assert mid.A.B.Q == [1, 2] and mid.A.C == 3
    plain = config.cfg_from_yaml_file(str(d / "plain.yaml"))
    assert plain.P == 7 and plain.Q == [1, 2]
