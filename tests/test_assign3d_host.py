"""CPU: the MATCH_HEIGHT / NORM_BY_NUM_EXAMPLES target assigner without a device.  The numpy host form of tests/assign3d_cases.py over
the build's CPU oracle of the rotated 3-D IoU reproduces fixture G26 — the reference's own AxisAlignedTargetAssigner with
MATCH_HEIGHT True (tests/golden/make_golden_assign3d.py) — so the GPU suite may use that form, fed with any IoU table, as its
statement of the semantics; and the two _ex entry points are exported, bound from include/hvpr_amd.h and sized on the host."""
import ctypes

import numpy as np
import pytest

import assign3d_cases as A3


@pytest.fixture(scope="module")
def g26(golden_dir):
    return A3.load_g26(golden_dir)


@pytest.mark.parametrize("which", ["car", "3c"])
def test_host_form_over_the_oracle_reproduces_g26(g26, which):
    """Every frame of G26 alone, NORM_BY_NUM_EXAMPLES False and True: labels and reg_weights exactly the reference's, reg_targets
    within 1e-5 (the bar of G8 and G18); then all frames padded to 50 rows as one batch, frame by frame the same arrays."""
    sets, names = A3.g26_anchor_sets(g26, which)
    iou = A3.oracle_iou3d()
    cases = [str(c) for c in g26[which + ".cases"]]
    assert len(cases) == {"car": 29, "3c": 32}[which]
    alone = {}
    for name in cases:
        gt = g26[f"{which}.{name}.gt"]
        for norm in (False, True):
            got = tuple(x[0] for x in A3.host_assign(sets, gt[None], len(names), norm, iou))
            A3.check_against_g26(g26, which, name, norm, got)
            alone[name, norm] = got
        assert np.array_equal(alone[name, False][0], alone[name, True][0]) and np.array_equal(alone[name, False][1], alone[name, True][1])
    batch = np.zeros((len(cases), int(g26["pad_rows"]), 8), np.float32)
    for i, name in enumerate(cases):
        gt = g26[f"{which}.{name}.gt"]
        batch[i, :len(gt)] = gt
    whole = A3.host_assign(sets, batch, len(names), True, iou)
    for i, name in enumerate(cases):
        for k in range(3):
            assert np.array_equal(whole[k][i], alone[name, True][k]), (which, name, k)


def test_g26_cases_do_what_they_are_for(g26):
    """With the flag the ground truth above the anchors (BEV overlap, disjoint in z) matches nothing; the nearest-axis matcher, fed the
    same frame, forces a match.  The corner frame leaves a workgroup one pair to clip, the stacked frame more than eight rounds."""
    sets, names = A3.g26_anchor_sets(g26, "car")
    gt = g26["car.z_disjoint_only.gt"]
    assert not (g26["car.z_disjoint_only.labels"] > 0).any() and (g26["car.z_sliver.labels"] > 0).sum() == 1
    import torch
    import torch_forms
    nearest = lambda a, b: torch_forms.boxes3d_nearest_bev_iou(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())).numpy()
    lab, _, _ = A3.host_assign(sets, gt[None], 1, False, nearest)
    assert (lab > 0).sum() >= 1
    assert (A3.pairs_per_workgroup(sets[0][0], g26["car.corner_reach.gt"], 0, 1) == 1).any()
    assert A3.pairs_per_workgroup(sets[0][0], g26["car.stacked10.gt"], 0, 1).max() >= 8 * 64


def test_ex_entry_points_are_exported_and_bound_from_the_header():
    from hvpr_amd import _lib, build
    L = ctypes.CDLL(build.build())
    ex = ["hvpr_assign_targets_ex_f32", "hvpr_assign_targets_ex_workspace_bytes"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hvpr_assign_targets_ex_")) == ex
    for n in ex:
        assert hasattr(L, n) and n in _lib.PARAMS, n
    old, new = _lib.SIGNATURES["hvpr_assign_targets_f32"], _lib.SIGNATURES["hvpr_assign_targets_ex_f32"]
    assert new[0] is ctypes.c_int and new[1] == old[1][:17] + [ctypes.c_int, ctypes.c_int] + old[1][17:]
    names = [p for p, _ in _lib.PARAMS["hvpr_assign_targets_ex_f32"]]
    assert names[:17] == [p for p, _ in _lib.PARAMS["hvpr_assign_targets_f32"]][:17]
    assert names[17:] == ["match_height", "norm_by_num_examples", "workspace", "workspace_bytes", "stream"]
    assert _lib.lib().hvpr_abi_version() == 8
    assert "hvpr_assign_targets_ex_f32" in _lib._calls


def test_ex_workspace_query_needs_no_gpu():
    from hvpr_amd import _lib
    L = _lib.lib()
    for mh in (0, 1):
        for B, G in ((1, 0), (1, 4), (16, 50), (3, 256)):
            need = L.hvpr_assign_targets_ex_workspace_bytes(B, G, 960, mh)
            assert need >= L.hvpr_assign_targets_workspace_bytes(B, G) + 256 + 4 * B and need % 256 == 0
        assert L.hvpr_assign_targets_ex_workspace_bytes(0, 4, 960, mh) == 0
        assert L.hvpr_assign_targets_ex_workspace_bytes(1, -1, 960, mh) == 0
        assert L.hvpr_assign_targets_ex_workspace_bytes(1, 4, 0, mh) == 0


def test_assigner_takes_both_flags_and_still_refuses_sampling_and_cpu_tensors():
    import torch
    from hvpr_amd import anchor_head
    from hvpr_amd.config import hvpr_car_cfg
    cfg = hvpr_car_cfg().MODEL.DENSE_HEAD
    cfg.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT = True
    cfg.TARGET_ASSIGNER_CONFIG.NORM_BY_NUM_EXAMPLES = True
    head = anchor_head.AnchorHeadSingle(model_cfg=cfg, input_channels=64, num_class=1, class_names=["Car"], grid_size=np.array([16, 16, 1]),
                                        point_cloud_range=np.array([0, -1.28, -3, 2.56, 1.28, 1], np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the flags are taken; the CPU is still refused
        head.assign_targets(torch.zeros(1, 2, 8))
    assert head.target_assigner.match_height is True and head.target_assigner.norm_by_num_examples is True
    cfg.TARGET_ASSIGNER_CONFIG.POS_FRACTION = 0.5
    head.target_assigner = None
    with pytest.raises(AssertionError, match="no fg/bg sampling"):
        head.assign_targets(torch.zeros(1, 2, 8))
