"""Anchor target assignment on the device through the library's own kernels.

AxisAlignedTargetAssigner (pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-213) with
boxes3d_nearest_bev_iou (pcdet/utils/box_utils.py:252-323) and ResidualCoder.encode_torch (pcdet/utils/box_coder_utils.py:13-43):
hvpr_assign_targets_f32, two launches per anchor set for the whole batch, results written in the head's anchor order.  The
reference trims padded ground-truth rows with a python loop over `.sum()` and takes its arg-maxes through `.cpu().numpy()`
(:53-57,:148,:153): two host syncs per frame; here there is none.  MATCH_HEIGHT True (the rotated 3-D IoU in place of the
nearest-axis one, :145) and NORM_BY_NUM_EXAMPLES True (:201-204) go through hvpr_assign_targets_ex_f32; with both false, as
hvpr.yaml:114-124 sets them, the call is the one it always was.  The head's losses rebuild their weights from the labels
(anchor_head_template.py:113-119, 190-192), so NORM_BY_NUM_EXAMPLES only changes the returned reg_weights, in the reference as
here.  POS_FRACTION < 0 only: the reference's sampling branch (:173-184) is not built.  CPU tensors raise (torch form:
tests/torch_forms.py).  NAME: ATSS selects ATSSTargetAssigner below (hvpr_assign_targets_atss_f32).  The three entry points are
declared side by side in include/hvpr_amd.h; what the two classes do around them (input check, anchor sets, the head's anchor
order, the four outputs) is _Assigner, so each assign_targets is its workspace query and its call loop."""
import torch

from . import kernels


class _Assigner:
    """What both assigners do around their entry point: the input check, the anchor sets, the head's anchor order and the outputs."""

    _flat = None

    def _anchor_sets(self, all_anchors, device):
        """Every anchor set as a contiguous (n, 7) device tensor + its per-location count, kept between calls."""
        key = (tuple(a.data_ptr() for a in all_anchors), device)
        if self._flat is None or self._flat[0] != key:
            sets = []
            for a in all_anchors:
                assert a.shape[-1] == 7 and a.shape[0] == 1, "hvpr path: one anchor height, 7 box parameters"
                per_loc = int(a.shape[3] * a.shape[4])
                sets.append((a.reshape(-1, 7).to(device=device, dtype=torch.float32).contiguous(), per_loc))
            self._flat = (key, sets)
        return self._flat[1]

    def _prepare(self, all_anchors, gt):
        """(gt contiguous, anchor sets, anchors per location over all sets, anchors in all, the dict of the four outputs)"""
        if not gt.is_cuda or gt.dtype != torch.float32:
            raise RuntimeError("hvpr_amd: the target assigner needs fp32 GPU tensors (the HIP path has no CPU fallback)")
        gt = gt.contiguous()
        B = int(gt.shape[0])
        sets = self._anchor_sets(all_anchors, gt.device)
        stride = sum(p for _, p in sets)
        n_loc = sets[0][0].shape[0] // sets[0][1]
        assert all(a.shape[0] // p == n_loc for a, p in sets), "every anchor set covers the same feature map"
        A = n_loc * stride
        out = {"box_cls_labels": torch.empty((B, A), dtype=torch.int32, device=gt.device),
               "box_reg_targets": torch.empty((B, A, self.box_coder.code_size), dtype=torch.float32, device=gt.device),
               "reg_weights": torch.empty((B, A), dtype=torch.float32, device=gt.device),
               "positives_per_frame": torch.zeros((B,), dtype=torch.int32, device=gt.device)}
        return gt, sets, stride, A, out


class AxisAlignedTargetAssigner(_Assigner):
    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        acfg = model_cfg.ANCHOR_GENERATOR_CONFIG
        tcfg = model_cfg.TARGET_ASSIGNER_CONFIG
        assert tcfg.POS_FRACTION < 0, "hvpr path: no fg/bg sampling (hvpr.yaml:122)"
        self.box_coder = box_coder
        self.class_names = list(class_names)
        self.anchor_class_names = [c["class_name"] for c in acfg]
        self.matched = {c["class_name"]: c["matched_threshold"] for c in acfg}
        self.unmatched = {c["class_name"]: c["unmatched_threshold"] for c in acfg}
        self.norm_by_num_examples = bool(tcfg.NORM_BY_NUM_EXAMPLES)
        self.match_height = bool(match_height)

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """all_anchors: list of (nz,ny,nx,S,R,7); gt (B,G,8).  Returns box_cls_labels (B,A) i32, box_reg_targets (B,A,7),
        reg_weights (B,A) and positives_per_frame (B,) i32, anchors ordered (z,y,x,class,size,rot) as the single head predicts them."""
        gt, sets, stride, A, out = self._prepare(all_anchors, gt_boxes_with_classes)
        B, G = int(gt.shape[0]), int(gt.shape[1])
        L = kernels.lib()
        ex = self.match_height or self.norm_by_num_examples
        if ex:
            need = max(int(L.hvpr_assign_targets_ex_workspace_bytes(B, G, a.shape[0], int(self.match_height))) for a, _ in sets)
        else:
            need = int(L.hvpr_assign_targets_workspace_bytes(B, G))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=gt.device)
        off = 0
        for cname, (a, per_loc) in zip(self.anchor_class_names, sets):
            args = (a, a.shape[0], gt, B, G, self.class_names.index(cname), len(self.class_names), float(self.matched[cname]),
                    float(self.unmatched[cname]), per_loc, stride, off, A, out["box_cls_labels"], out["box_reg_targets"],
                    out["reg_weights"], out["positives_per_frame"])
            if ex:
                kernels.call("hvpr_assign_targets_ex_f32", *args, int(self.match_height), int(self.norm_by_num_examples), ws, ws.numel(),
                             kernels._stream())
            else:
                kernels.call("hvpr_assign_targets_f32", *args, ws, ws.numel(), kernels._stream())
            off += per_loc
        return out


class ATSSTargetAssigner(_Assigner):
    """TARGET_ASSIGNER_CONFIG.NAME: ATSS (pcdet/models/dense_heads/target_assigner/atss_target_assigner.py:7-141) through
    hvpr_assign_targets_atss_f32: per anchor set seven launches for the whole batch, no (N, M) table and no host read
    (the reference trims padded rows with a host read per row and builds dense IoU and distance tables per frame).  Every ground
    truth of every class is matched against every anchor set, as in the reference; labels are int32 with no -1 band; several
    anchor sets come back in the head's order, not set after set.  CPU tensors raise."""

    def __init__(self, topk, box_coder, match_height=False, n_classes=None):
        """n_classes: class values outside 0 .. n_classes label an anchor 0 (the head passes its class count; None: 0 .. 255)."""
        if not 1 <= int(topk) <= 64:
            raise ValueError(f"hvpr_amd: ATSS TOPK must be 1 .. 64, got {topk}")
        self.topk = int(topk)
        self.box_coder = box_coder
        self.match_height = bool(match_height)
        self.n_classes = 255 if n_classes is None else int(n_classes)

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """all_anchors: list of (nz,ny,nx,S,R,7); gt (B,G,8).  The four keys of AxisAlignedTargetAssigner.assign_targets."""
        gt, sets, stride, A, out = self._prepare(all_anchors, gt_boxes_with_classes)
        B, G = int(gt.shape[0]), int(gt.shape[1])
        L = kernels.lib()
        need = max(int(L.hvpr_assign_targets_atss_workspace_bytes(B, G, a.shape[0], self.topk)) for a, _ in sets)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=gt.device)
        off = 0
        rows = gt if G else gt.new_zeros((B, 1, 8))        # G == 0: an empty tensor has no address to pass; n_gt 0 reads no row
        for a, per_loc in sets:
            kernels.call("hvpr_assign_targets_atss_f32", a, a.shape[0], rows, B, G, self.n_classes, self.topk, int(self.match_height), per_loc,
                         stride, off, A, out["box_cls_labels"], out["box_reg_targets"], out["reg_weights"], out["positives_per_frame"],
                         ws, ws.numel(), kernels._stream())
            off += per_loc
        return out
