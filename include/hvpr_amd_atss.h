/*
 * hvpr_amd — the ATSS target assigner, entry points added to ABI version 8.
 *
 * include/hvpr_amd.h and include/hvpr_amd_ext.h are pinned name by name by the test suite; a further compatible addition — new
 * symbols, no existing signature touched, hvpr_abi_version() still 8 — gets a header of its own, under the same conventions
 * (plain device pointers, a stream, no allocation, no host read, a negative hvpr_status on refusal with every output untouched).
 * hvpr_amd/_lib.py derives the ctypes signatures from this file exactly as it does from the other two.
 */
#ifndef HVPR_AMD_ATSS_H
#define HVPR_AMD_ATSS_H

#include "hvpr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * a12 (training)  TARGET_ASSIGNER_CONFIG.NAME: ATSS — ATSSTargetAssigner.assign_targets for one anchor set and a whole batch
 *     (pcdet/models/dense_heads/target_assigner/atss_target_assigner.py:16-141), written in the head's anchor order like
 *     hvpr_assign_targets_f32: output row (a / per_loc) * loc_stride + loc_offset + a % per_loc of anchors_total, each exactly once.
 *     anchors (n_anchors, 7), gt_boxes (batch, n_gt, 8) with the class in column 7.  Per frame:
 *       - trailing rows whose signed fp32 sum over the 7 box columns is 0 are cut, row 0 never is; NO class mask: every remaining
 *         row of every class takes part;
 *       - the IoU of (anchor, ground truth) is the bits of hvpr_boxes_pairwise_f32 mode 1 (match_height 0) or mode 2 (non-zero);
 *       - candidates of a ground truth: the topk anchors with the smallest 64-bit key (bits of the fp32 squared centre distance
 *         (dx*dx + dy*dy) + dz*dz, then anchor index); thresh = float(mean) + float(std) + 1e-6f of their IoUs, mean and unbiased
 *         variance summed in float64 in key order (topk 1: NaN, nothing positive); a candidate is positive when iou >= thresh
 *         and its centre passes the reference's inside test (rotate by -heading, x against dy / 2, y against dx / 2, closed);
 *       - an anchor takes the ground truth of its highest positive IoU, the lowest row on ties;
 *       - then every ground truth, in ascending order, takes the anchor of its maximum IoU over ALL anchors (lowest index on ties,
 *         anchor 0 where the maximum is 0): no `> 0` guard, the highest row wins a shared anchor;
 *       - labels = class of the matched row (int32; 0 for an unmatched anchor and for a class outside 0 .. n_classes), no -1 band;
 *         reg_targets = ResidualCoder.encode_torch where label > 0, zero elsewhere; reg_weights = 1 / 0; pos_count[frame] +=
 *         #(label > 0) (the caller zeroes it).
 *     n_gt == 0 writes background.  Limits: 1 <= topk <= 64, topk <= n_anchors, n_gt <= 256.  Integer atomics only: the same bytes
 *     on every run; capturable.  workspace: hvpr_assign_targets_atss_workspace_bytes(batch, n_gt, n_anchors, topk) bytes (0 for
 *     arguments the call would refuse).
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_assign_targets_atss_workspace_bytes(int batch, int n_gt, int n_anchors, int topk);
int hvpr_assign_targets_atss_f32(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int n_classes,
                                 int topk, int match_height, int per_loc, int loc_stride, int loc_offset, long long anchors_total,
                                 int32_t *labels, float *reg_targets, float *reg_weights, int32_t *pos_count,
                                 void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HVPR_AMD_ATSS_H */
