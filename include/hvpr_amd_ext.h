/*
 * hvpr_amd — entry points added to ABI version 8 after include/hvpr_amd.h was pinned.
 *
 * hvpr_amd.h is the surface tests/test_capi_symbols.py pins parameter by parameter (names, kinds and their number); a compatible
 * addition — a new symbol, no existing signature touched, hvpr_abi_version() still 8 — is declared here instead, under the same
 * conventions (plain device pointers, a stream, no allocation, a negative hvpr_status on refusal with every output untouched), and
 * hvpr_amd/_lib.py derives its ctypes signatures from this file exactly as it does from hvpr_amd.h.
 */
#ifndef HVPR_AMD_EXT_H
#define HVPR_AMD_EXT_H

#include "hvpr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * a12 (training)  hvpr_assign_targets_f32 with the two remaining switches of TARGET_ASSIGNER_CONFIG
 *     (pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:113-213); every argument up to pos_count, the
 *     trim of padded rows, the class mask, the first maximum over the ground truths, the forced matches, the box code and the
 *     head's anchor order are those of hvpr_assign_targets_f32 (hvpr_amd.h, a12).
 *     match_height          0: boxes3d_nearest_bev_iou, the kernels of hvpr_assign_targets_f32.  non-zero: MATCH_HEIGHT True (:145) —
 *                           the table entry of (anchor, ground truth) is the rotated 3-D IoU, bit for bit what
 *                           hvpr_boxes_pairwise_f32 mode 2 gives for the two rows (the reference's absent native
 *                           boxes_iou3d_gpu).  Two launches: exact rejects on the whole table, the polygon clip on densely packed
 *                           survivors only, once per pass with the same bits; integer atomics only, so labels, targets and
 *                           counts are the same bits on every run.
 *     norm_by_num_examples  non-zero: NORM_BY_NUM_EXAMPLES True (:201-204) — per frame and anchor set n = #(labels >= 0) and
 *                           reg_weights = 1 / max(n, 1) (fp32) on the positives, two small launches more, no host read.  labels,
 *                           reg_targets and pos_count do not depend on it.  The head's losses do not consume reg_weights: they
 *                           rebuild their weights from the labels (anchor_head_template.py:113-119, 190-192), so this flag only
 *                           changes the returned tensor, in the reference as here.
 *     Both 0: the call IS hvpr_assign_targets_f32 (same launches, same bits).  n_gt <= 256; POS_FRACTION sampling is not built.
 *     workspace: hvpr_assign_targets_ex_workspace_bytes(batch, n_gt, n_anchors, match_height) bytes (>= what
 *     hvpr_assign_targets_f32 asks).  After a match_height call its first 8 bytes hold, as one uint64, the number of (anchor,
 *     ground truth) pairs that passed the rejects and were clipped, counted once (pass 1), summed over the frames.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_assign_targets_ex_workspace_bytes(int batch, int n_gt, int n_anchors, int match_height);
int hvpr_assign_targets_ex_f32(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int class_index,
                               int n_classes, float matched_thr, float unmatched_thr, int per_loc, int loc_stride, int loc_offset,
                               long long anchors_total, int32_t *labels, float *reg_targets, float *reg_weights, int32_t *pos_count,
                               int match_height, int norm_by_num_examples, void *workspace, size_t workspace_bytes,
                               hvpr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HVPR_AMD_EXT_H */
