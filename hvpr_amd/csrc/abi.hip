// ABI bookkeeping for libhvpr_amd.so (include/hvpr_amd.h).
#include "common.h"

// 2: packed memory bank (bank_packed argument); 3: bank_packed is required and holds IEEE fp16 tiles (v_mfma_f32_16x16x32_f16) +
// channel maxima; 4: the packed bank ends in 128 floats (64 channel maxima, their sum and maximum: hvpr_memory_bank_packed_floats grew
// by 64) and the voxelizer workspace holds the one-launch index kernel's per-cell words and barrier flags (hvpr_voxelize_workspace_bytes
// grew) — a caller that sized either buffer with a version-3 formula is too small: always size them with the two functions; 5: adds
// hvpr_bn_train_affine_f32 and hvpr_bn_relu_fwd / bwd_slice_nhwc_f32; hvpr_conv2d_wino_wgrad_nhwc_f32 answers HVPR_ERR_UNSUPPORTED for images of 2 GB and more (32-bit offsets
// inside an image; its workspace size is unchanged); 6: hvpr_encode_fwd_f32 takes index_mode (the one-launch index kernel is opt-in and guarded),
// hvpr_voxelize_workspace_status, HVPR_ERR_TIMEOUT; 7: hvpr_bn_relu_fwd_nhwc_f32 takes y_cstride / y_coff and hvpr_bn_relu_bwd_sums /
// _apply_nhwc_f32 take dy_cstride / dy_coff (a channel slice of a wider tensor); hvpr_bn_relu_fwd / bwd_slice_nhwc_f32, hvpr_bn_relu_bwd_nhwc_f32
// (= _sums then _apply), hvpr_group_rows_grad_f32 and hvpr_fp_rows_grad_f32 are gone.  Later within 7 (no signature changed):
// hvpr_nms_workspace_bytes grows with n_max (past 4096 it also reserves the two-launch mask's segments, ~17 MB more), so a
// workspace serves every smaller n_max; the hvpr_score_topk_f32 workspace keeps its zeroed state in front of the keys, and calls
// that share one pass the same batch; -0.0 scores rank as +0.0; hvpr_attend_rows_fwd_f32 is added (csrc/attend_rows.hip); 8:
// hvpr_group_points_grad_f32, hvpr_three_interpolate_grad_f32 and hvpr_scatter_add_rows_f32 (float atomics) are gone: every scattering
// gradient is hvpr_segment_sum_rows_f32 over a plan of its edges.  Later within 8 (no signature changed): hvpr_fused_adam_l2_f32 and
// hvpr_fused_sgd_f32 are added (csrc/train_ops.hip); hvpr_assign_targets_ex_f32 and hvpr_assign_targets_ex_workspace_bytes are added
// (csrc/assign_loss.hip: MATCH_HEIGHT and NORM_BY_NUM_EXAMPLES of the target assigner); hvpr_assign_targets_atss_f32 and
// hvpr_assign_targets_atss_workspace_bytes are added (csrc/assign_atss.hip: NAME: ATSS); hvpr_pillar_vfe_plain_fwd_f32 is added within 8
// (csrc/vfe_plain.hip: the one-layer pillar encoder of plain PointPillars)
extern "C" int hvpr_abi_version(void) { return 8; }

extern "C" const char *hvpr_status_string(int status) {
    switch (status) {
        case HVPR_OK: return "ok";
        case HVPR_ERR_INVALID_ARG: return "invalid argument";
        case HVPR_ERR_UNSUPPORTED: return "unsupported shape for this build of the kernels";
        case HVPR_ERR_WORKSPACE: return "workspace too small";
        case HVPR_ERR_LAUNCH: return "HIP launch failed";
        case HVPR_ERR_TIMEOUT: return "a one-launch index kernel gave up a wait: reset the voxelizer workspace";
        default: return "unknown status";
    }
}

// SyncBatchNorm hook (include/hvpr_amd.h): the only state this library keeps between calls
namespace { hvpr_allreduce_fn g_bn_allreduce = nullptr; void *g_bn_allreduce_ctx = nullptr; }

extern "C" void hvpr_set_batchnorm_allreduce(hvpr_allreduce_fn fn, void *ctx) { g_bn_allreduce = fn; g_bn_allreduce_ctx = ctx; }

int hvpr_i_bn_allreduce(double *buf, int n, hipStream_t s) {
    if (!g_bn_allreduce) return 0;
    return g_bn_allreduce(buf, n, (hvpr_stream_t)s, g_bn_allreduce_ctx);
}
