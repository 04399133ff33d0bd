// What the two target assigners share (assign_loss.hip: axis-aligned and MATCH_HEIGHT; assign_atss.hip: ATSS).  ONE copy: labels,
// weights and counts of both are compared exactly with the reference's (tests/golden G8, G16, G18, G26, G27), so a fix to the trim,
// the box code, the head's order or the sweep has to reach every kernel that uses it.  Both files are compiled with
// -ffp-contract=off (hvpr_amd/build.py), like every file that includes iou_geom.h.
#pragma once
#include "common.h"
#include "iou_geom.h"

namespace {

constexpr int kMaxGt = 256;          // ground-truth rows per frame (hvpr.yaml pads to ~50); a ring entry keeps the row in 8 bits
constexpr int kSweepRing = 128;      // pairs; a step adds at most 64 to fewer than 64

// The last row of a frame that is no padding: trailing rows whose SIGNED fp32 sum over the 7 box fields, class column excluded, is
// exactly 0 are cut, row 0 always stays (`while cnt > 0 and cur_gt[cnt].sum() == 0`, axis_aligned_target_assigner.py:53-57,
// atss_target_assigner.py:40-46).  Every thread of the workgroup calls it, whatever the block size; s_last is one int of LDS.
__device__ __forceinline__ int last_real_row(const float *gt_frame, int G, int *s_last) {
    const int step = blockDim.x;
    if (threadIdx.x == 0) *s_last = 0;
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += step) {
        const float *p = gt_frame + (size_t)g * 8;
        float sum = 0.f;
        for (int j = 0; j < 7; ++j) sum += p[j];                  // left to right, as written (contraction is off)
        if (sum != 0.f) atomicMax(s_last, g);
    }
    __syncthreads();
    return *s_last;
}

// a row of class value c belongs to the anchor set of class_index (axis_aligned_target_assigner.py:62-66; python's class_names[c - 1]:
// class 0 wraps to the last class)
__device__ __forceinline__ bool of_class(int c, int class_index, int n_classes) {
    int m = (c - 1) % n_classes;
    if (m < 0) m += n_classes;
    return m == class_index;
}

// ResidualCoder.encode_torch, box_coder_utils.py:13-43, of the ground-truth row gp against the anchor row an
__device__ __forceinline__ void encode_residual(const float *an, const float *gp, float t[7]) {
    const float dxa = fmaxf(an[3], 1e-5f), dya = fmaxf(an[4], 1e-5f), dza = fmaxf(an[5], 1e-5f);
    const float dxg = fmaxf(gp[3], 1e-5f), dyg = fmaxf(gp[4], 1e-5f), dzg = fmaxf(gp[5], 1e-5f);
    const float diag = sqrtf(dxa * dxa + dya * dya);
    t[0] = (gp[0] - an[0]) / diag;
    t[1] = (gp[1] - an[1]) / diag;
    t[2] = (gp[2] - an[2]) / dza;
    t[3] = logf(dxg / dxa);
    t[4] = logf(dyg / dya);
    t[5] = logf(dzg / dza);
    t[6] = gp[6] - an[6];
}

// anchor a of a set in the head's anchor order: per_loc of the set at each location, loc_stride anchors per location over all sets
__device__ __forceinline__ long long head_row(int a, int per_loc, int loc_stride, int loc_offset) {
    return (long long)(a / per_loc) * loc_stride + loc_offset + (a % per_loc);
}

// The sweep of the kernels that need a rotated IoU against a whole table.  The polygon clip costs ~18 k cycles and is data dependent,
// the two exact rejects cost ~50 flops and leave a few hundred anchors per ground truth, so a workgroup is ONE wave that sweeps its 64
// anchors (al: this lane's, valid: it exists) over the rows gl_rows[0 .. n) with the rejects only and packs the surviving (anchor, g)
// pairs by ballot and prefix count into ring[kSweepRing] in LDS, (anchor in workgroup) << 8 | g; whenever the ring holds 64 pairs,
// clip(head, 64) clips them, one pair per lane — so every clipping round but the last has 64 live lanes, and no wave clips for one
// live lane.  use(g), workgroup-uniform, says whether row g takes part.  A rejected pair is IoU exactly +0, what box_overlap would have
// returned; a caller that ranks those too (k_assign3d<2>: the first maximum over g) gets the lane's first rejected row back — a
// result and no callback: a caller's variable updated from a lambda cost the loop over the whole table a branch per row.
struct Swept {
    int clipped;         // pairs that reached the clip, over the workgroup
    int first_miss;      // this lane's first row in use whose pair was rejected, -1: none
};

template <class Use, class Clip>
__device__ __forceinline__ Swept sweep_pairs(unsigned short *ring, const BoxLite *gl_rows, int n, const BoxLite &al, bool valid, Use use,
                                             Clip clip) {
    const int lane = threadIdx.x;
    int head = 0, tail = 0, first_miss = -1;
    for (int g = 0; g < n; ++g) {
        if (!use(g)) continue;
        const BoxLite gl = gl_rows[g];
        const bool near = valid && !far_apart(al, gl);
        bool live = false;
        if (__ballot(near)) live = near && !axes_separate(al, gl);       // most rows are out of every lane's reach
        if (valid && !live && first_miss < 0) first_miss = g;
        const unsigned long long m = __ballot(live);
        if (!m) continue;                                                 // the workgroup is one wave: uniform
        if (live) ring[(tail + __popcll(m & ((1ull << lane) - 1ull))) & (kSweepRing - 1)] = (unsigned short)((lane << 8) | g);
        tail += __popcll(m);
        __syncthreads();
        if (tail - head >= 64) {
            clip(head, 64);
            head += 64;
            __syncthreads();                                              // the round's ring slots are free again
        }
    }
    if (tail > head) clip(head, tail - head);
    __syncthreads();
    return Swept{tail, first_miss};
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// the arguments every assigner entry point takes: HVPR_ERR_INVALID_ARG where one is missing or the head's order does not hold
// together.  ATSS has no class mask and passes class_index 0.
inline int assign_args_status(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int class_index,
                              int n_classes, int per_loc, int loc_stride, int loc_offset, long long anchors_total, const int32_t *labels,
                              const float *reg_targets, const float *reg_weights, const int32_t *pos_count, const void *workspace) {
    if (!anchors || !gt_boxes || !labels || !reg_targets || !reg_weights || !pos_count || !workspace) return HVPR_ERR_INVALID_ARG;
    if (n_anchors < 1 || batch < 1 || n_gt < 0 || n_classes < 1 || class_index < 0 || class_index >= n_classes || per_loc < 1 ||
        n_anchors % per_loc != 0 || loc_stride < per_loc || loc_offset < 0 || loc_offset + per_loc > loc_stride ||
        anchors_total < (long long)(n_anchors / per_loc) * loc_stride)
        return HVPR_ERR_INVALID_ARG;
    return HVPR_OK;
}

}  // namespace
