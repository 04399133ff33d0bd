// f5 — the evaluation epilogue on the device: what lies between post_processing(sync=False) and the AP tables of kitti_ap.hip.
//   hvpr_recall_record_f32     Detector3DTemplate.generate_recall_record (detector3d_template.py:276-318) for all frames of a batch
//   hvpr_prediction_annos_f32  KittiDataset.generate_prediction_dicts (kitti_dataset.py:246-320, box_utils.py:152-235) for a batch,
//                              written compactly into the annotation tables hvpr_kitti_* read (rows of kRow doubles)
// Neither reads anything back: live counts arrive as device words, results stay on the device.  Built with -ffp-contract=off: the
// 3-D IoU is the fp32 sequence of the pairwise table (iou_geom.h), so the recalled counts are those of the host loop.
#include "common.h"
#include "iou_geom.h"

namespace {

constexpr int kMaxThresh = 8, kMaxLabels = 16, kRow = 16, kCalib = 26;

// ---- recall ------------------------------------------------------------------------------------------------------------------
struct Thresholds { float v[kMaxThresh]; };

// One wave per frame: the reference's trim of the padded ground-truth table.  A row is empty when the left-to-right fp32 sum of its
// C columns is 0; trailing empty rows are cut by `while k > 0`, so row 0 always stays.  counts[b] = {ground truths, 0 ... 0}.
__global__ void __launch_bounds__(64) k_gt_count(const float *__restrict__ gt, int G, int C, int T, int32_t *__restrict__ counts) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *__restrict__ g = gt + (size_t)b * G * C;
    int last = 0;
    for (int r = lane; r < G; r += 64) {
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s += g[(size_t)r * C + c];
        if (!(s == 0.0f)) last = r;                       // rising r: the lane's last non-empty row
    }
    HVPR_WAVE_MAX_XOR(last);
    if (lane <= T) counts[(size_t)b * (1 + T) + lane] = lane == 0 ? (G > 0 ? last + 1 : 0) : 0;
}

// One wave per (frame, ground truth).  The lanes stride over the frame's live predictions, each with its PolyStore slot as in
// k_pairwise; the best IoU is reduced inside the wave (DPP, no LDS round trip), and lane 0 adds 1 per passed threshold.
__global__ void __launch_bounds__(64) k_recall(const float *__restrict__ pred, const int32_t *__restrict__ pred_count, int P,
                                               const float *__restrict__ gt, int G, int C, const Thresholds thr, int T,
                                               int32_t *__restrict__ counts, float *__restrict__ best_iou) {
    __shared__ PolyStore ps;
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    int32_t *__restrict__ cnt = counts + (size_t)b * (1 + T);
    const int n_gt = cnt[0];                              // written by k_gt_count, the launch before this one
    if (g >= n_gt) {
        if (best_iou && lane == 0) best_iou[(size_t)b * G + g] = 0.0f;
        return;
    }
    const int n = P > 0 ? min(max(pred_count[b], 0), P) : 0;
    const float *__restrict__ pg = gt + ((size_t)b * G + g) * C;
    Box Bg;
    make_box(pg, Bg);
    float best = 0.0f;                                    // an IoU is never negative
    for (int j = lane; j < n; j += 64) {
        const float *__restrict__ pp = pred + ((size_t)b * P + j) * 7;
        Box A;
        make_box(pp, A);
        best = fmaxf(best, iou_3d(pp, pg, A, Bg, ps, lane));
    }
    best = hvpr_reduce_max<64>(best);
    if (lane == 0) {
        if (best_iou) best_iou[(size_t)b * G + g] = best;
        if (n > 0)
            for (int t = 0; t < T; ++t)
                if (best > thr.v[t]) atomicAdd(&cnt[1 + t], 1);
    }
}

// ---- annotations -------------------------------------------------------------------------------------------------------------
struct LabelMap { int32_t cls[kMaxLabels]; };

struct AnnoArgs {
    const float *boxes, *scores;
    const int64_t *labels;
    const int32_t *count;
    const float *calib;
    int B, P, n_labels, frame_base;
    LabelMap map;
    const int64_t *row_base;
    long long cap;
    double *dt_rows;
    int32_t *dt_cls, *dt_label;
    float *dt_box7, *boxes_lidar;
    int64_t *dt_off;
    int32_t *overflow;
};

__device__ __forceinline__ int live_of(const int32_t *count, int b, int P) { return P > 0 ? min(max(count[b], 0), P) : 0; }

// Block (x, b): 64 boxes of frame b, one lane per box.  Every block sums the live counts of the frames before b (B is a batch: a few
// lanes' worth), so frame b's rows follow frame b - 1's with no gap; block (0, b) records where frame b ends in dt_off.
__global__ void __launch_bounds__(64) k_prediction_annos(const AnnoArgs a) {
    const int b = blockIdx.y, lane = threadIdx.x;
    int before = 0;
    for (int i = lane; i < b; i += 64) before += live_of(a.count, i, a.P);
    HVPR_WAVE_SUM_XOR(before);
    const int n = live_of(a.count, b, a.P);
    const long long first = a.row_base[0] + before;
    if (blockIdx.x == 0 && lane == 0) {
        a.dt_off[a.frame_base + b + 1] = min(first + n, a.cap);
        if (first + n > a.cap) *a.overflow = 1;
    }
    const int j = blockIdx.x * 64 + lane;
    const long long r = first + j;
    if (j >= n || r >= a.cap) return;

    const float *__restrict__ p = a.boxes + ((size_t)b * a.P + j) * 7;
    const float *__restrict__ M = a.calib + (size_t)b * kCalib, *__restrict__ P2 = M + 12;
    const float img_h = M[24], img_w = M[25];
    const float x = p[0], y = p[1], l = p[3], w = p[4], h = p[5];
    const float zb = p[2] - h / 2;                                              // box_utils.py:162
    float loc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) loc[k] = x * M[k] + y * M[3 + k] + zb * M[6 + k] + M[9 + k];     // calibration_kitti.py:70-71
    const float ry = -p[6] - 1.57079632679489661923f;                           // box_utils.py:165
    const float c = cosf(ry), s = sinf(ry);
    const float hx = l / 2, hz = w / 2;
    float u0 = 0.f, v0 = 0.f, u1 = 0.f, v1 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                               // box_utils.py:184-208
        const float xc = (k & 2) ? -hx : hx, zc = ((k + 1) & 2) ? -hz : hz, yc = (k & 4) ? -h : 0.0f;
        const float cx = loc[0] + (xc * c + zc * s), cy = loc[1] + yc, cz = loc[2] + (xc * (-s) + zc * c);
        const float u = (cx * P2[0] + cy * P2[1] + cz * P2[2] + P2[3]) / cz;    // calibration_kitti.py:80-82: by the rect depth
        const float v = (cx * P2[4] + cy * P2[5] + cz * P2[6] + P2[7]) / cz;
        u0 = k ? fminf(u0, u) : u; u1 = k ? fmaxf(u1, u) : u;
        v0 = k ? fminf(v0, v) : v; v1 = k ? fmaxf(v1, v) : v;
    }
    const float wmax = img_w - 1.0f, hmax = img_h - 1.0f;                       // box_utils.py:229-233
    u0 = fminf(fmaxf(u0, 0.0f), wmax); u1 = fminf(fmaxf(u1, 0.0f), wmax);
    v0 = fminf(fmaxf(v0, 0.0f), hmax); v1 = fminf(fmaxf(v1, 0.0f), hmax);
    const float alpha = -atan2f(-y, x) + ry;                                    // kitti_dataset.py:287

    double *__restrict__ d = a.dt_rows + (size_t)r * kRow;
    d[0] = u0; d[1] = v0; d[2] = u1; d[3] = v1; d[4] = alpha;
    d[5] = loc[0]; d[6] = loc[1]; d[7] = loc[2];
    d[8] = l; d[9] = h; d[10] = w; d[11] = ry;
    d[12] = 0.0; d[13] = 0.0; d[14] = a.scores[(size_t)b * a.P + j]; d[15] = 0.0;
    const long long lab = a.labels[(size_t)b * a.P + j];
    a.dt_label[r] = (int32_t)lab;
    a.dt_cls[r] = (lab >= 1 && lab <= a.n_labels) ? a.map.cls[lab - 1] : -1;
    float *__restrict__ t = a.dt_box7 + (size_t)r * 7;                          // kitti_eval_device._as7
    t[0] = loc[0]; t[1] = loc[2]; t[2] = 0.0f; t[3] = l; t[4] = w; t[5] = 1.0f; t[6] = -ry;
    float *__restrict__ q = a.boxes_lidar + (size_t)r * 7;                      // the reference lowers z of the array it returns
    q[0] = x; q[1] = y; q[2] = zb; q[3] = l; q[4] = w; q[5] = h; q[6] = p[6];
}

// After k_prediction_annos, on the same stream: row_base += the batch's live rows (never past cap).
__global__ void __launch_bounds__(64) k_advance_rows(const int32_t *__restrict__ count, int B, int P, long long cap,
                                                     int64_t *__restrict__ row_base) {
    const int lane = threadIdx.x;
    int total = 0;
    for (int i = lane; i < B; i += 64) total += live_of(count, i, P);
    HVPR_WAVE_SUM_XOR(total);
    if (lane == 0) row_base[0] = min(row_base[0] + total, cap);
}

}  // namespace

extern "C" int hvpr_recall_record_f32(const float *pred_boxes, const int32_t *pred_count, int B, int P, const float *gt_boxes, int G,
                                      int C, const float *thresholds, int T, int32_t *counts, float *best_iou,
                                      hvpr_stream_t stream) {
    if (B < 0 || P < 0 || G < 0 || T < 0 || (G > 0 && C < 7)) return HVPR_ERR_INVALID_ARG;
    if (T > kMaxThresh || B > 65535 || (long long)B * P > (1ll << 30) || (long long)B * G * (long long)(C > 1 ? C : 1) > (1ll << 30))
        return HVPR_ERR_UNSUPPORTED;
    if (B == 0) return HVPR_OK;
    if (!counts || (T > 0 && !thresholds) || (G > 0 && !gt_boxes) || (G > 0 && P > 0 && (!pred_boxes || !pred_count)))
        return HVPR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (G == 0) {                                          // nothing to count: no launch over an empty grid
        if (hipMemsetAsync(counts, 0, (size_t)B * (1 + T) * sizeof(int32_t), s) != hipSuccess) return HVPR_ERR_LAUNCH;
        return HVPR_OK;
    }
    Thresholds thr;
    for (int t = 0; t < kMaxThresh; ++t) thr.v[t] = t < T ? thresholds[t] : 0.0f;
    hipLaunchKernelGGL(k_gt_count, dim3(B), dim3(64), 0, s, gt_boxes, G, C, T, counts);
    HVPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_recall, dim3(G, B), dim3(64), 0, s, pred_boxes, pred_count, P, gt_boxes, G, C, thr, T, counts, best_iou);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_prediction_annos_f32(const float *pred_boxes, const float *pred_scores, const int64_t *pred_labels,
                                         const int32_t *pred_count, int B, int P, const float *calib,
                                         const int32_t *class_of_label, int n_labels, int64_t *row_base, long long cap,
                                         int frame_base, int max_frames, double *dt_rows, int32_t *dt_cls, int32_t *dt_label,
                                         float *dt_box7, float *boxes_lidar, int64_t *dt_off, int32_t *overflow,
                                         hvpr_stream_t stream) {
    if (B < 0 || P < 0 || n_labels < 0 || cap < 0 || frame_base < 0 || max_frames < 0) return HVPR_ERR_INVALID_ARG;
    if (n_labels > kMaxLabels || B > 65535 || (long long)B * P > (1ll << 30) || cap >= (1ll << 31)) return HVPR_ERR_UNSUPPORTED;
    if ((long long)frame_base + B > max_frames) return HVPR_ERR_INVALID_ARG;             // dt_off holds max_frames + 1 words
    if (B == 0) return HVPR_OK;
    if (!pred_count || !row_base || !dt_off || !overflow || (n_labels > 0 && !class_of_label)) return HVPR_ERR_INVALID_ARG;
    if (P > 0 && (!pred_boxes || !pred_scores || !pred_labels || !calib)) return HVPR_ERR_INVALID_ARG;
    if (P > 0 && cap > 0 && (!dt_rows || !dt_cls || !dt_label || !dt_box7 || !boxes_lidar)) return HVPR_ERR_INVALID_ARG;
    AnnoArgs a;
    a.boxes = pred_boxes; a.scores = pred_scores; a.labels = pred_labels; a.count = pred_count; a.calib = calib;
    a.B = B; a.P = P; a.n_labels = n_labels; a.frame_base = frame_base;
    for (int i = 0; i < kMaxLabels; ++i) a.map.cls[i] = i < n_labels ? class_of_label[i] : -1;
    a.row_base = row_base; a.cap = cap;
    a.dt_rows = dt_rows; a.dt_cls = dt_cls; a.dt_label = dt_label; a.dt_box7 = dt_box7; a.boxes_lidar = boxes_lidar;
    a.dt_off = dt_off; a.overflow = overflow;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_prediction_annos, dim3(P > 0 ? hvpr_cdiv(P, 64) : 1, B), dim3(64), 0, s, a);   // P == 0 still records dt_off
    HVPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_advance_rows, dim3(1), dim3(64), 0, s, pred_count, B, P, cap, row_base);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
