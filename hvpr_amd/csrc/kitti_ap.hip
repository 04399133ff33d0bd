// f3 on the device — the KITTI AP evaluator's per-frame work (hvpr_amd/kitti_eval.py: frame_overlap, clean_data, _match,
// _frame_stats) over ALL frames of a split in a fixed number of launches.  The host evaluator stays the yardstick: every number
// that decides a comparison here is a double formed in the order of the numpy expression it restates, and this file is built with
// -ffp-contract=off, so overlaps are bit-equal and the integer counts equal.
//
// Annotation rows are kRow doubles: bbox[4], alpha, location[3], dimensions[3], rotation_y, occluded, truncated, score, pad
// (hvpr_amd/kitti_eval_device.py: AnnoTables).  Frame f owns ground truths gt_off[f] .. gt_off[f + 1), detections likewise, and
// the nd_f x ng_f overlaps at pair_off[f] (detection-major, the `overlaps[j, i]` orientation of the host).
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kRow = 16;
enum { kAlpha = 4, kLoc = 5, kDim = 8, kOcc = 12, kTrunc = 13, kScore = 14 };
constexpr int kMaxClasses = 8, kMaxSets = 4;

// ---- overlaps ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kitti_overlaps(const double *__restrict__ gt, const double *__restrict__ dt,
                                                        const float *__restrict__ inter, const int64_t *__restrict__ gt_off,
                                                        const int64_t *__restrict__ dt_off, const int64_t *__restrict__ pair_off,
                                                        int n_frames, long long n_pairs, int metric, double *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    int lo = 0, hi = n_frames;                           // the largest f with pair_off[f] <= p
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= p) lo = mid; else hi = mid;
    }
    const long long ng = gt_off[lo + 1] - gt_off[lo], r = p - pair_off[lo];
    const double *d = dt + (size_t)(dt_off[lo] + r / ng) * kRow, *g = gt + (size_t)(gt_off[lo] + r % ng) * kRow;
    double res;
    if (metric == 0) {                                   // image_box_overlap(dt, gt, -1)
        const double iw = fmin(d[2], g[2]) - fmax(d[0], g[0]), ih = fmin(d[3], g[3]) - fmax(d[1], g[1]);
        const double in = (iw > 0 && ih > 0) ? iw * ih : 0.0;
        const double area_d = (d[2] - d[0]) * (d[3] - d[1]), area_g = (g[2] - g[0]) * (g[3] - g[1]);
        res = in > 0 ? in / ((area_d + area_g) - in) : 0.0;
    } else {
        const double in = (double)inter[p];
        if (metric == 1) {
            const double area_d = d[kDim] * d[kDim + 2], area_g = g[kDim] * g[kDim + 2];
            res = in > 0 ? in / ((area_d + area_g) - in) : 0.0;
        } else {                                         // camera y points down, location is the bottom centre
            const double dy = d[kLoc + 1], dh = d[kDim + 1], gy = g[kLoc + 1], gh = g[kDim + 1];
            const double ih = fmin(dy, gy) - fmax(dy - dh, gy - gh);
            const double vol = (in > 0 && ih > 0) ? in * ih : 0.0;
            const double vd = (d[kDim] * d[kDim + 1]) * d[kDim + 2], vg = (g[kDim] * g[kDim + 1]) * g[kDim + 2];
            res = vol > 0 ? vol / ((vd + vg) - vol) : 0.0;
        }
    }
    out[p] = res;
}

// ---- matching ----------------------------------------------------------------------------------------------------------------
struct FrameStat { int tp, fp, fn, pad; double sim; };    // one (combo, threshold, frame) of the counting pass

struct MatchArgs {
    const double *gt, *dt;
    const int32_t *gt_cls, *dt_cls;
    const uint8_t *gt_dc;
    const int64_t *gt_off, *dt_off, *pair_off;
    const double *ov;
    int n_frames, metric, pass, n_classes, n_sets, n_thresh, aos;
    int classes[kMaxClasses];
    double min_overlap[kMaxSets][kMaxClasses];
    const double *thresholds;
    const int32_t *thresh_count;
    double *tp_score;
    long long n_gt_total;
    int32_t *n_valid;
    FrameStat *ws;
};

// One wave per work item: (frame, combo) in the threshold pass (pass 0, _match(with_fp=False)), (frame, combo, threshold) in the
// counting pass (pass 1, _frame_stats); combo = (class m, difficulty l, overlap set k).  Items of one frame are neighbours, so a
// split of 24 frames still spreads over 24 * combos * thresholds waves and the waves of a workgroup read the same rows.  The lanes
// cover the frame's detections in chunks of 64 and lane `j % 64` keeps the `assigned` bit of detection j at bit j / 64 of one
// register (at most 4096 detections per frame); the ground truths are walked in order by the whole wave.
__global__ void __launch_bounds__(256) k_kitti_match(const MatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_combo = a.n_classes * 3 * a.n_sets, T = a.pass ? a.n_thresh : 1;
    const long long item = (long long)blockIdx.x * 4 + wave;
    if (item >= (long long)a.n_frames * n_combo * T) return;
    const int t = (int)(item % T), combo = (int)(item / T % n_combo), f = (int)(item / T / n_combo);
    const int k = combo % a.n_sets, l = combo / a.n_sets % 3, m = combo / a.n_sets / 3;
    double thresh = 0.0;
    if (a.pass) {
        if (t >= a.thresh_count[combo]) return;
        thresh = a.thresholds[(size_t)combo * T + t];
    }
    const bool pass = a.pass != 0;
    const int cls = a.classes[m];
    const double mo = a.min_overlap[k][m];
    const double min_height = l == 0 ? 40.0 : 25.0, max_occ = (double)l, max_trunc = l == 0 ? 0.15 : (l == 1 ? 0.3 : 0.5);
    const long long g0 = a.gt_off[f], d0 = a.dt_off[f];
    const int ng = (int)(a.gt_off[f + 1] - g0), nd = (int)(a.dt_off[f + 1] - d0);
    const double *__restrict__ ov = a.ov + a.pair_off[f];
    const int n_chunks = (nd + 63) >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // clean_data's detection flag: 1 ignore (too small, whatever its class), 0 evaluate, -1 other class
    auto dflag_of = [&](int j) -> int {
        const double *d = a.dt + (size_t)(d0 + j) * kRow;
        return fabs(d[3] - d[1]) < min_height ? 1 : (a.dt_cls[d0 + j] == cls ? 0 : -1);
    };
    auto score_of = [&](int j) -> double { return a.dt[(size_t)(d0 + j) * kRow + kScore]; };

    unsigned long long assigned = 0ull;
    int tp = 0, fn = 0, n_valid = 0;
    double sim = 0.0;
    for (int i = 0; i < ng; ++i) {
        const double *g = a.gt + (size_t)(g0 + i) * kRow;
        const int gc = a.gt_cls[g0 + i];
        const bool same = gc == cls, neighbour = (cls == 1 && gc == 4) || (cls == 0 && gc == 3);
        const bool hard = g[kOcc] > max_occ || g[kTrunc] > max_trunc || (g[3] - g[1]) <= min_height;
        const int gflag = (neighbour || (same && hard)) ? 1 : (same ? 0 : -1);
        double *tp_out = pass ? nullptr : a.tp_score + (size_t)combo * a.n_gt_total + (g0 + i);
        if (gflag == -1) {
            if (!pass && lane == 0) *tp_out = nan;
            continue;
        }
        n_valid += gflag == 0;
        // per lane, over its detections in rising j.  key / kj: the evaluated candidate with the largest overlap (pass 0: any
        // candidate with the highest score), first one on ties; ij: the first ignored candidate (pass 1)
        double key = 0.0;
        int kj = -1, ij = INT_MAX;
        for (int c = 0; c < n_chunks; ++c) {
            const int j = c * 64 + lane;
            if (j >= nd || ((assigned >> c) & 1ull)) continue;
            const int df = dflag_of(j);
            const double s = score_of(j), o = ov[(size_t)j * ng + i];
            if (df == -1 || !(o > mo) || (pass && s < thresh)) continue;
            if (!pass) {
                if (kj < 0 || s > key) { key = s; kj = j; }
            } else if (df == 0) {
                if (kj < 0 || o > key) { key = o; kj = j; }
            } else if (ij == INT_MAX) {
                ij = j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double okey = __shfl_xor(key, o, 64);
            const int okj = __shfl_xor(kj, o, 64), oij = __shfl_xor(ij, o, 64);
            if (okj >= 0 && (kj < 0 || okey > key || (okey == key && okj < kj))) { key = okey; kj = okj; }
            ij = min(ij, oij);
        }
        const int best = kj >= 0 ? kj : (ij != INT_MAX ? ij : -1);
        if (best < 0) {
            fn += gflag == 0;
            if (!pass && lane == 0) *tp_out = nan;
            continue;
        }
        if ((best & 63) == lane) assigned |= 1ull << (best >> 6);
        const int bflag = pass ? (kj >= 0 ? 0 : 1) : dflag_of(best);
        const bool hit = !(gflag == 1 || bflag == 1);
        if (hit) {
            ++tp;
            if (a.aos) sim += (1.0 + cos(g[kAlpha] - a.dt[(size_t)(d0 + best) * kRow + kAlpha])) / 2.0;
        }
        if (!pass && lane == 0) *tp_out = hit ? score_of(best) : nan;
    }
    if (!pass) {
        if (k == 0 && lane == 0 && n_valid) atomicAdd(&a.n_valid[m * 3 + l], n_valid);
        return;
    }
    // false positives: evaluated detections left unassigned at this threshold; for the 2-D boxes, not those lying in a DontCare
    // region (intersection / detection area > min_overlap with ANY DontCare box: the host's loop over them is order-free)
    int fp = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const int j = c * 64 + lane;
        if (j >= nd || ((assigned >> c) & 1ull) || dflag_of(j) != 0 || score_of(j) < thresh) continue;
        bool dontcare = false;
        if (a.metric == 0) {
            const double *d = a.dt + (size_t)(d0 + j) * kRow;
            const double area_d = (d[2] - d[0]) * (d[3] - d[1]);
            for (int i = 0; i < ng && !dontcare; ++i) {
                if (!a.gt_dc[g0 + i]) continue;
                const double *g = a.gt + (size_t)(g0 + i) * kRow;
                const double iw = fmin(d[2], g[2]) - fmax(d[0], g[0]), ih = fmin(d[3], g[3]) - fmax(d[1], g[1]);
                const double in = (iw > 0 && ih > 0) ? iw * ih : 0.0;
                const double ua = area_d + 0.0 * ((g[2] - g[0]) * (g[3] - g[1]));
                dontcare = (in > 0 ? in / ua : 0.0) > mo;
            }
        }
        fp += !dontcare;
    }
    HVPR_WAVE_SUM_XOR(fp);
    if (lane == 0) a.ws[((size_t)combo * T + t) * a.n_frames + f] = FrameStat{tp, fp, fn, 0, sim};
}

// One wave per (combo, threshold): integer sums over the frames, and the similarity sums in ONE fixed order (lane-strided partial
// sums, then an xor butterfly), so two runs give the same bits.  No floating-point atomics.
__global__ void __launch_bounds__(64) k_kitti_reduce(const FrameStat *__restrict__ ws, const int32_t *__restrict__ thresh_count,
                                                     int n_frames, int n_thresh, int32_t *__restrict__ counts,
                                                     double *__restrict__ sim_out) {
    const int ct = blockIdx.x, lane = threadIdx.x;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    if (ct % n_thresh < thresh_count[ct / n_thresh])
        for (int f = lane; f < n_frames; f += 64) {
            const FrameStat s = ws[(size_t)ct * n_frames + f];
            tp += s.tp; fp += s.fp; fn += s.fn; sim += s.sim;
        }
    HVPR_WAVE_SUM_XOR(tp, fp, fn, sim);
    if (lane == 0) {
        counts[ct * 3 + 0] = tp; counts[ct * 3 + 1] = fp; counts[ct * 3 + 2] = fn;
        if (sim_out) sim_out[ct] = sim;
    }
}

}  // namespace

extern "C" int hvpr_kitti_overlaps_f64(const double *gt_rows, const double *dt_rows, const float *inter, const int64_t *gt_off,
                                       const int64_t *dt_off, const int64_t *pair_off, int n_frames, long long n_pairs, int metric,
                                       double *out, hvpr_stream_t stream) {
    if (n_frames < 0 || n_pairs < 0 || n_pairs > (1ll << 36) || metric < 0 || metric > 2) return HVPR_ERR_INVALID_ARG;
    if (n_frames == 0 || n_pairs == 0) return HVPR_OK;
    if (!gt_rows || !dt_rows || !gt_off || !dt_off || !pair_off || !out || (metric != 0 && !inter)) return HVPR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_kitti_overlaps, dim3(hvpr_cdiv(n_pairs, 256)), dim3(256), 0, (hipStream_t)stream, gt_rows, dt_rows, inter,
                       gt_off, dt_off, pair_off, n_frames, n_pairs, metric, out);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" size_t hvpr_kitti_match_workspace_bytes(int n_frames, int n_classes, int n_sets, int n_thresh) {
    if (n_frames < 1 || n_classes < 1 || n_sets < 1 || n_thresh < 1) return 0;
    return (size_t)n_frames * n_classes * 3 * n_sets * n_thresh * sizeof(FrameStat);
}

extern "C" int hvpr_kitti_match_f64(const double *gt_rows, const int32_t *gt_cls, const uint8_t *gt_dontcare, const double *dt_rows,
                                    const int32_t *dt_cls, const int64_t *gt_off, const int64_t *dt_off, const int64_t *pair_off,
                                    int n_frames, long long n_gt_total, const double *overlaps, int metric, int pass,
                                    const int32_t *classes, int n_classes, const double *min_overlaps, int n_sets,
                                    const double *thresholds, const int32_t *thresh_count, int n_thresh, int compute_aos,
                                    double *tp_score, int32_t *n_valid, int32_t *counts, double *sim, void *workspace,
                                    size_t workspace_bytes, hvpr_stream_t stream) {
    if (n_frames < 0 || n_gt_total < 0 || metric < 0 || metric > 2 || pass < 0 || pass > 1) return HVPR_ERR_INVALID_ARG;
    if (n_classes < 1 || n_classes > kMaxClasses || n_sets < 1 || n_sets > kMaxSets || !classes || !min_overlaps)
        return HVPR_ERR_INVALID_ARG;
    MatchArgs a;
    for (int m = 0; m < n_classes; ++m) {
        if (classes[m] < 0 || classes[m] > 5) return HVPR_ERR_INVALID_ARG;
        a.classes[m] = classes[m];
        // a candidate has overlap > min_overlap >= 0: the counting pass's pick relies on candidates having a positive overlap
        for (int k = 0; k < n_sets; ++k) {
            if (!(min_overlaps[k * n_classes + m] >= 0.0)) return HVPR_ERR_INVALID_ARG;
            a.min_overlap[k][m] = min_overlaps[k * n_classes + m];
        }
    }
    const int n_combo = n_classes * 3 * n_sets;
    if (pass == 0 ? !n_valid : (n_thresh < 1 || !thresholds || !thresh_count || !counts || (compute_aos && !sim)))
        return HVPR_ERR_INVALID_ARG;
    const long long waves = (long long)n_frames * n_combo * (pass ? n_thresh : 1);
    if (waves > (1ll << 32)) return HVPR_ERR_UNSUPPORTED;
    if (n_frames > 0) {
        if (!gt_off || !dt_off || !pair_off || (n_gt_total > 0 && (!gt_rows || !gt_cls || !gt_dontcare))) return HVPR_ERR_INVALID_ARG;
        if (pass == 0 && n_gt_total > 0 && !tp_score) return HVPR_ERR_INVALID_ARG;
        if (pass == 1 && !workspace) return HVPR_ERR_INVALID_ARG;
        if (pass == 1 && workspace_bytes < hvpr_kitti_match_workspace_bytes(n_frames, n_classes, n_sets, n_thresh))
            return HVPR_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    if (pass == 0 && hipMemsetAsync(n_valid, 0, (size_t)n_classes * 3 * sizeof(int32_t), s) != hipSuccess) return HVPR_ERR_LAUNCH;
    if (n_frames == 0) {
        if (pass == 1) {
            if (hipMemsetAsync(counts, 0, (size_t)n_combo * n_thresh * 3 * sizeof(int32_t), s) != hipSuccess) return HVPR_ERR_LAUNCH;
            if (sim && hipMemsetAsync(sim, 0, (size_t)n_combo * n_thresh * sizeof(double), s) != hipSuccess)
                return HVPR_ERR_LAUNCH;
        }
        return HVPR_OK;
    }
    a.gt = gt_rows; a.dt = dt_rows; a.gt_cls = gt_cls; a.dt_cls = dt_cls; a.gt_dc = gt_dontcare;
    a.gt_off = gt_off; a.dt_off = dt_off; a.pair_off = pair_off; a.ov = overlaps;
    a.n_frames = n_frames; a.metric = metric; a.pass = pass; a.n_classes = n_classes; a.n_sets = n_sets; a.n_thresh = n_thresh;
    a.aos = pass == 1 && compute_aos;
    a.thresholds = thresholds; a.thresh_count = thresh_count;
    a.tp_score = tp_score; a.n_gt_total = n_gt_total; a.n_valid = n_valid; a.ws = (FrameStat *)workspace;
    hipLaunchKernelGGL(k_kitti_match, dim3(hvpr_cdiv(waves, 4)), dim3(256), 0, s, a);
    if (pass == 1)
        hipLaunchKernelGGL(k_kitti_reduce, dim3(n_combo * n_thresh), dim3(64), 0, s, (const FrameStat *)workspace, thresh_count,
                           n_frames, n_thresh, counts, sim);         // without compute_aos the sums are zeros
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
