// a12 (training), NAME: ATSS — adaptive training sample selection (https://arxiv.org/abs/1912.02424) as the library's own kernels.
//   Replaces ATSSTargetAssigner.assign_targets / assign_targets_single (pcdet/models/dense_heads/target_assigner/
//   atss_target_assigner.py:16-141) with rotate_points_along_z (pcdet/utils/common_utils.py:34-56) and ResidualCoder.encode_torch
//   (pcdet/utils/box_coder_utils.py:13-43).  The reference builds per frame a dense (N, M) rotated-IoU table, a dense (N, M)
//   distance table, a topk over N rows, a (M*N) scatter and two arg-maxes, and trims padded rows with a host read per row; here a
//   batch and anchor set is seven launches, no table, no host read:
//     trim        per frame the number of rows that stay (:40-46)
//     nearest     per (anchor chunk, ground truth, frame) the TOPK smallest 64-bit keys (bits of the fp32 squared centre distance,
//                 then anchor index) of the chunk: one wave, the sorted list one key per lane, insertion by shuffle (:93-94)
//     candidates  per (ground truth, frame) one wave merges the chunk lists, clips its TOPK anchors against the ground truth, one per
//                 lane, takes mean + unbiased std + 1e-6 (float64 sums in key order), applies the inside test (:95-111) and raises
//                 the anchor's entry of a (batch, n_anchors) key plane: (IoU, lowest g) (:117-123)
//     best        per ground truth the best IoU over ALL anchors and its lowest anchor index: sweep_pairs (assign_common.h), as
//                 k_assign3d — exact rejects on the whole table, the polygon clip on densely packed survivors only (:126)
//     forced      the best anchor of every ground truth takes it, the highest g wins (:127-128)
//     write       label, box code, weight in the head's anchor order, every output row exactly once, and the positive count (:130-139)
//   The IoU of a pair is iou_bev / iou_3d of iou_geom.h on boxes rebuilt by make_box from the two rows: the bits of
//   hvpr_boxes_pairwise_f32 mode 1 / mode 2.  Integer atomics only: the same bytes on every run.  Compiled with -ffp-contract=off
//   (hvpr_amd/build.py) like every file that includes iou_geom.h.
#include "common.h"
#include "iou_geom.h"
#include "assign_common.h"

namespace {

constexpr int kAtssMaxK = 64;        // TOPK: the sorted list is one key per lane of a wave
constexpr int kAtssChunk = 2048;     // anchors a wave of the nearest kernel streams
constexpr unsigned long long kAtssNone = ~0ull;              // above every key
constexpr unsigned long long kAtssForced = 1ull << 62;       // key-plane bit of a forced match; the low 8 bits are g

// Lane i of the wave holds the i-th smallest key seen so far (kAtssNone where there is none yet); c, wave-uniform, goes to its place
// and the 64th key falls off.  Keys are unique (they end in the anchor index).
__device__ __forceinline__ void atss_insert(unsigned long long &mine, unsigned long long c, int lane) {
    const unsigned long long prev = __shfl_up(mine, 1);
    const bool prev_above = lane > 0 && prev > c;
    mine = prev_above ? prev : (mine > c ? c : mine);
}

// the keys of the lanes (kAtssNone: none) against the list: only those under the k-th key are inserted, in lane order
__device__ __forceinline__ void atss_offer(unsigned long long &mine, unsigned long long &bound, unsigned long long key, int k, int lane) {
    unsigned long long m = __ballot(key < bound);
    while (m) {                                                       // wave-uniform
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const unsigned long long c = __shfl(key, src);
        if (c < bound) {
            atss_insert(mine, c, lane);
            bound = __shfl(mine, k - 1);
        }
    }
}

// the head of the workspace (row counts, per-ground-truth maxima, key plane) to zero.  A kernel where a hipMemsetAsync over the same
// bytes would do: with the memset, tests/test_gpu_atss.py's captured call replayed to labels that differed from the eager run's
// (every other test passed); with this kernel the replay gives the eager bytes.  Why the memset node did so was not established.
__global__ void __launch_bounds__(256) k_atss_clear(unsigned long long *__restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0ull;
}

// :40-46 — n_rows = last_real_row + 1
__global__ void __launch_bounds__(256) k_atss_trim(const float *__restrict__ gt, int G, int *__restrict__ n_rows) {
    __shared__ int s_last;
    const int b = blockIdx.x;
    const int last = last_real_row(gt + (size_t)b * G * 8, G, &s_last);
    if (threadIdx.x == 0) n_rows[b] = last + 1;
}

// grid (chunk, g, frame), one wave: the k nearest anchors of the chunk, ascending, into partial[((frame * G + g) * chunks + chunk) * k ..]
__global__ void __launch_bounds__(64) k_atss_nearest(const float *__restrict__ anchors, int A, const float *__restrict__ gt, int G, int k,
                                                     const int *__restrict__ n_rows, unsigned long long *__restrict__ partial) {
    const int lane = threadIdx.x, chunk = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    if (g >= n_rows[b]) return;
    const float *gp = gt + ((size_t)b * G + g) * 8;
    const float gx = gp[0], gy = gp[1], gz = gp[2];
    unsigned long long mine = kAtssNone, bound = kAtssNone;
    const int a_begin = chunk * kAtssChunk;
    const int a_end = A - a_begin < kAtssChunk ? A : a_begin + kAtssChunk;
    for (int a0 = a_begin; a0 < a_end; a0 += 64) {
        const int a = a0 + lane;
        unsigned long long key = kAtssNone;
        if (a < a_end) {
            const float *p = anchors + (size_t)a * 7;
            const float dx = p[0] - gx, dy = p[1] - gy, dz = p[2] - gz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)a;
        }
        atss_offer(mine, bound, key, k, lane);
    }
    if (lane < k) partial[(((size_t)b * G + g) * gridDim.x + chunk) * k + lane] = mine;
}

// grid (g, frame), one wave, one candidate per lane
template <int MATCH_HEIGHT>
__global__ void __launch_bounds__(64) k_atss_candidates(const float *__restrict__ anchors, int A, const float *__restrict__ gt, int G, int k,
                                                        int chunks, const int *__restrict__ n_rows,
                                                        const unsigned long long *__restrict__ partial,
                                                        unsigned long long *__restrict__ plane) {
    __shared__ PolyStore ps;
    __shared__ float s_iou[kAtssMaxK];
    const int lane = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
    if (g >= n_rows[b]) return;
    const unsigned long long *src = partial + ((size_t)b * G + g) * chunks * k;
    const int total = chunks * k;
    unsigned long long mine = kAtssNone, bound = kAtssNone;
    for (int i0 = 0; i0 < total; i0 += 64) {
        const int i = i0 + lane;
        atss_offer(mine, bound, i < total ? src[i] : kAtssNone, k, lane);
    }
    const float *pb = gt + ((size_t)b * G + g) * 8;
    const bool live = lane < k && mine != kAtssNone;                  // k <= n_anchors: every one of the k lanes holds an anchor
    const unsigned a = live ? (unsigned)mine : 0u;
    const float *pa = anchors + (size_t)a * 7;
    float v = 0.f;
    if (live) {
        Box Ab, Bb;
        make_box(pa, Ab);
        make_box(pb, Bb);
        v = MATCH_HEIGHT ? iou_3d(pa, pb, Ab, Bb, ps, lane) : iou_bev(Ab, Bb, ps, lane);
    }
    s_iou[lane] = v;
    __syncthreads();
    // :96-98, the sums in float64 over the candidates in key order; TOPK 1: 0 / 0, a NaN threshold that nothing reaches
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += (double)s_iou[i];
    const double mean = sum / (double)k;
    double ss = 0.0;
    for (int i = 0; i < k; ++i) {
        const double d = (double)s_iou[i] - mean;
        ss += d * d;
    }
    const double var = ss / (double)(k - 1);
    const float thresh = (float)mean + (float)sqrt(var) + 1e-6f;
    if (!live) return;
    // :102-111, as written: rotate_points_along_z by -heading, then x against dy and y against dx
    const float h = pb[6];
    const float c = cosf(-h), s = sinf(-h);
    const float dx = pa[0] - pb[0], dy = pa[1] - pb[1];
    const float xl = dx * c + dy * (-s);
    const float yl = dx * s + dy * c;
    const float lx = pb[4], ly = pb[3];
    const bool inside = xl <= lx / 2 && xl >= -lx / 2 && yl <= ly / 2 && yl >= -ly / 2;
    if (v >= thresh && inside)                                        // the maximum is the highest IoU, then the lowest g (:123)
        atomicMax(&plane[(size_t)b * A + a], ((unsigned long long)hvpr_ord_of(v) << 8) | (unsigned)(255 - g));
}

// ---- the best anchor of every ground truth: sweep_pairs (assign_common.h) over every row that stays, no class mask ---------------------
struct AtssLds {
    PolyStore ps;
    __attribute__((aligned(16))) BoxLite gl[kMaxGt];
    unsigned long long gv[kMaxGt];           // the workgroup's best (hvpr_ord_of(iou), ~anchor) per ground truth; 0: no pair reached the clip
    unsigned short ring[kSweepRing];         // (anchor in workgroup) << 8 | g
};

template <int MATCH_HEIGHT>
__device__ __forceinline__ void atss_clip_round(AtssLds &s, const float *__restrict__ anchors, int a0, const float *__restrict__ gt_frame,
                                                int head, int n) {
    const int lane = threadIdx.x;
    if (lane < n) {
        const int e = s.ring[(head + lane) & (kSweepRing - 1)];
        const int al = e >> 8, g = e & 255;
        const float *pa = anchors + (size_t)(a0 + al) * 7, *pb = gt_frame + (size_t)g * 8;
        Box A, B;
        make_box(pa, A);
        make_box(pb, B);
        const float v = MATCH_HEIGHT ? iou_3d(pa, pb, A, B, s.ps, lane) : iou_bev(A, B, s.ps, lane);
        atomicMax(&s.gv[g], ((unsigned long long)hvpr_ord_of(v) << 32) | (unsigned)~(unsigned)(a0 + al));
    }
}

template <int MATCH_HEIGHT>
__global__ void __launch_bounds__(64) k_atss_best(const float *__restrict__ anchors, int A, const float *__restrict__ gt, int G,
                                                  const int *__restrict__ n_rows, unsigned long long *__restrict__ gbest) {
    __shared__ AtssLds s;
    const int lane = threadIdx.x, b = blockIdx.y;
    const float *gt_frame = gt + (size_t)b * G * 8;
    const int n = n_rows[b];
    for (int g = lane; g < n; g += 64) {
        Box bx;
        make_box(gt_frame + (size_t)g * 8, bx);
        s.gl[g] = lite_of(bx);
        s.gv[g] = 0ull;
    }
    __syncthreads();
    const int a0 = blockIdx.x * 64, a = a0 + lane;
    const bool valid = a < A;
    BoxLite al = BoxLite{0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    if (valid) {
        Box ab;
        make_box(anchors + (size_t)a * 7, ab);
        al = lite_of(ab);
    }
    sweep_pairs(s.ring, s.gl, n, al, valid, [](int) { return true; },
                [&](int head, int cnt) { atss_clip_round<MATCH_HEIGHT>(s, anchors, a0, gt_frame, head, cnt); });
    for (int g = lane; g < n; g += 64)
        if (s.gv[g]) atomicMax(&gbest[(size_t)b * G + g], s.gv[g]);
}

// :126-128 — a rejected pair is IoU +0 and no IoU is below it, so an entry that is untouched or holds 0 means the first of all
// anchors, anchor 0; there is no `> 0` guard.  The plane's maximum is the highest g.
__global__ void __launch_bounds__(256) k_atss_forced(int A, int G, int batch, const int *__restrict__ n_rows,
                                                     const unsigned long long *__restrict__ gbest, unsigned long long *__restrict__ plane) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= batch * G) return;
    const int b = t / G, g = t % G;
    if (g >= n_rows[b]) return;
    const unsigned long long key = gbest[t];
    unsigned a = 0u;
    if (key && hvpr_of_ord((unsigned)(key >> 32)) > 0.f) a = ~(unsigned)key;
    atomicMax(&plane[(size_t)b * A + a], kAtssForced | (unsigned)g);
}

// :130-139, one thread per anchor, written straight into the head's anchor order
__global__ void __launch_bounds__(256) k_atss_write(const float *__restrict__ anchors, int A, const float *__restrict__ gt, int G,
                                                    int n_classes, const unsigned long long *__restrict__ plane, int per_loc,
                                                    int loc_stride, int loc_offset, long long a_total, int *__restrict__ labels,
                                                    float *__restrict__ targets, float *__restrict__ weights, int *__restrict__ pos_count) {
    __shared__ int s_pos;
    if (threadIdx.x == 0) s_pos = 0;
    __syncthreads();
    const int a = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    int fg = 0;
    if (a < A) {
        const unsigned long long key = plane[(size_t)b * A + a];
        int lab = 0, arg = 0;
        if (key) {
            arg = (key & kAtssForced) ? (int)(key & 255u) : 255 - (int)(key & 255u);
            const float c = gt[((size_t)b * G + arg) * 8 + 7];
            lab = (c >= 0.f && c <= (float)n_classes) ? (int)c : 0;
        }
        fg = lab > 0 ? 1 : 0;
        const float *an = anchors + (size_t)a * 7;
        const size_t o = (size_t)b * a_total + head_row(a, per_loc, loc_stride, loc_offset);
        labels[o] = lab;
        weights[o] = fg ? 1.f : 0.f;
        float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (fg) encode_residual(an, gt + ((size_t)b * G + arg) * 8, t);
        for (int j = 0; j < 7; ++j) targets[o * 7 + j] = t[j];
    }
    const unsigned long long m = __ballot(fg != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_pos, __popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_pos) atomicAdd(&pos_count[b], s_pos);
}

// workspace: [n_rows: batch ints][gbest: batch * n_gt keys][plane: batch * n_anchors keys] — cleared by k_atss_clear — then the chunk lists
struct AtssLayout {
    size_t n_rows, gbest, plane, partial, total;
    int chunks;
};

AtssLayout atss_layout(int batch, int n_gt, int n_anchors, int topk) {
    AtssLayout l;
    const size_t g = n_gt > 0 ? n_gt : 1;
    l.chunks = hvpr_cdiv(n_anchors, kAtssChunk);
    l.n_rows = 0;
    l.gbest = round256((size_t)batch * sizeof(int));
    l.plane = l.gbest + round256((size_t)batch * g * sizeof(unsigned long long));
    l.partial = l.plane + round256((size_t)batch * n_anchors * sizeof(unsigned long long));
    l.total = l.partial + round256((size_t)batch * g * l.chunks * topk * sizeof(unsigned long long));
    return l;
}

}  // namespace

extern "C" size_t hvpr_assign_targets_atss_workspace_bytes(int batch, int n_gt, int n_anchors, int topk) {
    if (batch < 1 || n_gt < 0 || n_anchors < 1 || topk < 1 || topk > kAtssMaxK) return 0;
    return atss_layout(batch, n_gt, n_anchors, topk).total;
}

extern "C" int hvpr_assign_targets_atss_f32(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int n_classes,
                                            int topk, int match_height, int per_loc, int loc_stride, int loc_offset,
                                            long long anchors_total, int32_t *labels, float *reg_targets, float *reg_weights,
                                            int32_t *pos_count, void *workspace, size_t workspace_bytes, hvpr_stream_t stream) {
    const int bad = assign_args_status(anchors, n_anchors, gt_boxes, batch, n_gt, 0, n_classes, per_loc, loc_stride, loc_offset,
                                       anchors_total, labels, reg_targets, reg_weights, pos_count, workspace);
    if (bad) return bad;
    if (topk < 1 || topk > n_anchors) return HVPR_ERR_INVALID_ARG;       // torch.topk raises there
    if (topk > kAtssMaxK || n_gt > kMaxGt || batch > 65535) return HVPR_ERR_UNSUPPORTED;
    const AtssLayout l = atss_layout(batch, n_gt, n_anchors, topk);
    if (workspace_bytes < l.total) return HVPR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int *n_rows = (int *)(ws + l.n_rows);
    unsigned long long *gbest = (unsigned long long *)(ws + l.gbest);
    unsigned long long *plane = (unsigned long long *)(ws + l.plane);
    unsigned long long *partial = (unsigned long long *)(ws + l.partial);
    const size_t words = l.partial / sizeof(unsigned long long);       // every region is a multiple of 256 bytes
    hipLaunchKernelGGL(k_atss_clear, dim3(hvpr_cdiv((long long)words, 256 * 8) < 2048 ? hvpr_cdiv((long long)words, 256 * 8) : 2048), dim3(256), 0, s,
                       (unsigned long long *)ws, words);
    if (n_gt > 0) {
        hipLaunchKernelGGL(k_atss_trim, dim3(batch), dim3(256), 0, s, gt_boxes, n_gt, n_rows);
        hipLaunchKernelGGL(k_atss_nearest, dim3(l.chunks, n_gt, batch), dim3(64), 0, s, anchors, n_anchors, gt_boxes, n_gt, topk, n_rows,
                           partial);
        const dim3 gc(n_gt, batch), gb(hvpr_cdiv(n_anchors, 64), batch);
        if (match_height) {
            hipLaunchKernelGGL(k_atss_candidates<1>, gc, dim3(64), 0, s, anchors, n_anchors, gt_boxes, n_gt, topk, l.chunks, n_rows, partial,
                               plane);
            hipLaunchKernelGGL(k_atss_best<1>, gb, dim3(64), 0, s, anchors, n_anchors, gt_boxes, n_gt, n_rows, gbest);
        } else {
            hipLaunchKernelGGL(k_atss_candidates<0>, gc, dim3(64), 0, s, anchors, n_anchors, gt_boxes, n_gt, topk, l.chunks, n_rows, partial,
                               plane);
            hipLaunchKernelGGL(k_atss_best<0>, gb, dim3(64), 0, s, anchors, n_anchors, gt_boxes, n_gt, n_rows, gbest);
        }
        hipLaunchKernelGGL(k_atss_forced, dim3(hvpr_cdiv((long long)batch * n_gt, 256)), dim3(256), 0, s, n_anchors, n_gt, batch, n_rows,
                           gbest, plane);
    }
    hipLaunchKernelGGL(k_atss_write, dim3(hvpr_cdiv(n_anchors, 256), batch), dim3(256), 0, s, anchors, n_anchors, gt_boxes, n_gt, n_classes,
                       plane, per_loc, loc_stride, loc_offset, anchors_total, labels, reg_targets, reg_weights, pos_count);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
