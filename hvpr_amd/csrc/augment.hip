// Training augmentation on the device, for every frame of a batch at once: the reference's DataAugmentor
// (pcdet/datasets/augmentor/: database_sampler.py GT sampling, augmentor_utils.py world flip / rotation / scaling,
// data_augmentor.py:95-97 limit_period) and the training-only box trim of data_processor.py:24-28.
//
// Every random draw stays on the host (hvpr_amd/augment.py, AugmentPlanner) and comes here as ONE packed plan; everything that
// touches points or tests geometry runs below.  The plan is a block of 32-bit words, present twice: in (pinned) host memory, where
// every entry point checks it before any launch, and on the device, where the kernels read it.
//
//   words 0..7  magic, B frames, NG sample groups, G ground truths, C candidates, ops, 0, 0
//   int32       gt_off[B+1]  grp_off[B*NG+1]  pt_off[B+1]  gt_cls[G]  cand_obj[C]  cand_cls[C]  cand_frame[C]  cand_start[C]
//               cand_n[C]
//   float       gt_box[G*7]  cand_box[C*7]  cand_mv[C]  xf[B*8]
//
// gt_cls is class index + 1 of a ground truth, or 0 for one of a class that is not trained (the reference's gt_boxes_mask hides
// it, but it still blocks candidates: database_sampler.py:168-170).  Frame f owns candidates grp_off[f*NG] .. grp_off[(f+1)*NG],
// group g of it the slice grp_off[f*NG+g] .. grp_off[f*NG+g+1].  cand_start / cand_n are the candidate's rows in the bank arena,
// cand_mv its road-plane height move.  xf[f] = flip_x, flip_y, cos, sin, angle, scale, 0, 0; `ops` lists the world transforms in
// the configured order, four bits each (1 flip x, 2 flip y, 3 rotation, 4 scaling), 0 ends the list.
//
// Built with -ffp-contract=off: the fp32 operation order below is the reference's.
#include "box_cut.h"
#include "common.h"
#include "iou_geom.h"

#include <algorithm>

namespace {

constexpr int kMagic = 0x31475541;   // "AUG1"
constexpr int kHdr = 8;
constexpr int kMaxOps = 8;
constexpr int kFrameBoxes = 256;     // ground truths + candidates of one frame (collision kernel), candidates of one frame (points)
constexpr int kBlk = 256;            // scene points per workgroup of the count and write passes
constexpr float kPi = 3.14159274f, kTwoPi = 6.28318548f;     // float32(np.pi), float32(2 * np.pi)

struct Plan {
    int B, NG, G, C;
    unsigned ops;
    const int32_t *gt_off, *grp_off, *pt_off, *gt_cls, *cand_obj, *cand_cls, *cand_frame, *cand_start, *cand_n;
    const float *gt_box, *cand_box, *cand_mv, *xf;
};

long long plan_words(long long B, long long NG, long long G, long long C) {
    return kHdr + (B + 1) + (B * NG + 1) + (B + 1) + G + 5 * C + 7 * G + 7 * C + C + 8 * B;
}

Plan plan_view(const int32_t *w, int B, int NG, int G, int C, unsigned ops) {
    Plan p;
    p.B = B; p.NG = NG; p.G = G; p.C = C; p.ops = ops;
    const int32_t *q = w + kHdr;
    p.gt_off = q; q += B + 1;
    p.grp_off = q; q += (size_t)B * NG + 1;
    p.pt_off = q; q += B + 1;
    p.gt_cls = q; q += G;
    p.cand_obj = q; q += C;
    p.cand_cls = q; q += C;
    p.cand_frame = q; q += C;
    p.cand_start = q; q += C;
    p.cand_n = q; q += C;
    const float *f = (const float *)q;
    p.gt_box = f; f += (size_t)G * 7;
    p.cand_box = f; f += (size_t)C * 7;
    p.cand_mv = f; f += C;
    p.xf = f;
    return p;
}

bool rising(const int32_t *off, int n, int last) {     // off[0] = 0 <= off[1] <= ... <= off[n] = last
    if (off[0] != 0 || off[n] != last) return false;
    for (int i = 0; i < n; ++i)
        if (off[i] > off[i + 1]) return false;
    return true;
}

// Checks the host copy of a plan and makes the view of the device copy.  0, or the status to return.
int plan_open(const int32_t *host, const int32_t *dev, int words, Plan &h, Plan &d) {
    if (!host || !dev || words < kHdr) return HVPR_ERR_INVALID_ARG;
    const int B = host[1], NG = host[2], G = host[3], C = host[4];
    if (host[0] != kMagic || B < 1 || NG < 0 || G < 0 || C < 0 || B > 4096 || NG > 64) return HVPR_ERR_INVALID_ARG;
    if (plan_words(B, NG, G, C) != words) return HVPR_ERR_INVALID_ARG;
    const unsigned ops = (unsigned)host[5];
    bool ended = false;
    for (int k = 0; k < kMaxOps; ++k) {
        const unsigned op = (ops >> (4 * k)) & 15u;
        if (op > 4u || (ended && op)) return HVPR_ERR_INVALID_ARG;
        ended |= op == 0;
    }
    h = plan_view(host, B, NG, G, C, ops);
    d = plan_view(dev, B, NG, G, C, ops);
    if (!rising(h.gt_off, B, G) || !rising(h.grp_off, B * NG, C) || h.pt_off[0] != 0) return HVPR_ERR_INVALID_ARG;
    for (int f = 0; f < B; ++f) {
        if (h.pt_off[f] > h.pt_off[f + 1]) return HVPR_ERR_INVALID_ARG;
        const int c0 = h.grp_off[f * NG], c1 = h.grp_off[(f + 1) * NG];
        for (int c = c0; c < c1; ++c)
            if (h.cand_frame[c] != f) return HVPR_ERR_INVALID_ARG;
    }
    return 0;
}

struct Xf { float fx, fy, c, s, ang, sc; };

__device__ __forceinline__ Xf load_xf(const Plan &p, int f) {
    const float *x = p.xf + (size_t)f * 8;
    return Xf{x[0], x[1], x[2], x[3], x[4], x[5]};
}

// augmentor_utils.py on one point: flips :17 / :36, rotation (common_utils.rotate_points_along_z: [x y z] times
// [[c, s, 0], [-s, c, 0], [0, 0, 1]]), scaling :76.  The reference's product is a float32 gemm over all points of a frame, and a
// gemm accumulates along k with fused multiply-adds: x' = fma(y, -s, x c), y' = fma(y, c, x s) (fixture G19 holds exactly these
// bits).  The second product is therefore fused here ON PURPOSE, by an explicit fmaf: the file is still built with contraction
// off, nothing is left to the compiler.  The unfused sum differs by the rounding of one product, which is many ulp of the result
// where the two products cancel.  (For fewer than 45 rows torch sums unfused: that is the boxes' path, xf_box below.)
__device__ __forceinline__ void xf_point(unsigned ops, const Xf &t, float &x, float &y, float &z) {
    for (int k = 0; k < kMaxOps; ++k) {
        const unsigned op = (ops >> (4 * k)) & 15u;
        if (op == 0) break;
        if (op == 1) { if (t.fx != 0.0f) y = -y; }
        else if (op == 2) { if (t.fy != 0.0f) x = -x; }
        else if (op == 3) {
            const float nx = fmaf(y, -t.s, x * t.c), ny = fmaf(y, t.c, x * t.s);
            x = nx; y = ny;
        } else { x *= t.sc; y *= t.sc; z *= t.sc; }
    }
}

// ... and on one box row (x, y, z, dx, dy, dz, heading): :15-16, :34-35, :54-55, :77.  A frame's few boxes go through torch's
// small-matrix product, a plain sum of products: unfused.
__device__ __forceinline__ void xf_box(unsigned ops, const Xf &t, float *b) {
    for (int k = 0; k < kMaxOps; ++k) {
        const unsigned op = (ops >> (4 * k)) & 15u;
        if (op == 0) break;
        if (op == 1) { if (t.fx != 0.0f) { b[1] = -b[1]; b[6] = -b[6]; } }
        else if (op == 2) { if (t.fy != 0.0f) { b[0] = -b[0]; b[6] = -(b[6] + kPi); } }
        else if (op == 3) {
            const float nx = b[0] * t.c + b[1] * (-t.s), ny = b[0] * t.s + b[1] * t.c;
            b[0] = nx; b[1] = ny; b[6] = b[6] + t.ang;
        } else {
            for (int j = 0; j < 6; ++j) b[j] *= t.sc;
        }
    }
}

// ---- collision: which candidates of a frame may be pasted ------------------------------------------------------------------------
// One wave per frame, a lane per candidate of the current group; the groups go in order with a barrier between them, because a
// group is tested against what the groups before it accepted (database_sampler.py:172-193).
__global__ void __launch_bounds__(64) k_collide(const Plan p, int32_t *__restrict__ valid) {
    __shared__ PolyStore ps;
    __shared__ Box bx[kFrameBoxes];          // the frame's ground truths, then its candidates
    __shared__ int e_idx[kFrameBoxes];       // the existing set, as indices into bx
    __shared__ int ok[kFrameBoxes];
    const int f = blockIdx.x, ln = threadIdx.x;
    const int g0 = p.gt_off[f], nG = p.gt_off[f + 1] - g0;
    const int c0 = p.grp_off[f * p.NG], nC = p.grp_off[(f + 1) * p.NG] - c0;
    for (int i = ln; i < nG + nC; i += 64) {
        Box t;
        make_box(i < nG ? p.gt_box + (size_t)(g0 + i) * 7 : p.cand_box + (size_t)(c0 + i - nG) * 7, t);
        bx[i] = t;
        if (i < nG) e_idx[i] = i;
    }
    __syncthreads();
    int nE = nG;
    for (int g = 0; g < p.NG; ++g) {
        const int s0 = p.grp_off[f * p.NG + g] - c0, nS = p.grp_off[f * p.NG + g + 1] - c0 - s0;
        for (int k = ln; k < nS; k += 64) {
            const Box A = bx[nG + s0 + k];
            float m1 = -INFINITY, m2 = -INFINITY;
            for (int e = 0; e < nE; ++e) {                                   // iou1: against the existing set
                const Box E = bx[e_idx[e]];
                m1 = fmaxf(m1, iou_bev(A, E, ps, ln));
            }
            for (int j = 0; j < nS; ++j) {                                   // iou2: against the whole group, diagonal zeroed
                float v = 0.0f;
                if (j != k) {
                    const Box S = bx[nG + s0 + j];
                    v = iou_bev(A, S, ps, ln);
                }
                m2 = fmaxf(m2, v);
            }
            if (nE == 0) m1 = m2;                                            // :187
            ok[s0 + k] = (m1 + m2 == 0.0f) ? 1 : 0;                          // :188
        }
        __syncthreads();
        for (int k = 0; k < nS; ++k)                                         // every lane walks the group: nE stays uniform
            if (ok[s0 + k]) {
                if (ln == 0) e_idx[nE] = nG + s0 + k;
                ++nE;
            }
        __syncthreads();
    }
    for (int k = ln; k < nC; k += 64) valid[c0 + k] = ok[k];
}

// ---- boxes: masked-in ground truths, then the accepted candidates; transformed, trimmed, padded ---------------------------------
__global__ void __launch_bounds__(64) k_boxes(const Plan p, const int32_t *__restrict__ valid, float x0, float y0, float z0, float x1,
                                              float y1, float z1, int remove_outside, int g_cap, float *__restrict__ out,
                                              int32_t *__restrict__ count) {
    const int f = blockIdx.x, ln = threadIdx.x;
    const int g0 = p.gt_off[f], nG = p.gt_off[f + 1] - g0;
    const int c0 = p.grp_off[f * p.NG], nC = p.grp_off[(f + 1) * p.NG] - c0;
    const Xf t = load_xf(p, f);
    float *dst = out + (size_t)f * g_cap * 8;
    int base = 0;
    for (int i0 = 0; i0 < nG + nC; i0 += 64) {
        const int i = i0 + ln;
        bool keep = false;
        float b[7];
        float cls = 0.0f;
        if (i < nG + nC) {
            const bool gt = i < nG;
            const int c = gt ? p.gt_cls[g0 + i] : (valid[c0 + i - nG] ? p.cand_cls[c0 + i - nG] : 0);
            if (c > 0) {
                const float *src = gt ? p.gt_box + (size_t)(g0 + i) * 7 : p.cand_box + (size_t)(c0 + i - nG) * 7;
                for (int j = 0; j < 7; ++j) b[j] = src[j];
                xf_box(p.ops, t, b);
                b[6] = b[6] - floorf(b[6] / kTwoPi + 0.5f) * kTwoPi;          // limit_period(heading, 0.5, 2 pi)
                cls = (float)c;
                keep = true;
                if (remove_outside) {                                         // box_utils.py:55-71, min_num_corners = 1
                    const float cs = cosf(b[6]), sn = sinf(b[6]);
                    int inside = 0;
                    for (int k = 0; k < 8; ++k) {
                        const float lx = (k & 1 ? -0.5f : 0.5f) * b[3], ly = (k & 2 ? -0.5f : 0.5f) * b[4],
                                    lz = (k & 4 ? -0.5f : 0.5f) * b[5];
                        const float cx = lx * cs + ly * (-sn) + b[0], cy = lx * sn + ly * cs + b[1], cz = lz + b[2];
                        inside += (cx >= x0 && cx <= x1 && cy >= y0 && cy <= y1 && cz >= z0 && cz <= z1) ? 1 : 0;
                    }
                    keep = inside >= 1;
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            float *r = dst + (size_t)(base + __popcll(m & ((1ull << ln) - 1ull))) * 8;
            for (int j = 0; j < 7; ++j) r[j] = b[j];
            r[7] = cls;
        }
        base += __popcll(m);
    }
    for (int i = base * 8 + ln; i < g_cap * 8; i += 64) dst[i] = 0.0f;
    if (ln == 0) count[f] = base;
}

// ---- points ----------------------------------------------------------------------------------------------------------------------
// The accepted candidates of the frame, enlarged by REMOVE_EXTRA_WIDTH (box_utils.enlarge_box3d), for the inside test of
// box_cut.h.  A rejected candidate gets a negative half height: nothing is inside it.
__device__ __forceinline__ void load_cuts(const Plan &p, const int32_t *valid, int c0, int nC, float ex, float ey, float ez,
                                          hvpr_cut *cut) {
    for (int k = threadIdx.x; k < nC; k += blockDim.x) {
        hvpr_cut c = hvpr_make_cut(p.cand_box + (size_t)(c0 + k) * 7, ex, ey, ez);
        if (!valid[c0 + k]) c.hz = -1.0f;
        cut[k] = c;
    }
}

// stable rank of the lanes with `keep` inside the workgroup (kBlk threads); total in `total`
__device__ __forceinline__ int block_rank(bool keep, int *wave_n, int &total) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (ln == 0) wave_n[wv] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < kBlk / 64; ++w) {
        if (w < wv) before += wave_n[w];
        total += wave_n[w];
    }
    return before + __popcll(m & ((1ull << ln) - 1ull));
}

// pass 1: flag[i] = scene point i stays; blk_cnt[f * max_blk + b] = how many of block b of frame f stay
__global__ void __launch_bounds__(kBlk) k_points_count(const Plan p, const int32_t *__restrict__ valid, const float *__restrict__ pts,
                                                       int F, float ex, float ey, float ez, uint8_t *__restrict__ flag,
                                                       int32_t *__restrict__ blk_cnt) {
    __shared__ hvpr_cut cut[kFrameBoxes];
    __shared__ int wave_n[kBlk / 64];
    const int f = blockIdx.y;
    const int c0 = p.grp_off[f * p.NG], nC = p.grp_off[(f + 1) * p.NG] - c0;
    const int n = p.pt_off[f + 1] - p.pt_off[f], j = blockIdx.x * kBlk + threadIdx.x;
    if (blockIdx.x * kBlk < n) load_cuts(p, valid, c0, nC, ex, ey, ez, cut);
    __syncthreads();
    bool keep = false;
    if (j < n) {
        const float *q = pts + (size_t)(p.pt_off[f] + j) * F;
        const float x = q[0], y = q[1], z = q[2];
        keep = true;
        for (int k = 0; k < nC; ++k)
            if (hvpr_cut_inside(cut[k], x, y, z)) { keep = false; break; }
        flag[p.pt_off[f] + j] = keep ? 1 : 0;
    }
    int total;
    block_rank(keep, wave_n, total);
    if (threadIdx.x == 0) blk_cnt[(size_t)f * gridDim.x + blockIdx.x] = total;
}

// pass 2: where everything goes.  Frame f's output is its accepted candidates' points in candidate order, then its kept scene
// points in their order (database_sampler.py:150-151).
__global__ void __launch_bounds__(256) k_points_scan(const Plan p, const int32_t *__restrict__ valid, const int32_t *__restrict__ blk_cnt,
                                                     int max_blk, int32_t *__restrict__ blk_pre, int32_t *__restrict__ cand_pre,
                                                     int32_t *__restrict__ out_off) {
    __shared__ int wave_sum[256 / 64];
    hvpr_block_scan([&](int i) { return blk_cnt[i]; }, p.B * max_blk, 0, blk_pre, true, wave_sum);
    hvpr_block_scan([&](int i) { return valid[i] ? p.cand_n[i] : 0; }, p.C, 0, cand_pre, true, wave_sum);
    for (int f = threadIdx.x; f <= p.B; f += blockDim.x)
        out_off[f] = f < p.B ? cand_pre[p.grp_off[f * p.NG]] + blk_pre[(size_t)f * max_blk] : cand_pre[p.C] + blk_pre[(size_t)p.B * max_blk];
}

// pass 3a: the kept scene points
__global__ void __launch_bounds__(kBlk) k_points_write_scene(const Plan p, const float *__restrict__ pts, int F,
                                                             const uint8_t *__restrict__ flag, const int32_t *__restrict__ blk_pre,
                                                             const int32_t *__restrict__ cand_pre, const int32_t *__restrict__ out_off,
                                                             float *__restrict__ out) {
    __shared__ int wave_n[kBlk / 64];
    const int f = blockIdx.y;
    const int n = p.pt_off[f + 1] - p.pt_off[f], j = blockIdx.x * kBlk + threadIdx.x;
    if (blockIdx.x * kBlk >= n) return;                                      // the whole workgroup leaves
    const bool keep = j < n && flag[p.pt_off[f] + j] != 0;
    int total;
    const int rank = block_rank(keep, wave_n, total);
    if (!keep) return;
    const size_t e = (size_t)f * gridDim.x + blockIdx.x;
    const int row = out_off[f] + (cand_pre[p.grp_off[(f + 1) * p.NG]] - cand_pre[p.grp_off[f * p.NG]]) +
                    (blk_pre[e] - blk_pre[(size_t)f * gridDim.x]) + rank;
    const float *q = pts + (size_t)(p.pt_off[f] + j) * F;
    float *r = out + (size_t)row * F;
    float x = q[0], y = q[1], z = q[2];
    xf_point(p.ops, load_xf(p, f), x, y, z);
    r[0] = x; r[1] = y; r[2] = z;
    for (int k = 3; k < F; ++k) r[k] = q[k];
}

// pass 3b: the accepted candidates' points, from the bank arena: a workgroup per candidate (database_sampler.py:133-142)
__global__ void __launch_bounds__(256) k_points_write_cand(const Plan p, const int32_t *__restrict__ valid, const float *__restrict__ bank,
                                                           const float *__restrict__ bank_box, int F, const int32_t *__restrict__ cand_pre,
                                                           const int32_t *__restrict__ out_off, float *__restrict__ out) {
    const int c = blockIdx.x;
    if (!valid[c]) return;
    const int f = p.cand_frame[c], n = p.cand_n[c];
    const float *ctr = bank_box + (size_t)p.cand_obj[c] * 7;
    const float bx = ctr[0], by = ctr[1], bz = ctr[2], mv = p.cand_mv[c];
    const Xf t = load_xf(p, f);
    const float *src = bank + (size_t)p.cand_start[c] * F;
    float *dst = out + (size_t)(out_off[f] + cand_pre[c] - cand_pre[p.grp_off[f * p.NG]]) * F;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const float *q = src + (size_t)j * F;
        float *r = dst + (size_t)j * F;
        float x = q[0] + bx, y = q[1] + by, z = (q[2] + bz) - mv;
        xf_point(p.ops, t, x, y, z);
        r[0] = x; r[1] = y; r[2] = z;
        for (int k = 3; k < F; ++k) r[k] = q[k];
    }
}

int max_frame_blocks(const Plan &h) {
    int m = 1;
    for (int f = 0; f < h.B; ++f) m = std::max(m, hvpr_cdiv(h.pt_off[f + 1] - h.pt_off[f], kBlk));
    return m;
}

struct PointsWs { uint8_t *flag; int32_t *blk_cnt, *blk_pre, *cand_pre; size_t bytes; };

PointsWs points_ws(void *base, int B, int max_blk, int C, long long n_points) {
    hvpr_carver cv(base);
    PointsWs w;
    w.flag = cv.take<uint8_t>((size_t)n_points);
    w.blk_cnt = cv.take<int32_t>((size_t)B * max_blk);
    w.blk_pre = cv.take<int32_t>((size_t)B * max_blk + 1);
    w.cand_pre = cv.take<int32_t>((size_t)C + 1);
    w.bytes = cv.off;
    return w;
}

}  // namespace

extern "C" int hvpr_augment_block_points(void) { return kBlk; }

extern "C" int hvpr_augment_collide_f32(const int32_t *plan_host, const int32_t *plan_dev, int plan_words, int32_t *valid,
                                        hvpr_stream_t stream) {
    Plan h, d;
    if (const int st = plan_open(plan_host, plan_dev, plan_words, h, d)) return st;
    if (h.C > 0 && !valid) return HVPR_ERR_INVALID_ARG;
    for (int f = 0; f < h.B; ++f)
        if (h.gt_off[f + 1] - h.gt_off[f] + h.grp_off[(f + 1) * h.NG] - h.grp_off[f * h.NG] > kFrameBoxes) return HVPR_ERR_UNSUPPORTED;
    if (h.C == 0) return HVPR_OK;
    hipLaunchKernelGGL(k_collide, dim3(h.B), dim3(64), 0, (hipStream_t)stream, d, valid);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_augment_boxes_f32(const int32_t *plan_host, const int32_t *plan_dev, int plan_words, const int32_t *valid,
                                      const float *range6, int remove_outside, int g_cap, float *gt_out, int32_t *box_count,
                                      hvpr_stream_t stream) {
    Plan h, d;
    if (const int st = plan_open(plan_host, plan_dev, plan_words, h, d)) return st;
    if ((h.C > 0 && !valid) || !range6 || g_cap < 0 || (g_cap > 0 && !gt_out) || !box_count) return HVPR_ERR_INVALID_ARG;
    for (int f = 0; f < h.B; ++f) {                                          // a frame's rows must fit whatever the collisions decide
        int rows = h.grp_off[(f + 1) * h.NG] - h.grp_off[f * h.NG];
        for (int g = h.gt_off[f]; g < h.gt_off[f + 1]; ++g) rows += h.gt_cls[g] > 0;
        if (rows > g_cap) return HVPR_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(k_boxes, dim3(h.B), dim3(64), 0, (hipStream_t)stream, d, valid, range6[0], range6[1], range6[2], range6[3],
                       range6[4], range6[5], remove_outside, g_cap, gt_out, box_count);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" size_t hvpr_augment_points_workspace_bytes(int n_frames, int max_frame_points, int n_candidates, long long n_points) {
    if (n_frames < 1 || max_frame_points < 0 || n_candidates < 0 || n_points < 0) return 0;
    return points_ws(nullptr, n_frames, std::max(1, hvpr_cdiv(max_frame_points, kBlk)), n_candidates, n_points).bytes;
}

extern "C" int hvpr_augment_points_f32(const int32_t *plan_host, const int32_t *plan_dev, int plan_words, const int32_t *valid,
                                       const float *points, long long n_points, int point_floats, const float *bank_points,
                                       long long bank_rows, const float *bank_boxes, int n_objects, int bank_floats,
                                       const float *extra_width3, float *out_points, long long out_capacity, int32_t *out_off,
                                       void *workspace, size_t workspace_bytes, hvpr_stream_t stream) {
    Plan h, d;
    if (const int st = plan_open(plan_host, plan_dev, plan_words, h, d)) return st;
    if (n_points < 0 || point_floats < 3 || bank_rows < 0 || n_objects < 0 || !extra_width3 || !out_off || !workspace ||
        (n_points > 0 && !points) || (h.C > 0 && (!valid || !bank_boxes)) || (bank_rows > 0 && !bank_points))
        return HVPR_ERR_INVALID_ARG;
    if (bank_floats != point_floats) return HVPR_ERR_INVALID_ARG;            // one feature width for scene and bank
    if (h.pt_off[h.B] != n_points) return HVPR_ERR_INVALID_ARG;
    long long upper = n_points;
    for (int c = 0; c < h.C; ++c) {
        if (h.cand_obj[c] < 0 || h.cand_obj[c] >= n_objects || h.cand_start[c] < 0 || h.cand_n[c] < 0 ||
            (long long)h.cand_start[c] + h.cand_n[c] > bank_rows)
            return HVPR_ERR_INVALID_ARG;
        upper += h.cand_n[c];
    }
    if (upper > 0x7fffffffLL) return HVPR_ERR_UNSUPPORTED;                   // 32-bit row offsets
    if (out_capacity < upper || (upper > 0 && !out_points)) return HVPR_ERR_INVALID_ARG;
    for (int f = 0; f < h.B; ++f)
        if (h.grp_off[(f + 1) * h.NG] - h.grp_off[f * h.NG] > kFrameBoxes) return HVPR_ERR_UNSUPPORTED;
    const int max_blk = max_frame_blocks(h);
    const PointsWs w = points_ws(workspace, h.B, max_blk, h.C, n_points);
    if (workspace_bytes < w.bytes) return HVPR_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(max_blk, h.B);
    hipLaunchKernelGGL(k_points_count, grid, dim3(kBlk), 0, s, d, valid, points, point_floats, extra_width3[0], extra_width3[1],
                       extra_width3[2], w.flag, w.blk_cnt);
    HVPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_points_scan, dim3(1), dim3(256), 0, s, d, valid, w.blk_cnt, max_blk, w.blk_pre, w.cand_pre, out_off);
    HVPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_points_write_scene, grid, dim3(kBlk), 0, s, d, points, point_floats, w.flag, w.blk_pre, w.cand_pre, out_off,
                       out_points);
    HVPR_CHECK_LAUNCH();
    if (h.C > 0) {
        hipLaunchKernelGGL(k_points_write_cand, dim3(h.C), dim3(256), 0, s, d, valid, bank_points, bank_boxes, point_floats, w.cand_pre,
                           out_off, out_points);
        HVPR_CHECK_LAUNCH();
    }
    return HVPR_OK;
}
