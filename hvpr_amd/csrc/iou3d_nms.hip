// a8 — rotated-BEV overlap / IoU / 3D IoU / NMS on device.  Replaces the reference's absent native module
// pcdet/ops/iou3d_nms (sources named by setup.py:53-62; call sites: model_utils/model_nms_utils.py:17-19,
// detectors/detector3d_template.py:298,303).  Boxes are [x, y, z, dx, dy, dz, heading].
//
// The geometry follows, operation for operation, the same fp32 sequence as the CPU oracle
// (oracle/iou3d_nms_ref.c): both are compiled with -ffp-contract=off so that survivor ids are bit-exact.
// MI355X-specific parts: 64 x 64 tiles = one wave per tile and one 64-bit mask word per lane; an exact
// circum-circle reject (no polygon work for far-apart pairs: overlap is exactly 0 there); the sequential sweep
// runs ON DEVICE in one wave (mask words live in lanes, diagonal block resolved with readlane, rows of kept
// boxes OR-ed in with independent coalesced loads) — no mask copy to the host, no host loop, no sync.
#include "common.h"
#include "iou_geom.h"     // P2, Box, PolyStore, box_overlap, iou_bev: shared with augment.hip

namespace {

// ---- pairwise (N,M) kernels: mode 0 overlap, 1 bev iou, 2 3d iou -----------------------------------------
__global__ void __launch_bounds__(64) k_pairwise(const float *__restrict__ a, int n, const float *__restrict__ b, int m,
                                                 int mode, float *__restrict__ out) {
    __shared__ PolyStore ps;
    const int ln = threadIdx.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * m) return;
    const int i = (int)(t / m), j = (int)(t % m);
    const float *pa = a + (size_t)i * 7, *pb = b + (size_t)j * 7;
    Box A, B;
    make_box(pa, A);
    make_box(pb, B);
    float r;
    if (mode == 0) r = box_overlap(A, B, ps, ln);
    else if (mode == 1) r = iou_bev(A, B, ps, ln);
    else r = iou_3d(pa, pb, A, B, ps, ln);
    out[t] = r;
}

// Ragged form of mode 0: F independent (n_f, m_f) problems packed end to end in ONE launch.  Pair p of frame f (pair_off[f] <= p <
// pair_off[f + 1], frames without pairs own nothing) is (i, j) = divmod(p - pair_off[f], m_f): row a_off[f] + i of table A against
// row b_off[f] + j of table B.  A pair is one lane running the same make_box / box_overlap sequence on the same two rows as in
// k_pairwise, so out[pair_off[f] ...] holds exactly the bits hvpr_boxes_pairwise_f32 gives for frame f alone.
__global__ void __launch_bounds__(64) k_pairwise_ragged(const float *__restrict__ a, const float *__restrict__ b,
                                                        const int64_t *__restrict__ a_off, const int64_t *__restrict__ b_off,
                                                        const int64_t *__restrict__ pair_off, int n_frames, long long n_pairs,
                                                        float *__restrict__ out) {
    __shared__ PolyStore ps;
    const int ln = threadIdx.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pairs) return;
    int lo = 0, hi = n_frames;                           // the largest f with pair_off[f] <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= t) lo = mid; else hi = mid;
    }
    const long long m = b_off[lo + 1] - b_off[lo], r = t - pair_off[lo];
    Box A, B;
    make_box(a + (size_t)(a_off[lo] + r / m) * 7, A);
    make_box(b + (size_t)(b_off[lo] + r % m) * 7, B);
    out[t] = box_overlap(A, B, ps, ln);
}

// ---- NMS: the segments of one call -------------------------------------------------------------------------
// A call holds S independent candidate lists (frames, or the classes of a frame that rank one box table).  The segment is the last
// grid dimension of every kernel below; a kernel finds everything that belongs to its segment from the segment id: the live count,
// the order row, the box table, and the segment's private copy of the workspace (mask | prepared boxes | per-tile pair segments |
// pair counts | ClipIndex, each part 256-byte aligned).  S = 1 is the single-list call, launch for launch.
constexpr int kTileCap = 64 * 64;                     // pairs a tile can hold
constexpr int kMaxTiles = 2080;                       // nb <= 64
struct ClipIndex { int pre[kMaxTiles + 1]; unsigned char rb[kMaxTiles], cb[kMaxTiles]; };

struct NmsCall {
    const float *boxes; int box_stride; long long table_stride; int segs_per_table;
    const int *order, *n_device;
    int n_segments, n_max, nb;
    char *ws; size_t seg_bytes, off_prepared, off_plist, off_pcount, off_ci;

    __device__ __forceinline__ int n(int s) const { return n_device ? min(n_device[s], n_max) : n_max; }
    __device__ __forceinline__ const int *order_row(int s) const { return order ? order + (size_t)s * n_max : nullptr; }
    __device__ __forceinline__ const float *table(int s) const { return boxes + (long long)(s / segs_per_table) * table_stride; }
    __device__ __forceinline__ unsigned long long *mask(int s) const { return (unsigned long long *)(ws + (size_t)s * seg_bytes); }
    __device__ __forceinline__ Box *prepared(int s) const { return (Box *)(ws + (size_t)s * seg_bytes + off_prepared); }
    __device__ __forceinline__ unsigned short *plist(int s) const { return (unsigned short *)(ws + (size_t)s * seg_bytes + off_plist); }
    __device__ __forceinline__ int *pcount(int s) const { return (int *)(ws + (size_t)s * seg_bytes + off_pcount); }
    __device__ __forceinline__ ClipIndex *clip_index(int s) const { return (ClipIndex *)(ws + (size_t)s * seg_bytes + off_ci); }
};

// ---- NMS: bit-mask tiles -------------------------------------------------------------------------------
// k_nms_prep: candidate i = boxes[order ? order[i] : i] -> Box (corners + sin/cos computed once per box, not once per tile)
__global__ void __launch_bounds__(256) k_nms_prep(const NmsCall nc) {
    const int seg = blockIdx.y;
    const int n = nc.n(seg);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int *order = nc.order_row(seg);
    Box B;
    make_box(nc.table(seg) + (size_t)(order ? order[i] : i) * nc.box_stride, B);
    nc.prepared(seg)[i] = B;
}

// One wave per 64 x 64 tile.  Phase 1: every lane tests its row box against the 64 column boxes with the two exact
// rejects only (circum-circle, then separating axes: a few flops on a 32-byte box record).  Phase 2: the surviving (row, col) pairs of the whole tile are compacted into
// LDS and dealt out to the lanes round-robin, so the expensive polygon clip runs on densely packed lanes instead of
// 64 divergent column iterations.  Results are identical to testing every pair (the reject is exact).
__global__ void __launch_bounds__(64) k_nms_mask(const NmsCall nc, float thresh) {
    const int seg = blockIdx.z, nb = nc.nb;
    const int n = nc.n(seg);
    const Box *__restrict__ prepared = nc.prepared(seg);
    unsigned long long *__restrict__ mask = nc.mask(seg);
    const int rb = blockIdx.y, cb = blockIdx.x;
    const int t = threadIdx.x;
    const int row = rb * 64 + t;
    if (rb * 64 >= n || cb * 64 >= n) return;
    if (cb < rb) {
        if (row < n) mask[(size_t)row * nb + cb] = 0ull;
        return;
    }
    __shared__ Box s_row[64], s_col[64];
    __shared__ __attribute__((aligned(16))) BoxLite s_lrow[64], s_lcol[64];
    __shared__ __attribute__((aligned(16))) float4 s_circ[64];   // column boxes: centre and circum-radius
    __shared__ unsigned long long s_bits[64];
    __shared__ unsigned short s_pairs[64 * 32];   // one half of the columns at a time: 37 KB of LDS = four tiles per CU
    __shared__ PolyStore ps;
    const int col = cb * 64 + t;
    if (row < n) s_row[t] = prepared[row];
    if (row < n) s_lrow[t] = lite_of(s_row[t]);
    if (col < n) {
        s_col[t] = prepared[col];
        s_lcol[t] = lite_of(s_col[t]);
        s_circ[t] = make_float4(s_lcol[t].x, s_lcol[t].y, s_lcol[t].rad, 0.f);
    }
    s_bits[t] = 0ull;
    __syncthreads();
    const int ncol = min(64, n - cb * 64);
    HVPR_IF_TIMING(const long long tq0 = __builtin_readcyclecounter();)
    int total2_all = 0;   // (only the HVPR_EXP_TIMING build reports it)
    (void)total2_all;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int c_lo = 32 * half;
        unsigned near = 0u;
        if (row < n) {   // reject no. 1 (the circum-circle test of far_apart()), one broadcast 16-byte LDS read per column box
            const float mx = s_lrow[t].x, my = s_lrow[t].y, mr = s_lrow[t].rad + 0.05f;
            const int i0 = (rb == cb) ? t + 1 : 0;
#pragma unroll 8
            for (int i = 0; i < 32; ++i) {
                const float4 c = s_circ[c_lo + i];
                const float ddx = mx - c.x, ddy = my - c.y, lim = mr + c.z;
                const bool close = !(ddx * ddx + ddy * ddy > lim * lim * 1.0001f);
                if (close && c_lo + i >= i0 && c_lo + i < ncol) near |= 1u << i;
            }
        }
        // exclusive prefix of the per-lane pair counts
        const int cnt = __popc(near);
        const int incl = hvpr_wave_scan_incl(cnt);
        const int total = __shfl(incl, 63, 64);
        int pos = incl - cnt;
        while (near) {
            const int i = __ffs((int)near) - 1;
            near &= near - 1;
            s_pairs[pos++] = (unsigned short)((t << 6) | (c_lo + i));
        }
        __syncthreads();
        // reject no. 2 (separating axes) on the packed pair list, compacted in place (one wave: writes trail reads)
        int total2 = 0;
        for (int k0 = 0; k0 < total; k0 += 64) {
            const int k = k0 + t;
            const int pr = k < total ? s_pairs[k] : 0;
            const bool keep = k < total && !axes_separate(s_lrow[pr >> 6], s_lcol[pr & 63]);
            const unsigned long long m = __ballot(keep);
            if (keep) s_pairs[total2 + __popcll(m & ((1ull << t) - 1ull))] = (unsigned short)pr;
            total2 += __popcll(m);
        }
        __syncthreads();
        for (int k = t; k < total2; k += 64) {
            const int pr = s_pairs[k];
            const int r = pr >> 6, c = pr & 63;
            if (iou_bev(s_row[r], s_col[c], ps, t) > thresh) atomicOr(&s_bits[r], 1ull << c);
        }
        __syncthreads();
        total2_all += total2;
    }
    __syncthreads();
    HVPR_IF_TIMING(if (t == 0 && rb % 8 == 0 && cb % 8 == 0)
        printf("nms tile %d %d: %d pairs clipped, %lld cycles\n", rb, cb, total2_all, (long long)__builtin_readcyclecounter() - tq0);)
    if (row < n) mask[(size_t)row * nb + cb] = s_bits[t];
}

// ---- NMS mask in two launches (n <= 4096): the rejects per tile, then the polygon clips over ONE balanced list --------------
// k_nms_mask above clips a tile's surviving pairs inside the tile's wave: tiles in dense regions of the scene hold thousands of
// pairs, tiles elsewhere none, and the launch lasts as long as its heaviest tiles (97 us for 4096 candidates of which the rejects
// leave a few 10^4 pairs).  Here the tile waves only run the two exact rejects and write their survivors to a per-tile segment of
// a global list (no atomics); k_nms_clip then walks the concatenation of all segments with every lane of the chip holding the
// same number of pairs, and sets the mask bits with atomicOr (order-independent: the mask, and with it the survivors, are
// identical to the one-launch form).
__host__ __device__ inline int tri_index(int rb, int cb, int nb) { return rb * nb - rb * (rb - 1) / 2 + (cb - rb); }

__global__ void __launch_bounds__(64) k_nms_pairs(const NmsCall nc) {
    const int seg = blockIdx.z, nb = nc.nb;
    const int n = nc.n(seg);
    const Box *__restrict__ prepared = nc.prepared(seg);
    unsigned long long *__restrict__ mask = nc.mask(seg);
    unsigned short *__restrict__ plist = nc.plist(seg);
    int *__restrict__ pcount = nc.pcount(seg);
    const int rb = blockIdx.y, cb = blockIdx.x;
    const int t = threadIdx.x;
    const int row = rb * 64 + t;
    if (rb * 64 >= n || cb * 64 >= n) return;
    if (row < n) mask[(size_t)row * nb + cb] = 0ull;      // k_nms_clip ORs the suppression bits in
    if (cb < rb) return;
    __shared__ __attribute__((aligned(16))) BoxLite s_lrow[64], s_lcol[64];
    __shared__ __attribute__((aligned(16))) float4 s_circ[64];   // column boxes: centre and circum-radius
    __shared__ unsigned short s_pairs[64 * 32];
    const int col = cb * 64 + t;
    if (row < n) s_lrow[t] = lite_of(prepared[row]);
    if (col < n) {
        s_lcol[t] = lite_of(prepared[col]);
        s_circ[t] = make_float4(s_lcol[t].x, s_lcol[t].y, s_lcol[t].rad, 0.f);
    }
    __syncthreads();
    const int ncol = min(64, n - cb * 64);
    const int tile = tri_index(rb, cb, nb);
    unsigned short *out = plist + (size_t)tile * kTileCap;
    int n_out = 0;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int c_lo = 32 * half;
        unsigned near = 0u;
        if (row < n) {   // reject no. 1 (the circum-circle test of far_apart())
            const float mx = s_lrow[t].x, my = s_lrow[t].y, mr = s_lrow[t].rad + 0.05f;
            const int i0 = (rb == cb) ? t + 1 : 0;
#pragma unroll 8
            for (int i = 0; i < 32; ++i) {
                const float4 c = s_circ[c_lo + i];
                const float ddx = mx - c.x, ddy = my - c.y, lim = mr + c.z;
                const bool close = !(ddx * ddx + ddy * ddy > lim * lim * 1.0001f);
                if (close && c_lo + i >= i0 && c_lo + i < ncol) near |= 1u << i;
            }
        }
        const int cnt = __popc(near);
        const int incl = hvpr_wave_scan_incl(cnt);
        const int total = __shfl(incl, 63, 64);
        int pos = incl - cnt;
        while (near) {
            const int i = __ffs((int)near) - 1;
            near &= near - 1;
            s_pairs[pos++] = (unsigned short)((t << 6) | (c_lo + i));
        }
        __syncthreads();
        // reject no. 2 (separating axes) on the packed pair list; survivors go to the tile's global segment
        for (int k0 = 0; k0 < total; k0 += 64) {
            const int k = k0 + t;
            const int pr = k < total ? s_pairs[k] : 0;
            const bool keep = k < total && !axes_separate(s_lrow[pr >> 6], s_lcol[pr & 63]);
            const unsigned long long m = __ballot(keep);
            if (keep) out[n_out + __popcll(m & ((1ull << t) - 1ull))] = (unsigned short)pr;
            n_out += __popcll(m);
        }
        __syncthreads();
    }
    if (t == 0) pcount[tile] = n_out;
}

// exclusive prefix of the live tiles' pair counts, in (rb, cb >= rb) order, + the tile of every position: one workgroup per segment
__global__ void __launch_bounds__(1024) k_nms_scan(const NmsCall nc) {
    __shared__ int s_wave[16];
    const int seg = blockIdx.x, nb = nc.nb;
    const int n = nc.n(seg);
    const int *__restrict__ pcount = nc.pcount(seg);
    ClipIndex *__restrict__ ci = nc.clip_index(seg);
    const int nba = (n + 63) / 64, n_tiles = nba * (nba + 1) / 2;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    // thread t owns live tiles 3t .. 3t + 2  (3 * 1024 >= 2080)
    int rb = 0, rem = 3 * t;
    while (rb < nba && rem >= nba - rb) { rem -= nba - rb; ++rb; }
    int cb = rb + rem;
    int c[3], trb[3], tcb[3], run = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool live = 3 * t + i < n_tiles;
        trb[i] = rb; tcb[i] = cb;
        c[i] = live ? pcount[tri_index(rb, cb, nb)] : 0;
        run += c[i];
        if (live && ++cb == nba) { ++rb; cb = rb; }
    }
    const int incl = hvpr_wave_scan_incl(run);
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    int base = incl - run;
    for (int w = 0; w < wid; ++w) base += s_wave[w];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (3 * t + i < n_tiles) {
            ci->pre[3 * t + i] = base;
            ci->rb[3 * t + i] = (unsigned char)trb[i]; ci->cb[3 * t + i] = (unsigned char)tcb[i];
        }
        base += c[i];
    }
    if (t == 1023) ci->pre[n_tiles] = base;
}

constexpr int kClipThreads = 128, kClipBlocks = 768;  // three workgroups per CU (a PolyStore per wave, 49 KB of LDS each)
// Several segments share ONE grid of about kClipBlocks workgroups (S grids of that size would each reload a 12 KB ClipIndex for a
// sliver of work, and the chip holds 768 of these workgroups at a time anyway).  Every workgroup serves one segment, and a
// segment gets workgroups in proportion to the pairs it has to clip: one for being non-empty plus its floor share of the
// gridDim.x - S others, so an empty frame costs nothing and a crowded one is not left to a fixed 1/S of the chip.  All
// workgroups derive the same split from the S totals the scan left behind (wave 0: a prefix sum over the segments); workgroups
// the floors leave over exit.  With one segment the split is the whole grid, as before.
__device__ __forceinline__ int clip_total(const NmsCall &nc, int s) {
    const int nba = (nc.n(s) + 63) / 64;
    return nc.clip_index(s)->pre[nba * (nba + 1) / 2];
}

__global__ void __launch_bounds__(kClipThreads) k_nms_clip(const NmsCall nc, float thresh) {
    __shared__ int s_pre[kMaxTiles + 1];
    __shared__ unsigned char s_rb[kMaxTiles], s_cb[kMaxTiles];
    __shared__ PolyStore ps[kClipThreads / 64];
    __shared__ int s_split[3];                        // segment, its first workgroup, its workgroup count
    const int t = threadIdx.x;
    int seg = 0, wg = blockIdx.x, n_wg = gridDim.x;
    if (nc.n_segments > 1) {
        if (t == 0) s_split[0] = -1;
        if (t < 64) {
            const int S = nc.n_segments, spare = (int)gridDim.x - S;
            long long all = 0;
            for (int s = t; s < S; s += 64) all += clip_total(nc, s);
            HVPR_WAVE_SUM_XOR(all);
            int base = 0;
            for (int s0 = 0; s0 < S; s0 += 64) {
                const int s = s0 + t;
                const int tot = s < S ? clip_total(nc, s) : 0;
                const int mine = tot > 0 ? 1 + (int)((long long)spare * tot / all) : 0;
                const int incl = hvpr_wave_scan_incl(mine);
                const int first = base + incl - mine;
                if ((int)blockIdx.x >= first && (int)blockIdx.x < first + mine) { s_split[0] = s; s_split[1] = first; s_split[2] = mine; }
                base += __shfl(incl, 63, 64);
            }
        }
        __syncthreads();
        if (s_split[0] < 0) return;
        seg = s_split[0]; wg = (int)blockIdx.x - s_split[1]; n_wg = s_split[2];
    }
    const int nb = nc.nb;
    const Box *__restrict__ prepared = nc.prepared(seg);
    unsigned long long *__restrict__ mask = nc.mask(seg);
    const unsigned short *__restrict__ plist = nc.plist(seg);
    const ClipIndex *__restrict__ ci = nc.clip_index(seg);
    const int n = nc.n(seg);
    const int nba = (n + 63) / 64, n_tiles = nba * (nba + 1) / 2;
    for (int i = t; i <= n_tiles; i += kClipThreads) s_pre[i] = ci->pre[i];
    for (int i = t; i < n_tiles; i += kClipThreads) { s_rb[i] = ci->rb[i]; s_cb[i] = ci->cb[i]; }
    __syncthreads();
    const int total = s_pre[n_tiles];
    PolyStore &my = ps[t >> 6];
    for (long long gidx = (long long)wg * kClipThreads + t; gidx < total; gidx += (long long)n_wg * kClipThreads) {
        // the tile holding pair gidx: largest i with s_pre[i] <= gidx
        int lo = 0, hi = n_tiles;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_pre[mid] <= (int)gidx) lo = mid; else hi = mid;
        }
        const int rb = s_rb[lo], cb = s_cb[lo];
        const int pr = plist[(size_t)tri_index(rb, cb, nb) * kTileCap + ((int)gidx - s_pre[lo])];
        const int row = rb * 64 + (pr >> 6), c = pr & 63;
        const Box A = prepared[row], B = prepared[cb * 64 + c];
        if (iou_bev(A, B, my, t & 63) > thresh) atomicOr(&mask[(size_t)row * nb + cb], 1ull << c);
    }
}

// ---- NMS: sequential sweep, one wave ----------------------------------------------------------------------
// keep[] receives positions in the sorted order (or order[pos] when `order` is given and map_through_order != 0).
__global__ void __launch_bounds__(64) k_nms_sweep(const NmsCall nc, int map_through_order, int max_keep,
                                                  int *__restrict__ keep_all, int *__restrict__ keep_count) {
    const int seg = blockIdx.x, nb_stride = nc.nb;
    const unsigned long long *__restrict__ mask = nc.mask(seg);
    const int *__restrict__ order = nc.order_row(seg);
    int *__restrict__ keep = keep_all + (size_t)seg * max_keep;
    const int n = nc.n(seg);
    const int lane = threadIdx.x;
    const int nb = (n + 63) / 64;
    int kept = 0;
    // remv words: lane w owns word w of chunk (w / 64); n_max <= 64*64*? -> up to NW words per lane
    constexpr int NW = 4;   // supports n <= 64 * 64 * NW = 16384
    unsigned long long remv[NW] = {0ull, 0ull, 0ull, 0ull};
    // diagonal words of the first 64 blocks are fetched up front (64 independent loads per lane), so the per-block
    // critical path is the resolve loop plus ONE batch of row loads
    constexpr int NPRE = 64;
    unsigned long long dpre[NPRE];
#pragma unroll
    for (int b = 0; b < NPRE; ++b) {
        const int row = b * 64 + lane;
        dpre[b] = (b < nb && row < n) ? mask[(size_t)row * nb_stride + b] : 0ull;
    }
    for (int b = 0; b < nb && kept < max_keep; ++b) {
        const int row = b * 64 + lane;
        unsigned long long diag = 0ull;
        if (b < NPRE) {
#pragma unroll
            for (int q = 0; q < NPRE; ++q) if (q == b) diag = dpre[q];
        } else {
            diag = row < n ? mask[(size_t)row * nb_stride + b] : 0ull;
        }
        // remv word of this block (uniform)
        unsigned long long rw = 0ull;
#pragma unroll
        for (int q = 0; q < NW; ++q)
            if ((b >> 6) == q) {
                const unsigned lo = __builtin_amdgcn_readlane((unsigned)(remv[q] & 0xffffffffull), b & 63);
                const unsigned hi = __builtin_amdgcn_readlane((unsigned)(remv[q] >> 32), b & 63);
                rw = ((unsigned long long)hi << 32) | lo;
            }
        unsigned long long kbits = 0ull;
        const int lim = min(64, n - b * 64);
        for (int i = 0; i < lim && kept < max_keep; ++i) {
            if (!((rw >> i) & 1ull)) {
                kbits |= 1ull << i;
                const unsigned lo = __builtin_amdgcn_readlane((unsigned)(diag & 0xffffffffull), i);
                const unsigned hi = __builtin_amdgcn_readlane((unsigned)(diag >> 32), i);
                rw |= ((unsigned long long)hi << 32) | lo;
                ++kept;
            }
        }
        // kept positions of this block -> keep[] (lane i writes its own entry)
        {
            const int base = kept - __popcll(kbits);
            if ((kbits >> lane) & 1ull) {
                const int pos = b * 64 + lane;
                keep[base + __popcll(kbits & ((1ull << lane) - 1ull))] = (order && map_through_order) ? order[pos] : pos;
            }
        }
        // OR the rows of the kept boxes into the later words: eight independent coalesced row loads in flight
        unsigned long long kb = kbits;
        while (kb) {
            int idx8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                idx8[u] = kb ? __ffsll((long long)kb) - 1 : -1;
                kb &= kb - 1;
            }
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                const int w = q * 64 + lane;
                if (q * 64 < nb && w > b && w < nb) {
                    unsigned long long t8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        t8[u] = idx8[u] >= 0 ? mask[(size_t)(b * 64 + idx8[u]) * nb_stride + w] : 0ull;
                    remv[q] |= ((t8[0] | t8[1]) | (t8[2] | t8[3])) | ((t8[4] | t8[5]) | (t8[6] | t8[7]));
                }
            }
        }
    }
    if (lane == 0) keep_count[seg] = kept;
}

// The greedy sweep for n <= 4096 candidates (nb <= 64 mask words per row).  The sweep is serial over the 64-box blocks and
// needs, per block, the mask rows of the boxes it keeps: read on demand that is one dependent L2 round trip per block
// (64 x ~3.5 us).  Here one workgroup of 8 waves streams ALL rows through an LDS ring, one block (64 rows x nb words, 32 KB)
// per phase, and wave 0 resolves phase p out of LDS.  Four of the eight loader waves OWN the phases p = g (mod 2), 16 rows
// each: they request the rows of their next phase two phases before they are needed and keep them in registers until the
// ring slot is free — two L2 round trips in flight, the barriers wait for LDS only (rounds 1-3: all loaders fetched phase
// p + 1 during phase p behind __syncthreads(), whose vmcnt(0) made every phase one round trip long: 71 us; now 59, bound
// by the ~300 dependent instructions wave 0 spends per block; more loader waves slow that wave down: 13 waves 63 us).  The
// diagonal words and the candidate ids travel through LDS too (a column read of the ring is a 64-way bank conflict, order[]
// a dependent global load).  Same greedy order, same result.
constexpr int kRingThreads = 576;                    // the resolving wave + 8 loaders
constexpr int kRingOwners = 4;                       // loader waves that share a phase (16 rows each)
constexpr int kRingDepth = (kRingThreads / 64 - 1) / kRingOwners;     // 2 phases in flight
constexpr int kRingWords = 64;                       // words per row in LDS (nb <= 64)
constexpr int kRingPieces = (64 / kRingOwners) * (kRingWords / 2) / 64;   // 16-byte pieces per lane and phase: 8

__global__ void __launch_bounds__(kRingThreads) k_nms_sweep_ring(const NmsCall nc, int map_through_order, int max_keep,
                                                                 int *__restrict__ keep_all, int *__restrict__ keep_count) {
    const int seg = blockIdx.x, nb_stride = nc.nb, n_max = nc.n_max;
    const unsigned long long *__restrict__ mask = nc.mask(seg);
    const int *__restrict__ order = nc.order_row(seg);
    int *__restrict__ keep = keep_all + (size_t)seg * max_keep;
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_rows[];   // [2][64][kRingWords]
    __shared__ int s_done;
    // per ring slot: the diagonal word of every row (row r of block b, word b: a column of s_rows — 64 lanes on one bank) and the
    // candidates' ids, so that the resolve reads both without a bank conflict / without a dependent global load
    __shared__ unsigned long long s_diag[2][64];
    __shared__ int s_ord[2][64];
    const int n = nc.n(seg);
    const int nb = (n + 63) / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // a loader lane holds pieces (row 32 * half + 2u + lane / 32, words 2c, 2c + 1 with c = lane % 32), u = 0..15, of its phase
    ulonglong2 v[kRingPieces];
    int ord = 0;
    const bool ord_lane = order && map_through_order && wid != 0 && (wid - 1) % kRingOwners == 0;
    const int pr = (lane >> 5) + (64 / kRingOwners) * ((wid - 1) % kRingOwners), pc = lane & 31, grp = (wid - 1) / kRingOwners;
    // global -> registers: 32 UNCONDITIONAL loads back to back, no select on an address or a result (the compiler turns those into
    // a branch and a wait per load).  What is not wanted is never looked at by the resolve, so it may hold anything: rows past n
    // (clamped to the last row of the buffer), words left of the diagonal block (the lower triangle; those lanes fetch the
    // diagonal piece again — same cache line, no extra traffic) and words past nb.
    const bool even = !(nb_stride & 1);             // 16-byte aligned pieces whose two words both exist
    auto request = [&](int ph) {
        const int pcc = max(pc, (ph - 1) >> 1);
        if (ord_lane) ord = order[min(ph * 64 + lane, n_max - 1)];
        if (even) {
            const int col = 2 * min(pcc, (nb_stride >> 1) - 1);
#pragma unroll
            for (int u = 0; u < kRingPieces; ++u)
                v[u] = *(const ulonglong2 *)(mask + (size_t)min(ph * 64 + 2 * u + pr, n_max - 1) * nb_stride + col);
        } else {
            const int c0 = min(2 * pcc, nb_stride - 1), c1 = min(2 * pcc + 1, nb_stride - 1);
#pragma unroll
            for (int u = 0; u < kRingPieces; ++u) {
                const size_t base = (size_t)min(ph * 64 + 2 * u + pr, n_max - 1) * nb_stride;
                v[u].x = mask[base + c0];
                v[u].y = mask[base + c1];
            }
        }
    };
    auto commit = [&](int ph) {         // registers -> ring slot ph & 1
        unsigned long long *dst = s_rows + (size_t)(ph & 1) * 64 * kRingWords;
#pragma unroll
        for (int u = 0; u < kRingPieces; ++u) *(ulonglong2 *)(dst + (size_t)(2 * u + pr) * kRingWords + 2 * pc) = v[u];
        if (pc == (ph >> 1)) {
            // (bit masks, not `odd ? v.y : v.x`: the compiler turns that select into a dynamic index and the whole array into scratch)
            const unsigned long long odd = 0ull - (unsigned long long)(ph & 1);
#pragma unroll
            for (int u = 0; u < kRingPieces; ++u) s_diag[ph & 1][2 * u + pr] = (v[u].x & ~odd) | (v[u].y & odd);
        }
        if (ord_lane) s_ord[ph & 1][lane] = ord;
    };
    if (tid == 0) s_done = 0;
    if (wid != 0) request(grp);         // phases 0..3
    if (wid != 0 && grp == 0) { commit(0); request(kRingDepth); }
    // The barriers of this kernel order LDS traffic only: __syncthreads() would also wait for every outstanding GLOBAL load of the
    // wave (vmcnt(0)) — exactly the round trip per phase the ring is there to hide.  The loaded registers are guarded by the
    // compiler's own vmcnt waits at their first use (commit).
    auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    lds_barrier();
    unsigned long long remv = 0ull;                  // wave 0: lane w owns suppression word w
    int kept = 0;
    for (int ph = 0; ph < nb; ++ph) {
        if (wid != 0) {
            // the owner of phase ph + 1 hands it over (its slot was read last in phase ph - 1) and requests its next one
            if ((ph + 1) % kRingDepth == grp && ph + 1 < nb && !s_done) {
                commit(ph + 1);
                request(ph + 1 + kRingDepth);
            }
        } else if (kept < max_keep) {
            const unsigned long long *rows = s_rows + (size_t)(ph & 1) * 64 * kRingWords;
            const int b = ph;
            const unsigned long long diag = s_diag[ph & 1][lane];                  // row `lane` of block b, word b
            const int my_id = (order && map_through_order) ? s_ord[ph & 1][lane] : b * 64 + lane;
            unsigned long long rw;
            {
                const unsigned lo = __builtin_amdgcn_readlane((unsigned)(remv & 0xffffffffull), b);
                const unsigned hi = __builtin_amdgcn_readlane((unsigned)(remv >> 32), b);
                rw = ((unsigned long long)hi << 32) | lo;
            }
            const int lim = min(64, n - b * 64);
            const unsigned long long valid = lim == 64 ? ~0ull : ((1ull << lim) - 1ull);
            unsigned long long kbits = 0ull;
            unsigned long long avail = ~rw & valid;
            while (avail && kept < max_keep) {                 // only unsuppressed candidates are visited
                const int i = __ffsll((long long)avail) - 1;
                kbits |= 1ull << i;
                const unsigned lo = __builtin_amdgcn_readlane((unsigned)(diag & 0xffffffffull), i);
                const unsigned hi = __builtin_amdgcn_readlane((unsigned)(diag >> 32), i);
                rw |= ((unsigned long long)hi << 32) | lo;
                ++kept;
                avail = ~rw & valid & ~((2ull << i) - 1ull);
            }
            const int base = kept - __popcll(kbits);
            if ((kbits >> lane) & 1ull) keep[base + __popcll(kbits & ((1ull << lane) - 1ull))] = my_id;
            // rows of the kept boxes, straight from LDS, four at a time: the reads of a round are issued together (one LDS
            // latency per round instead of one per kept box)
            for (unsigned long long kb = kbits; kb;) {
                unsigned long long t4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = kb ? __ffsll((long long)kb) - 1 : -1;
                    kb &= kb - 1ull;
                    t4[u] = i >= 0 ? rows[(size_t)i * kRingWords + lane] : 0ull;
                }
                remv |= (t4[0] | t4[1]) | (t4[2] | t4[3]);
            }
            if (kept >= max_keep && lane == 0) s_done = 1;
        }
        lds_barrier();
    }
    if (tid == 0) keep_count[seg] = kept;
}

}  // namespace

extern "C" int hvpr_boxes_pairwise_f32(const float *boxes_a, int n, const float *boxes_b, int m, int mode, float *out,
                                       hvpr_stream_t stream) {
    if (n < 0 || m < 0 || mode < 0 || mode > 2) return HVPR_ERR_INVALID_ARG;
    if (n == 0 || m == 0) return HVPR_OK;
    if (!boxes_a || !boxes_b || !out) return HVPR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_pairwise, dim3(hvpr_cdiv((long long)n * m, 64)), dim3(64), 0, (hipStream_t)stream, boxes_a, n,
                       boxes_b, m, mode, out);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_boxes_pairwise_ragged_f32(const float *boxes_a, const float *boxes_b, const int64_t *a_off, const int64_t *b_off,
                                              const int64_t *pair_off, int n_frames, long long n_pairs, float *out,
                                              hvpr_stream_t stream) {
    if (n_frames < 0 || n_pairs < 0 || n_pairs > (1ll << 36)) return HVPR_ERR_INVALID_ARG;
    if (n_frames == 0 || n_pairs == 0) return HVPR_OK;
    if (!boxes_a || !boxes_b || !a_off || !b_off || !pair_off || !out) return HVPR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_pairwise_ragged, dim3(hvpr_cdiv(n_pairs, 64)), dim3(64), 0, (hipStream_t)stream, boxes_a, boxes_b, a_off,
                       b_off, pair_off, n_frames, n_pairs, out);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" size_t hvpr_nms_workspace_bytes(int n_max) {
    if (n_max < 1) return 0;
    const size_t nb = (n_max + 63) / 64;
    size_t bytes = (size_t)n_max * nb * sizeof(unsigned long long) + 256 + (size_t)n_max * sizeof(Box) + 256;
    // the two-launch mask (nb <= 64): per-tile pair segments + counts.  Past 4096 they are reserved at their largest too, so
    // that the size grows with n_max and a workspace serves every n_max up to the one it was sized for.
    const size_t nbl = nb < 64 ? nb : 64, tiles = nbl * (nbl + 1) / 2;
    bytes += tiles * kTileCap * sizeof(unsigned short) + 256 + tiles * sizeof(int) + 256 + sizeof(ClipIndex) + 256;
    return bytes;
}

// segment s of a call owns workspace bytes [s * stride, s * stride + hvpr_nms_workspace_bytes(n_max))
static size_t nms_segment_stride(int n_max) { return (hvpr_nms_workspace_bytes(n_max) + 255) / 256 * 256; }

extern "C" size_t hvpr_nms_bev_batched_workspace_bytes(int n_segments, int n_max) {
    if (n_segments < 1 || n_max < 1) return 0;
    return (size_t)(n_segments - 1) * nms_segment_stride(n_max) + hvpr_nms_workspace_bytes(n_max);
}

extern "C" int hvpr_nms_bev_batched_f32(const float *boxes, int box_stride, long long table_stride, int segments_per_table,
                                        const int32_t *order, const int32_t *n_device, int n_segments, int n_max, float thresh,
                                        int max_keep, int map_through_order, int32_t *keep, int32_t *keep_count, void *workspace,
                                        size_t workspace_bytes, hvpr_stream_t stream) {
    if (n_segments < 0 || segments_per_table < 1 || n_max < 0 || box_stride < 7 || max_keep < 0) return HVPR_ERR_INVALID_ARG;
    if (n_segments == 0) return HVPR_OK;
    if (!keep_count) return HVPR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (n_max == 0) {
        if (hipMemsetAsync(keep_count, 0, (size_t)n_segments * sizeof(int), s) != hipSuccess) return HVPR_ERR_LAUNCH;
        return HVPR_OK;
    }
    if (!boxes || !keep || !workspace) return HVPR_ERR_INVALID_ARG;
    if (n_max > 16384 || n_segments > 65535) return HVPR_ERR_UNSUPPORTED;
    if (workspace_bytes < hvpr_nms_bev_batched_workspace_bytes(n_segments, n_max)) return HVPR_ERR_WORKSPACE;
    const int nb = (n_max + 63) / 64, S = n_segments;
    const size_t nbl = nb < 64 ? nb : 64, tiles = nbl * (nbl + 1) / 2;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    NmsCall nc;
    nc.boxes = boxes; nc.box_stride = box_stride; nc.table_stride = table_stride; nc.segs_per_table = segments_per_table;
    nc.order = order; nc.n_device = n_device;
    nc.n_segments = S; nc.n_max = n_max; nc.nb = nb;
    nc.ws = (char *)workspace; nc.seg_bytes = nms_segment_stride(n_max);
    nc.off_prepared = up((size_t)n_max * nb * sizeof(unsigned long long));
    nc.off_plist = nc.off_prepared + up((size_t)n_max * sizeof(Box));
    nc.off_pcount = nc.off_plist + up(tiles * kTileCap * sizeof(unsigned short));
    nc.off_ci = nc.off_pcount + up(tiles * sizeof(int));
    hipLaunchKernelGGL(k_nms_prep, dim3(hvpr_cdiv(n_max, 256), S), dim3(256), 0, s, nc);
    if (nb <= 64) {
        hipLaunchKernelGGL(k_nms_pairs, dim3(nb, nb, S), dim3(64), 0, s, nc);
        hipLaunchKernelGGL(k_nms_scan, dim3(S), dim3(1024), 0, s, nc);
        // one grid for all segments; k_nms_clip needs at least one workgroup per segment beside the ones it deals out by load
        const int clip_blocks = S == 1 || 2 * S <= kClipBlocks ? kClipBlocks : 2 * S;
        hipLaunchKernelGGL(k_nms_clip, dim3(clip_blocks), dim3(kClipThreads), 0, s, nc, thresh);
    } else {
        hipLaunchKernelGGL(k_nms_mask, dim3(nb, nb, S), dim3(64), 0, s, nc, thresh);
    }
    if (nb <= kRingWords) {
        const size_t lds = (size_t)2 * 64 * kRingWords * sizeof(unsigned long long);
        static unsigned long long lds_set = 0ull;   // per device
        if (hvpr_ensure_dyn_lds((const void *)k_nms_sweep_ring, (int)lds, &lds_set) != 0) return HVPR_ERR_LAUNCH;
        hipLaunchKernelGGL(k_nms_sweep_ring, dim3(S), dim3(kRingThreads), lds, s, nc, map_through_order, max_keep, keep, keep_count);
    } else {
        hipLaunchKernelGGL(k_nms_sweep, dim3(S), dim3(64), 0, s, nc, map_through_order, max_keep, keep, keep_count);
    }
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_nms_bev_f32(const float *boxes, int box_stride, const int32_t *order, const int32_t *n_device,
                                int n_max, float thresh, int max_keep, int map_through_order, int32_t *keep,
                                int32_t *keep_count, void *workspace, size_t workspace_bytes, hvpr_stream_t stream) {
    if (!keep_count) return HVPR_ERR_INVALID_ARG;
    return hvpr_nms_bev_batched_f32(boxes, box_stride, 0, 1, order, n_device, 1, n_max, thresh, max_keep, map_through_order, keep,
                                    keep_count, workspace, workspace_bytes, stream);
}
