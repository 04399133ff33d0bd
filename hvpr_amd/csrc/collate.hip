// f7 — training batches on the device: ragged select / shuffle / collate, a whole batch per launch.  The frames of a batch lie
// end to end in one (rows, F) float32 array with DEVICE-resident offsets (B + 1,) int32 (after hvpr_augment_points_f32 the host
// does not know them yet); rows at or past off[B] are capacity and are ignored.  Covers, for all frames at once,
//   KittiDataset.get_fov_flag + points[fov_flag]                  pcdet/datasets/kitti/kitti_dataset.py:100-116, 379-383
//   mask_points_by_range + points[mask]                           pcdet/datasets/processor/data_processor.py:20-23
//   shuffle_points (points[permutation], drawn on the host)       data_processor.py:32-39
//   collate_batch's `points` branch (batch index in column 0)     pcdet/datasets/dataset.py:161-166
// The keep decisions are the expressions of point_pred.h, shared with hvpr_point_flags_f32.
//
// A flat stable compaction over tiles of kTile rows.  Lane l of wave w looks at rows tile + (4 w + k) 64 + l, k = 0..3, so one
// ballot per k gives a group of 64 consecutive rows and the popcount of the lanes below gives a row's rank in it: loads and
// (unpermuted) stores stay coalesced.  A row's frame is the binary search over the offsets staged in LDS.
//   count pass   per-tile counts, and for every offset the count of kept rows in front of it inside the tile that contains it
//                (lane-masked ballot)
//   scan         one workgroup: exclusive prefix of the tile counts; new_off[b] = prefix of off[b]'s tile + that partial count
//   write pass   recomputes the decisions, places each kept row by its flat rank
// No atomics, no flag array, no spin-waits: bit-reproducible.
// hvpr_ragged_sample_*: the same three passes, the same code with NEAR on, with DataProcessor.sample_points
// (data_processor.py:77-108) between the mask and the shuffle.  Its draws depend on a frame only through the count n of kept
// rows and the count c of kept rows that are near (||xyz|| < 40, hvpr_pred_near): the host draws over ordinals from those two
// counts and hands back, for every kept row, the output rows it goes to.  So the count pass takes a second ballot (kept AND
// near) next to the first and the scan yields near_off next to new_off; the write pass recomputes both decisions, derives the
// row's ordinal from the two ranks and scatters it through the destination table.
#include "common.h"
#include "point_pred.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 4;
constexpr int kGroups = kWaves * kItems;       // ballots of 64 rows per tile
constexpr int kTile = kThreads * kItems;
constexpr int kMaxFrames = 1024;
constexpr int kCalib = 26;                     // eval_loop.pack_calib: a (4x3), P2 (3x4), image height, image width

struct SelArgs {
    const float *pts;
    int rows, F;
    const int *off;
    int B, mask, tiles;
    const float *calib;
    float x0, y0, x1, y1;
    float near;              // the sample calls' radius; 0 in the select calls, which never read it
};

struct Staged {
    int off[kMaxFrames + 1];
    float cal[kCalib];       // the tile's first frame, p transposed to the 4 x 3 layout point_pred.h reads
    int b0;
};

__device__ __forceinline__ void load_calib(const float *row, float *dst, int i) {
    // words 12..23 hold P2 (3 x 4, row-major); dst[12 + r*3 + c] = P2^T[r][c] = P2[c][r]
    if (i < 12 || i >= 24) dst[i] = row[i];
    else { const int r = (i - 12) / 3, c = (i - 12) % 3; dst[i] = row[12 + c * 4 + r]; }
}

// offsets clamped into [0, rows]: whatever the device words hold, no row outside the array is read
__device__ __forceinline__ void stage(const SelArgs &a, Staged &s, int tile_base) {
    for (int i = threadIdx.x; i <= a.B; i += kThreads) s.off[i] = min(max(a.off[i], 0), a.rows);
    __syncthreads();
    if (threadIdx.x == 0) s.b0 = (tile_base >= s.off[0] && tile_base < s.off[a.B]) ? hvpr_frame_of(s.off, a.B, tile_base) : 0;
    __syncthreads();
    if ((a.mask & 1) && threadIdx.x < kCalib) load_calib(a.calib + (size_t)s.b0 * kCalib, s.cal, threadIdx.x);
    __syncthreads();
}

__device__ __forceinline__ bool decide(const SelArgs &a, const Staged &s, int b, float x, float y, float z) {
    bool f = true;
    if (a.mask & 2) f = hvpr_pred_range_xy(x, y, a.x0, a.y0, a.x1, a.y1);
    if (f && (a.mask & 1)) {
        if (b == s.b0) {
            f = hvpr_pred_fov(x, y, z, s.cal, s.cal + 12, s.cal[24], s.cal[25]);
        } else {                                                     // a tile that spans frames: the later frames' rows
            float c[kCalib];
            const float *row = a.calib + (size_t)b * kCalib;
#pragma unroll
            for (int i = 0; i < kCalib; ++i) load_calib(row, c, i);
            f = hvpr_pred_fov(x, y, z, c, c + 12, c[24], c[25]);
        }
    }
    return f;
}

// The workspace: per count set (0: kept rows, 1: kept and near rows) the tile counts, their prefix, and per offset the count in
// front of it inside its tile.  Set 0 of the two-set layout lies where the one-set layout lies, because it is this code: the
// select write pass can read the workspace of a sample count pass (batch_loader.py, debug_choices, does).
struct Carved {
    int *count[2], *first[2], *partial[2];
    size_t bytes;
};

Carved carve(void *ws, int tiles, int B, int sets) {
    hvpr_carver c(ws);
    Carved r = {};
    for (int j = 0; j < sets; ++j) {
        r.count[j] = c.take<int>((size_t)tiles + 1);
        r.first[j] = c.take<int>((size_t)tiles + 1);
        r.partial[j] = c.take<int>((size_t)B + 1);
    }
    r.bytes = c.off;
    return r;
}

// set bits of the tile's ballots in front of its row `local`, 0 .. kTile
__device__ __forceinline__ int count_before(const unsigned long long *bal, int local) {
    const int g_end = local >> 6;
    int c = 0;
    for (int g = 0; g < g_end; ++g) c += __popcll(bal[g]);
    if (g_end < kGroups) c += __popcll(bal[g_end] & ((1ull << (local & 63)) - 1ull));
    return c;
}

template <bool NEAR>
__global__ void __launch_bounds__(kThreads) k_count(SelArgs a, Carved w) {
    constexpr int kSets = NEAR ? 2 : 1;
    __shared__ Staged s;
    __shared__ unsigned long long s_bal[kSets][kGroups];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int tile_base = blockIdx.x * kTile;
    stage(a, s, tile_base);
    const int lo = s.off[0], hi = s.off[a.B];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int row = tile_base + (wid * kItems + k) * 64 + lane;
        bool f = false, g = false;
        if (row >= lo && row < hi) {
            const float *p = a.pts + (size_t)row * a.F;
            const float x = p[0], y = p[1], z = p[2];
            f = decide(a, s, hvpr_frame_of(s.off, a.B, row), x, y, z);
            if constexpr (NEAR) g = f && hvpr_pred_near(x, y, z, a.near);
        }
        const unsigned long long bal = __ballot(f);
        if (lane == 0) s_bal[0][wid * kItems + k] = bal;
        if constexpr (NEAR) {
            const unsigned long long nbal = __ballot(g);
            if (lane == 0) s_bal[1][wid * kItems + k] = nbal;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSets; ++j) {
        if (threadIdx.x == 0) w.count[j][blockIdx.x] = count_before(s_bal[j], kTile);
        // the offsets that fall into this tile (the array's end belongs to the last tile)
        for (int b = threadIdx.x; b <= a.B; b += kThreads) {
            const int o = s.off[b];
            if (min(o / kTile, a.tiles - 1) == (int)blockIdx.x) w.partial[j][b] = count_before(s_bal[j], o - tile_base);
        }
    }
}

// one workgroup: first[t] = counted rows in front of tile t, first[tiles] = all; then the new offsets.  Per count set.
__global__ void __launch_bounds__(kThreads) k_scan(const int *__restrict__ off, int B, int rows, int tiles, Carved w, int sets,
                                                   int *__restrict__ new_off, int *__restrict__ near_off) {
    __shared__ int wave_sum[kWaves];
    const auto scan_set = [&](const int *count, int *first, const int *partial, int *out) {
        hvpr_block_scan([&](int t) { return count[t]; }, tiles, 0, first, true, wave_sum);
        for (int b = threadIdx.x; b <= B; b += kThreads) {
            if (tiles == 0) { out[b] = 0; continue; }
            const int o = min(max(off[b], 0), rows);
            out[b] = first[min(o / kTile, tiles - 1)] + partial[b];
        }
    };
    scan_set(w.count[0], w.first[0], w.partial[0], new_off);
    if (sets == 2) scan_set(w.count[1], w.first[1], w.partial[1], near_off);
}

// a kept row to its place in the output: (float)b in front when the batch column is on, one 16-byte store where it can be
template <bool VEC4>
__device__ __forceinline__ void store_row(float *o, int batch_column, int b, const float4 &v, const float *src, int F) {
    if (batch_column) *o++ = (float)b;
    if (VEC4) {
        if (!batch_column) {
            *reinterpret_cast<float4 *>(o) = v;
        } else {
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    } else {
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
        for (int j = 3; j < F; ++j) o[j] = src[j];
    }
}

// The write pass over one tile, up to where a kept row goes: recomputes the decisions and calls
//   place(b, src, v, isnear, rank, nrank)
// for every kept row, with its frame, its row in a.pts, its first four floats (three without VEC4), its flat rank among the
// kept rows and, under NEAR, whether it is near and its flat rank among the kept near rows.
template <bool NEAR, bool VEC4, typename Place>
__device__ __forceinline__ void walk_tile(const SelArgs &a, const Carved &w, Place place) {
    __shared__ Staged s;
    __shared__ int s_w[NEAR ? 2 : 1][kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int tile_base = blockIdx.x * kTile;
    stage(a, s, tile_base);
    const int lo = s.off[0], hi = s.off[a.B];
    unsigned long long bal[kItems], nbal[kItems];
    int frame[kItems];
    bool keep[kItems], isnear[kItems];
    float4 v[kItems];
    int total = 0, ntotal = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int row = tile_base + (wid * kItems + k) * 64 + lane;
        keep[k] = isnear[k] = false;
        frame[k] = 0;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row >= lo && row < hi) {
            if (VEC4) {
                v[k] = *reinterpret_cast<const float4 *>(a.pts + (size_t)row * 4);       // one 16-byte access per lane
            } else {
                const float *p = a.pts + (size_t)row * a.F;
                v[k].x = p[0]; v[k].y = p[1]; v[k].z = p[2];
            }
            frame[k] = hvpr_frame_of(s.off, a.B, row);
            keep[k] = decide(a, s, frame[k], v[k].x, v[k].y, v[k].z);
            if constexpr (NEAR) isnear[k] = keep[k] && hvpr_pred_near(v[k].x, v[k].y, v[k].z, a.near);
        }
        bal[k] = __ballot(keep[k]);
        total += __popcll(bal[k]);
        if constexpr (NEAR) {
            nbal[k] = __ballot(isnear[k]);
            ntotal += __popcll(nbal[k]);
        }
    }
    if (lane == 0) {
        s_w[0][wid] = total;
        if constexpr (NEAR) s_w[1][wid] = ntotal;
    }
    __syncthreads();
    long long pos = w.first[0][blockIdx.x], npos = 0;
    if constexpr (NEAR) npos = w.first[1][blockIdx.x];
    for (int i = 0; i < wid; ++i) {
        pos += s_w[0][i];
        if constexpr (NEAR) npos += s_w[1][i];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const long long rank = pos + __popcll(bal[k] & below);
        pos += __popcll(bal[k]);
        long long nrank = 0;
        if constexpr (NEAR) {
            nrank = npos + __popcll(nbal[k] & below);
            npos += __popcll(nbal[k]);
        }
        if (keep[k]) place(frame[k], a.pts + (size_t)(tile_base + (wid * kItems + k) * 64 + lane) * a.F, v[k], isnear[k], rank, nrank);
    }
}

template <bool VEC4>
__global__ void __launch_bounds__(kThreads) k_select_write(SelArgs a, Carved w, const int *__restrict__ new_off,
                                                           const int *__restrict__ inv_perm, long long n_perm, int batch_column,
                                                           float *__restrict__ out, long long out_capacity, int *__restrict__ flag) {
    __shared__ int s_noff[kMaxFrames + 1];
    for (int i = threadIdx.x; i <= a.B; i += kThreads) s_noff[i] = new_off[i];                // walk_tile's barriers follow
    const int W = a.F + (batch_column ? 1 : 0);
    walk_tile<false, VEC4>(a, w, [&](int b, const float *src, const float4 &v, bool, long long rank, long long) {
        long long d = rank;
        if (inv_perm) {
            const int first = s_noff[b], m = s_noff[b + 1] - first;
            if (rank >= n_perm) { *flag = 1; return; }
            const int q = inv_perm[rank];
            if (q < 0 || q >= m) { *flag = 1; return; }                 // never a row of another frame, never out of bounds
            d = (long long)first + q;
        }
        if (d < 0 || d >= out_capacity) { *flag = 1; return; }
        store_row<VEC4>(out + (size_t)d * W, batch_column, b, v, src, a.F);
    });
}

struct SampleArgs {
    const int *new_off, *near_off, *mode, *dest;
    long long n_dest, out_capacity;
    int P, batch_column;
};

template <bool VEC4>
__global__ void __launch_bounds__(kThreads) k_sample_write(SelArgs a, Carved w, SampleArgs q, float *__restrict__ out,
                                                           int *__restrict__ flag) {
    __shared__ int s_noff[kMaxFrames + 1], s_near[kMaxFrames + 1];
    for (int i = threadIdx.x; i <= a.B; i += kThreads) { s_noff[i] = q.new_off[i]; s_near[i] = q.near_off[i]; }
    const int W = a.F + (q.batch_column ? 1 : 0);
    walk_tile<true, VEC4>(a, w, [&](int b, const float *src, const float4 &v, bool isnear, long long rank, long long nrank) {
        const long long first = s_noff[b], n_b = s_noff[b + 1] - first;
        const long long r = rank - first, an = nrank - s_near[b], c_b = s_near[b + 1] - s_near[b];
        const int mode = q.mode[b];
        long long ord = r;                                               // mode 0: the in-frame rank
        if (mode == 1) ord = isnear ? an : c_b + (r - an);              // mode 1: near ordinals first, then the far ones
        const long long t = first + ord;
        if ((mode != 0 && mode != 1) || ord < 0 || ord >= n_b || t < 0 || t >= q.n_dest) { *flag = 1; return; }
        const int2 d2 = *reinterpret_cast<const int2 *>(q.dest + 2 * t);
        const int dd[2] = {d2.x, d2.y};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int d = dd[e];
            if (d == -1) continue;
            if (d < -1 || d >= q.P) { *flag = 1; continue; }
            const long long at = (long long)b * q.P + d;
            if (at >= q.out_capacity) { *flag = 1; continue; }           // never outside `out`
            store_row<VEC4>(out + (size_t)at * W, q.batch_column, b, v, src, a.F);
        }
    });
}

// what all four entry points check; `need` is the workspace size of the caller's layout, `near` 0 where there is none
int check_args(const float *points, long long rows, int F, const int32_t *off, int B, int mask, const float *calib,
               const float *range_xy, float near, void *workspace, size_t workspace_bytes, size_t need, SelArgs *a) {
    if (rows < 0 || F < 3 || B < 1 || mask < 0 || mask > 3 || !off || !workspace) return HVPR_ERR_INVALID_ARG;
    if ((rows > 0 && !points) || ((mask & 1) && !calib) || ((mask & 2) && !range_xy)) return HVPR_ERR_INVALID_ARG;
    if (B > kMaxFrames || F > 64 || rows > 0x7fffffffLL - kTile) return HVPR_ERR_UNSUPPORTED;
    if (!(near >= 0.f)) return HVPR_ERR_INVALID_ARG;
    if (workspace_bytes < need) return HVPR_ERR_WORKSPACE;
    a->pts = points; a->rows = (int)rows; a->F = F; a->off = off; a->B = B; a->mask = mask;
    a->tiles = hvpr_cdiv(rows, kTile);
    a->calib = calib;
    a->x0 = (mask & 2) ? range_xy[0] : 0.f; a->y0 = (mask & 2) ? range_xy[1] : 0.f;
    a->x1 = (mask & 2) ? range_xy[2] : 0.f; a->y1 = (mask & 2) ? range_xy[3] : 0.f;
    a->near = near;
    return HVPR_OK;
}

size_t workspace_bytes_of(long long rows, int B, int sets) {
    if (rows < 0 || B < 1) return 0;
    return carve(nullptr, hvpr_cdiv(rows, kTile), B, sets).bytes;
}

void launch_count(const SelArgs &a, const Carved &w, int sets, int32_t *new_off, int32_t *near_off, hipStream_t s) {
    if (a.tiles > 0) {
        if (sets == 2) hipLaunchKernelGGL(k_count<true>, dim3(a.tiles), dim3(kThreads), 0, s, a, w);
        else hipLaunchKernelGGL(k_count<false>, dim3(a.tiles), dim3(kThreads), 0, s, a, w);
    }
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kThreads), 0, s, a.off, a.B, a.rows, a.tiles, w, sets, new_off, near_off);
}

// one 16-byte access per row, where the rows allow it
bool rows_vec4(const float *points, int F, int batch_column, const float *out) {
    return F == 4 && ((uintptr_t)points & 15) == 0 && (batch_column || ((uintptr_t)out & 15) == 0);
}

}  // namespace

extern "C" int hvpr_ragged_select_tile_rows(void) { return kTile; }

extern "C" size_t hvpr_ragged_select_workspace_bytes(long long rows, int n_frames) { return workspace_bytes_of(rows, n_frames, 1); }

extern "C" size_t hvpr_ragged_sample_workspace_bytes(long long rows, int n_frames) { return workspace_bytes_of(rows, n_frames, 2); }

extern "C" int hvpr_ragged_select_count_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                            int mask, const float *calib, const float *range_xy, int32_t *new_off, void *workspace,
                                            size_t workspace_bytes, hvpr_stream_t stream) {
    SelArgs a;
    const int st = check_args(points, rows, point_floats, off, n_frames, mask, calib, range_xy, 0.f, workspace, workspace_bytes,
                              workspace_bytes_of(rows, n_frames, 1), &a);
    if (st != HVPR_OK) return st;
    if (!new_off) return HVPR_ERR_INVALID_ARG;
    launch_count(a, carve(workspace, a.tiles, n_frames, 1), 1, new_off, nullptr, (hipStream_t)stream);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_ragged_sample_count_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                            int mask, const float *calib, const float *range_xy, float near, int32_t *new_off,
                                            int32_t *near_off, void *workspace, size_t workspace_bytes, hvpr_stream_t stream) {
    SelArgs a;
    const int st = check_args(points, rows, point_floats, off, n_frames, mask, calib, range_xy, near, workspace, workspace_bytes,
                              workspace_bytes_of(rows, n_frames, 2), &a);
    if (st != HVPR_OK) return st;
    if (!new_off || !near_off) return HVPR_ERR_INVALID_ARG;
    launch_count(a, carve(workspace, a.tiles, n_frames, 2), 2, new_off, near_off, (hipStream_t)stream);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_ragged_select_write_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                            int mask, const float *calib, const float *range_xy, const int32_t *new_off,
                                            const int32_t *inv_perm, long long n_perm, int batch_column, float *out,
                                            long long out_capacity, int32_t *flag, void *workspace, size_t workspace_bytes,
                                            hvpr_stream_t stream) {
    SelArgs a;
    const int st = check_args(points, rows, point_floats, off, n_frames, mask, calib, range_xy, 0.f, workspace, workspace_bytes,
                              workspace_bytes_of(rows, n_frames, 1), &a);
    if (st != HVPR_OK) return st;
    if (!new_off || !flag || out_capacity < 0 || n_perm < 0 || (out_capacity > 0 && !out)) return HVPR_ERR_INVALID_ARG;
    if (out_capacity > 0x7fffffffLL) return HVPR_ERR_UNSUPPORTED;
    if (a.tiles == 0) return HVPR_OK;
    const Carved w = carve(workspace, a.tiles, n_frames, 1);
    hipStream_t s = (hipStream_t)stream;
    if (rows_vec4(points, point_floats, batch_column, out))
        hipLaunchKernelGGL(k_select_write<true>, dim3(a.tiles), dim3(kThreads), 0, s, a, w, new_off, inv_perm, n_perm,
                           batch_column ? 1 : 0, out, out_capacity, flag);
    else
        hipLaunchKernelGGL(k_select_write<false>, dim3(a.tiles), dim3(kThreads), 0, s, a, w, new_off, inv_perm, n_perm,
                           batch_column ? 1 : 0, out, out_capacity, flag);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_ragged_sample_write_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                            int mask, const float *calib, const float *range_xy, float near,
                                            const int32_t *new_off, const int32_t *near_off, const int32_t *mode,
                                            const int32_t *dest, long long n_dest, int num_points, int batch_column, float *out,
                                            long long out_capacity, int32_t *flag, void *workspace, size_t workspace_bytes,
                                            hvpr_stream_t stream) {
    SelArgs a;
    const int st = check_args(points, rows, point_floats, off, n_frames, mask, calib, range_xy, near, workspace, workspace_bytes,
                              workspace_bytes_of(rows, n_frames, 2), &a);
    if (st != HVPR_OK) return st;
    if (!new_off || !near_off || !mode || !flag || out_capacity < 0 || n_dest < 0 || num_points < 0) return HVPR_ERR_INVALID_ARG;
    if ((out_capacity > 0 && !out) || (n_dest > 0 && !dest) || ((uintptr_t)dest & 7) != 0) return HVPR_ERR_INVALID_ARG;
    if (out_capacity > 0x7fffffffLL || n_dest > 0x3fffffffLL) return HVPR_ERR_UNSUPPORTED;
    if (a.tiles == 0) return HVPR_OK;
    const Carved w = carve(workspace, a.tiles, n_frames, 2);
    SampleArgs q;
    q.new_off = new_off; q.near_off = near_off; q.mode = mode; q.dest = dest;
    q.n_dest = n_dest; q.out_capacity = out_capacity; q.P = num_points; q.batch_column = batch_column ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    if (rows_vec4(points, point_floats, batch_column, out))
        hipLaunchKernelGGL(k_sample_write<true>, dim3(a.tiles), dim3(kThreads), 0, s, a, w, q, out, flag);
    else
        hipLaunchKernelGGL(k_sample_write<false>, dim3(a.tiles), dim3(kThreads), 0, s, a, w, q, out, flag);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
