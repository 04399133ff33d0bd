// The GT-sampling database from raw frames, on the device, for every frame of a chunk at once: the loop of
// KittiDataset.create_groundtruth_database (pcdet/datasets/kitti/kitti_dataset.py:205-238).  Per annotated box the points of
// its frame that lie inside it (points_in_boxes_cpu, :217), moved into the box's own frame (:226), end to end in one arena.
//
// The inside test is box_cut.h's, shared with augment.hip.  The move is numpy's: a float32 column minus a float64 centre is
// computed in double and rounded once (:226 subtracts float64 boxes from a float32 array), so the centres come as doubles.
//
// Three passes, no atomics, stable, bit-reproducible: a count pass (per box and block of kBlk scene points how many points are
// inside, then per box the sum), a scan (obj_off over the boxes, then each box's blocks), a write pass.  The count and write
// passes run one grid over (point blocks x frames) with the frame's boxes staged in LDS, so a frame with one box and one with
// 200 keep the machine equally busy.  Between the two entry points the host reads obj_count and sizes the arena.
//
// Built with -ffp-contract=off: the fp32 operation order below is the CPU native's.
#include "box_cut.h"
#include "common.h"

#include <algorithm>

namespace {

constexpr int kFrameBoxes = 256;     // boxes of one frame
constexpr int kBlk = 256;            // scene points per workgroup of the count and write passes
constexpr int kWaves = kBlk / 64;
constexpr int kMaxFrames = 65535;    // gridDim.y

// The boxes as they are: no extra width.  size + 0.0f is the size for every float except that -0 becomes +0, and a half width
// of either zero rejects every point under `<` and decides `<=` alike, so every inside decision is that of size / 2.0f.
__device__ __forceinline__ void load_cuts(const float *__restrict__ boxes, int b0, int nb, hvpr_cut *cut) {
    for (int k = threadIdx.x; k < nb; k += blockDim.x) cut[k] = hvpr_make_cut(boxes + (size_t)(b0 + k) * 7, 0.0f, 0.0f, 0.0f);
}

// wave_n[w * kFrameBoxes + k] = how many points of wave w of this workgroup lie in box k of the frame
__device__ __forceinline__ void wave_counts(const hvpr_cut *cut, int nb, bool live, float x, float y, float z, int *wave_n) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < nb; ++k) {
        const unsigned long long m = __ballot(live && hvpr_cut_inside(cut[k], x, y, z));
        if (ln == 0) wave_n[wv * kFrameBoxes + k] = __popcll(m);
    }
}

// pass 1: blk_cnt[(b0 + k) * max_blk + block] for every box k of frame f = blockIdx.y and every block of the grid (blocks past
// the frame's last point write zeros: the scan reads every entry)
__global__ void __launch_bounds__(kBlk) k_count(const float *__restrict__ pts, int F, const int32_t *__restrict__ pt_off,
                                                const float *__restrict__ boxes, const int32_t *__restrict__ box_off,
                                                int32_t *__restrict__ blk_cnt) {
    __shared__ hvpr_cut cut[kFrameBoxes];
    __shared__ int wave_n[kWaves * kFrameBoxes];
    const int f = blockIdx.y;
    const int b0 = box_off[f], nb = min(box_off[f + 1] - b0, kFrameBoxes);
    const int p0 = pt_off[f], n = pt_off[f + 1] - p0, j = blockIdx.x * kBlk + threadIdx.x;
    const size_t max_blk = gridDim.x;
    if (blockIdx.x * kBlk >= n) {                                            // the whole workgroup: nothing of the frame here
        for (int k = threadIdx.x; k < nb; k += kBlk) blk_cnt[(size_t)(b0 + k) * max_blk + blockIdx.x] = 0;
        return;
    }
    load_cuts(boxes, b0, nb, cut);
    __syncthreads();
    const bool live = j < n;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) {
        const float *q = pts + (size_t)(p0 + j) * F;
        x = q[0]; y = q[1]; z = q[2];
    }
    wave_counts(cut, nb, live, x, y, z, wave_n);
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += kBlk) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += wave_n[w * kFrameBoxes + k];
        blk_cnt[(size_t)(b0 + k) * max_blk + blockIdx.x] = s;
    }
}

// pass 1b: obj_count[k] = the sum of box k's blocks; a wave per box
__global__ void __launch_bounds__(64) k_obj_count(const int32_t *__restrict__ blk_cnt, int max_blk, int32_t *__restrict__ obj_count) {
    const int32_t *row = blk_cnt + (size_t)blockIdx.x * max_blk;
    int s = 0;
    for (int i = threadIdx.x; i < max_blk; i += 64) s += row[i];
    HVPR_WAVE_SUM_XOR(s);
    if (threadIdx.x == 0) obj_count[blockIdx.x] = s;
}

// pass 2a: obj_off [n_obj + 1]
__global__ void __launch_bounds__(256) k_scan_obj(const int32_t *__restrict__ obj_count, int n_obj, int32_t *__restrict__ obj_off) {
    __shared__ int wave_sum[256 / 64];
    hvpr_block_scan([&](int i) { return obj_count[i]; }, n_obj, 0, obj_off, true, wave_sum);
}

// pass 2b: blk_pre[k * max_blk + b] = the arena row of the first point of block b in box k; a workgroup per box
__global__ void __launch_bounds__(64) k_scan_blk(const int32_t *__restrict__ blk_cnt, int max_blk, const int32_t *__restrict__ obj_off,
                                                 int32_t *__restrict__ blk_pre) {
    __shared__ int wave_sum[1];
    const size_t o = (size_t)blockIdx.x * max_blk;
    hvpr_block_scan([&](int i) { return blk_cnt[o + i]; }, max_blk, obj_off[blockIdx.x], blk_pre + o, false, wave_sum);
}

// pass 3: every (point, box) pair that is inside writes one arena row.  The test is made again, on the same values by the same
// instructions, so it decides as pass 1 did; a row past `capacity` (the counts were not those of this input) is not written.
__global__ void __launch_bounds__(kBlk) k_write(const float *__restrict__ pts, int F, const int32_t *__restrict__ pt_off,
                                                const float *__restrict__ boxes, const int32_t *__restrict__ box_off,
                                                const double *__restrict__ centres, const int32_t *__restrict__ blk_pre,
                                                long long capacity, float *__restrict__ arena) {
    __shared__ hvpr_cut cut[kFrameBoxes];
    __shared__ int wave_n[kWaves * kFrameBoxes];
    const int f = blockIdx.y;
    const int b0 = box_off[f], nb = min(box_off[f + 1] - b0, kFrameBoxes);
    const int p0 = pt_off[f], n = pt_off[f + 1] - p0, j = blockIdx.x * kBlk + threadIdx.x;
    if (blockIdx.x * kBlk >= n) return;                                      // the whole workgroup leaves
    const size_t max_blk = gridDim.x;
    load_cuts(boxes, b0, nb, cut);
    __syncthreads();
    const bool live = j < n;
    const float *q = pts + (size_t)(p0 + (live ? j : 0)) * F;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) { x = q[0]; y = q[1]; z = q[2]; }
    wave_counts(cut, nb, live, x, y, z, wave_n);
    __syncthreads();
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < nb; ++k) {
        const bool in = live && hvpr_cut_inside(cut[k], x, y, z);
        const unsigned long long m = __ballot(in);
        if (!in) continue;
        int before = 0;
        for (int w = 0; w < wv; ++w) before += wave_n[w * kFrameBoxes + k];
        const long long row = (long long)blk_pre[(size_t)(b0 + k) * max_blk + blockIdx.x] + before + __popcll(m & ((1ull << ln) - 1ull));
        if (row < 0 || row >= capacity) continue;
        const double *c = centres + (size_t)(b0 + k) * 3;
        float *r = arena + (size_t)row * F;
        r[0] = (float)((double)x - c[0]);
        r[1] = (float)((double)y - c[1]);
        r[2] = (float)((double)z - c[2]);
        for (int i = 3; i < F; ++i) r[i] = q[i];
    }
}

struct Ws { int32_t *blk_cnt, *blk_pre; size_t bytes; };

Ws carve(void *base, int max_blk, int n_obj) {
    hvpr_carver cv(base);
    Ws w;
    w.blk_cnt = cv.take<int32_t>((size_t)n_obj * max_blk);
    w.blk_pre = cv.take<int32_t>((size_t)n_obj * max_blk);
    w.bytes = cv.off;
    return w;
}

bool rising(const int32_t *off, int n, long long last) {     // off[0] = 0 <= off[1] <= ... <= off[n] = last
    if (off[0] != 0 || off[n] != last) return false;
    for (int i = 0; i < n; ++i)
        if (off[i] > off[i + 1]) return false;
    return true;
}

// Everything both entry points check about the chunk.  0, or the status to return; max_blk = blocks of the longest frame.
int open_chunk(const float *points, long long n_points, int F, const int32_t *pt_off_host, const int32_t *pt_off, int B,
               const float *boxes, const int32_t *box_off_host, const int32_t *box_off, int n_obj, int &max_blk) {
    if (B < 1 || n_obj < 0 || n_points < 0 || F < 3 || F > 8 || !pt_off_host || !pt_off || !box_off_host || !box_off ||
        (n_points > 0 && !points) || (n_obj > 0 && !boxes))
        return HVPR_ERR_INVALID_ARG;
    if (n_points > 0x7fffffffLL || B > kMaxFrames) return HVPR_ERR_UNSUPPORTED;       // 32-bit offsets; one grid row per frame
    if (!rising(pt_off_host, B, n_points) || !rising(box_off_host, B, n_obj)) return HVPR_ERR_INVALID_ARG;
    max_blk = 1;
    for (int f = 0; f < B; ++f) {
        if (box_off_host[f + 1] - box_off_host[f] > kFrameBoxes) return HVPR_ERR_UNSUPPORTED;
        max_blk = std::max(max_blk, hvpr_cdiv(pt_off_host[f + 1] - pt_off_host[f], kBlk));
    }
    return 0;
}

}  // namespace

extern "C" int hvpr_gt_database_block_points(void) { return kBlk; }

extern "C" size_t hvpr_gt_database_workspace_bytes(int n_frames, int max_frame_points, int n_obj) {
    if (n_frames < 1 || max_frame_points < 0 || n_obj < 1) return 0;
    return carve(nullptr, std::max(1, hvpr_cdiv(max_frame_points, kBlk)), n_obj).bytes;
}

extern "C" int hvpr_gt_database_count_f32(const float *points, long long n_points, int point_floats, const int32_t *pt_off_host,
                                          const int32_t *pt_off, int n_frames, const float *boxes, const int32_t *box_off_host,
                                          const int32_t *box_off, int n_obj, int32_t *obj_count, void *workspace,
                                          size_t workspace_bytes, hvpr_stream_t stream) {
    int max_blk = 1;
    if (const int st = open_chunk(points, n_points, point_floats, pt_off_host, pt_off, n_frames, boxes, box_off_host, box_off, n_obj,
                                  max_blk))
        return st;
    if (n_obj == 0) return HVPR_OK;
    if (!obj_count || !workspace) return HVPR_ERR_INVALID_ARG;
    const Ws w = carve(workspace, max_blk, n_obj);
    if (workspace_bytes < w.bytes) return HVPR_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_count, dim3(max_blk, n_frames), dim3(kBlk), 0, s, points, point_floats, pt_off, boxes, box_off, w.blk_cnt);
    HVPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_obj_count, dim3(n_obj), dim3(64), 0, s, w.blk_cnt, max_blk, obj_count);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}

extern "C" int hvpr_gt_database_extract_f32(const float *points, long long n_points, int point_floats, const int32_t *pt_off_host,
                                            const int32_t *pt_off, int n_frames, const float *boxes, const int32_t *box_off_host,
                                            const int32_t *box_off, const double *centres, int n_obj,
                                            const int32_t *obj_count_host, const int32_t *obj_count, int32_t *obj_off, float *arena,
                                            long long arena_capacity, void *workspace, size_t workspace_bytes,
                                            hvpr_stream_t stream) {
    int max_blk = 1;
    if (const int st = open_chunk(points, n_points, point_floats, pt_off_host, pt_off, n_frames, boxes, box_off_host, box_off, n_obj,
                                  max_blk))
        return st;
    if (!obj_off || arena_capacity < 0 || (n_obj > 0 && (!centres || !obj_count_host || !obj_count || !workspace)))
        return HVPR_ERR_INVALID_ARG;
    long long rows = 0;
    for (int f = 0; f < n_frames; ++f)                                       // a box holds no more points than its frame has
        for (int k = box_off_host[f]; k < box_off_host[f + 1]; ++k) {
            if (obj_count_host[k] < 0 || obj_count_host[k] > pt_off_host[f + 1] - pt_off_host[f]) return HVPR_ERR_INVALID_ARG;
            rows += obj_count_host[k];
        }
    if (rows > 0x7fffffffLL) return HVPR_ERR_UNSUPPORTED;                    // 32-bit row offsets
    if (arena_capacity < rows || (rows > 0 && !arena)) return HVPR_ERR_INVALID_ARG;
    const Ws w = carve(workspace, max_blk, n_obj);
    if (n_obj > 0 && workspace_bytes < w.bytes) return HVPR_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_scan_obj, dim3(1), dim3(256), 0, s, obj_count, n_obj, obj_off);
    HVPR_CHECK_LAUNCH();
    if (n_obj == 0) return HVPR_OK;
    hipLaunchKernelGGL(k_scan_blk, dim3(n_obj), dim3(64), 0, s, w.blk_cnt, max_blk, obj_off, w.blk_pre);
    HVPR_CHECK_LAUNCH();
    if (rows == 0) return HVPR_OK;
    hipLaunchKernelGGL(k_write, dim3(max_blk, n_frames), dim3(kBlk), 0, s, points, point_floats, pt_off, boxes, box_off, centres, w.blk_pre,
                       arena_capacity, arena);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
