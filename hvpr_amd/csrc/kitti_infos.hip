// get_infos' num_points_in_gt on the device, for every frame of a chunk at once: the loop of KittiDataset.get_infos
// (pcdet/datasets/kitti/kitti_dataset.py:171-184).  Per annotated box the number of points of its frame that are in the camera's
// view (lidar_to_rect, get_fov_flag, :174-177) AND inside the hull of the box's corners (in_hull, :181-183).
//
// Both decisions are shared expressions, included and not restated: the view test is point_pred.h's hvpr_pred_fov, so this count
// and the batch loader (collate.hip) decide bit-equally on every point; the hull of a cuboid's corners is the cuboid, so the hull
// test is box_cut.h's hvpr_cut_inside on the box as it is (no extra width), as in gt_database.hip.  On a face Qhull's tolerance
// decides in the reference and box_cut.h's `<=` / `<` decide here: unpinned.  A box with a zero size counts 0.
//
// The shape is gt_database.hip's count pass: one grid over (point blocks x frames), the frame's calibration row and the cuts of
// its boxes staged in LDS, the view test once per point, a wave with no point in view skips the box loop, per box a wave ballot
// and popcount, per (box, block) a partial count in the caller's workspace, then one sum per box (and, when asked for, per
// frame: the points in view).  No atomics, deterministic, bit-reproducible.  Memory-bound: a point's 16 bytes are read once.
//
// Built with -ffp-contract=off: both included headers require it.
#include "box_cut.h"
#include "common.h"
#include "point_pred.h"

#include <algorithm>

namespace {

constexpr int kFrameBoxes = 256;     // boxes of one frame (gt_database.hip's limit)
constexpr int kBlk = 256;            // scene points per workgroup: the database's block
constexpr int kWaves = kBlk / 64;
constexpr int kMaxFrames = 65535;    // gridDim.y
constexpr int kCalib = 26;           // eval_loop.pack_calib: a (4x3), P2 (3x4), image height, image width

// blk_cnt[(b0 + k) * max_blk + block] for every box k of frame f = blockIdx.y, fov_blk[f * max_blk + block] = points in view
// (blocks past the frame's last point write zeros: the sums read every entry)
template <bool VEC4>
__global__ void __launch_bounds__(kBlk) k_count(const float *__restrict__ pts, int F, const int32_t *__restrict__ pt_off,
                                                const float *__restrict__ boxes, const int32_t *__restrict__ box_off,
                                                const float *__restrict__ calib, int32_t *__restrict__ blk_cnt,
                                                int32_t *__restrict__ fov_blk) {
    __shared__ hvpr_cut cut[kFrameBoxes];
    __shared__ int wave_n[kWaves * kFrameBoxes];
    __shared__ int wave_fov[kWaves];
    __shared__ float cal[kCalib];    // P2 transposed to the 4 x 3 layout point_pred.h reads
    const int f = blockIdx.y;
    const int b0 = box_off[f], nb = min(box_off[f + 1] - b0, kFrameBoxes);
    const int p0 = pt_off[f], n = pt_off[f + 1] - p0, j = blockIdx.x * kBlk + threadIdx.x;
    const size_t max_blk = gridDim.x;
    if (blockIdx.x * kBlk >= n) {                                            // the whole workgroup: nothing of the frame here
        for (int k = threadIdx.x; k < nb; k += kBlk) blk_cnt[(size_t)(b0 + k) * max_blk + blockIdx.x] = 0;
        if (fov_blk && threadIdx.x == 0) fov_blk[(size_t)f * max_blk + blockIdx.x] = 0;
        return;
    }
    for (int k = threadIdx.x; k < nb; k += kBlk) cut[k] = hvpr_make_cut(boxes + (size_t)(b0 + k) * 7, 0.0f, 0.0f, 0.0f);
    if (threadIdx.x < kCalib) {
        const int i = threadIdx.x;
        const float *row = calib + (size_t)f * kCalib;
        // words 12..23 hold P2 (3 x 4, row-major); cal[12 + r*3 + c] = P2^T[r][c] = P2[c][r]
        cal[i] = (i < 12 || i >= 24) ? row[i] : row[12 + ((i - 12) % 3) * 4 + (i - 12) / 3];
    }
    __syncthreads();
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (j < n) {
        if (VEC4) {
            const float4 v = *reinterpret_cast<const float4 *>(pts + (size_t)(p0 + j) * 4);     // one 16-byte access per lane
            x = v.x; y = v.y; z = v.z;
        } else {
            const float *q = pts + (size_t)(p0 + j) * F;
            x = q[0]; y = q[1]; z = q[2];
        }
    }
    const bool vis = j < n && hvpr_pred_fov(x, y, z, cal, cal + 12, cal[24], cal[25]);
    const unsigned long long seen = __ballot(vis);
    if (ln == 0) wave_fov[wv] = __popcll(seen);
    if (seen == 0ull) {                                                      // wave-uniform: no point in view, no box loop
        for (int k = ln; k < nb; k += 64) wave_n[wv * kFrameBoxes + k] = 0;
    } else {
        for (int k = 0; k < nb; ++k) {
            const unsigned long long m = __ballot(vis && hvpr_cut_inside(cut[k], x, y, z));
            if (ln == 0) wave_n[wv * kFrameBoxes + k] = __popcll(m);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += kBlk) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += wave_n[w * kFrameBoxes + k];
        blk_cnt[(size_t)(b0 + k) * max_blk + blockIdx.x] = s;
    }
    if (fov_blk && threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += wave_fov[w];
        fov_blk[(size_t)f * max_blk + blockIdx.x] = s;
    }
}

// a wave per row of `max_blk` partial counts: rows 0 .. n_obj - 1 are the boxes', the rows behind them the frames'
__global__ void __launch_bounds__(64) k_sum(const int32_t *__restrict__ blk_cnt, const int32_t *__restrict__ fov_blk, int n_obj,
                                            int max_blk, int32_t *__restrict__ obj_count, int32_t *__restrict__ fov_count) {
    const int r = blockIdx.x;
    const bool box = r < n_obj;
    const int32_t *row = box ? blk_cnt + (size_t)r * max_blk : fov_blk + (size_t)(r - n_obj) * max_blk;
    int s = 0;
    for (int i = threadIdx.x; i < max_blk; i += 64) s += row[i];
    HVPR_WAVE_SUM_XOR(s);
    if (threadIdx.x == 0) {
        if (box) obj_count[r] = s; else fov_count[r - n_obj] = s;
    }
}

struct Ws { int32_t *blk_cnt, *fov_blk; size_t bytes; };

Ws carve(void *base, int n_frames, int max_blk, int n_obj) {
    hvpr_carver cv(base);
    Ws w;
    w.blk_cnt = cv.take<int32_t>((size_t)n_obj * max_blk);
    w.fov_blk = cv.take<int32_t>((size_t)n_frames * max_blk);
    w.bytes = cv.off;
    return w;
}

bool rising(const int32_t *off, int n, long long last) {     // off[0] = 0 <= off[1] <= ... <= off[n] = last
    if (off[0] != 0 || off[n] != last) return false;
    for (int i = 0; i < n; ++i)
        if (off[i] > off[i + 1]) return false;
    return true;
}

}  // namespace

extern "C" int hvpr_kitti_infos_block_points(void) { return kBlk; }

extern "C" size_t hvpr_kitti_infos_workspace_bytes(int n_frames, int max_frame_points, int n_obj) {
    if (n_frames < 1 || max_frame_points < 0 || n_obj < 0) return 0;
    return carve(nullptr, n_frames, std::max(1, hvpr_cdiv(max_frame_points, kBlk)), n_obj).bytes;
}

extern "C" int hvpr_kitti_infos_count_f32(const float *points, long long n_points, int point_floats, const int32_t *pt_off_host,
                                          const int32_t *pt_off, int n_frames, const float *boxes, const int32_t *box_off_host,
                                          const int32_t *box_off, int n_obj, const float *calib_host, const float *calib,
                                          int32_t *obj_count, int32_t *fov_count, void *workspace, size_t workspace_bytes,
                                          hvpr_stream_t stream) {
    const int B = n_frames, F = point_floats;
    if (B < 1 || n_obj < 0 || n_points < 0 || F < 3 || F > 8 || !pt_off_host || !pt_off || !box_off_host || !box_off || !calib_host ||
        !calib || (n_points > 0 && !points) || (n_obj > 0 && (!boxes || !obj_count)))
        return HVPR_ERR_INVALID_ARG;
    if (n_points > 0x7fffffffLL || B > kMaxFrames) return HVPR_ERR_UNSUPPORTED;       // 32-bit offsets; one grid row per frame
    if (!rising(pt_off_host, B, n_points) || !rising(box_off_host, B, n_obj)) return HVPR_ERR_INVALID_ARG;
    int max_blk = 1;
    for (int f = 0; f < B; ++f) {
        if (box_off_host[f + 1] - box_off_host[f] > kFrameBoxes) return HVPR_ERR_UNSUPPORTED;
        if (!(calib_host[f * kCalib + 24] > 0.f) || !(calib_host[f * kCalib + 25] > 0.f)) return HVPR_ERR_INVALID_ARG;   // img_h, img_w
        max_blk = std::max(max_blk, hvpr_cdiv(pt_off_host[f + 1] - pt_off_host[f], kBlk));
    }
    if (n_obj == 0 && !fov_count) return HVPR_OK;
    if (!workspace) return HVPR_ERR_INVALID_ARG;
    const Ws w = carve(workspace, B, max_blk, n_obj);
    if (workspace_bytes < w.bytes) return HVPR_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    int32_t *fov_blk = fov_count ? w.fov_blk : nullptr;
    if (F == 4 && ((uintptr_t)points & 15) == 0)
        hipLaunchKernelGGL(k_count<true>, dim3(max_blk, B), dim3(kBlk), 0, s, points, F, pt_off, boxes, box_off, calib, w.blk_cnt, fov_blk);
    else
        hipLaunchKernelGGL(k_count<false>, dim3(max_blk, B), dim3(kBlk), 0, s, points, F, pt_off, boxes, box_off, calib, w.blk_cnt, fov_blk);
    HVPR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sum, dim3(n_obj + (fov_count ? B : 0)), dim3(64), 0, s, w.blk_cnt, w.fov_blk, n_obj, max_blk, obj_count, fov_count);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
