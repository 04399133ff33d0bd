// The bird's-eye-view picture of a batch on the device: the reference's tools/vis.py kitti_vis (:279-286) as one op, from the
// loader's ragged point batch and the padded `sync=False` records to [B, H, W, 3] uint8.
//
// Height pass: _points_to_bevmap_reverse_kernel (:9-60) as points_to_bev (:63-106) and point_to_vis_bev (:109-121) call it for
// kitti_vis, that is with ONE height slice (the z size of a cell is the z extent of the view).  A point belongs to cell
// floor((p - lo) / size) per axis in float32 (a true division) and is dropped when that is < 0 or >= the grid, z included;
// a cell's value is the maximum over its points of (z - z_lo) / (z_hi - z_lo), formed in DOUBLE (height_lowers is np.linspace's
// float64) and rounded to float32 where it is stored (bev_map is float32), starting from 0; bev_map[-1] counts the points of a
// cell.  Every value is >= 0, so the maximum is an unsigned atomic max on the float's bits and the count an integer atomic add:
// no float atomics, the same bytes on every run.  The picture value is uint8(v * 255) with the product in float32.
//
// Box pass: draw_box_in_bev (:223-249).  center_to_corner_box2d's corners in float32 (corners_nd's order (-,-), (-,+), (+,+),
// (+,-) times the sizes; rotation_2d: x' = x cos + y sin, y' = -x sin + y cos, clockwise for a positive angle), plus the centre,
// minus range[:2], times (W, H) / (hi - lo)[:2] -- numpy forms that factor and both in-place updates in float64 and rounds each
// result to the float32 array, and so does this file -- then truncated toward zero (astype(np.int32)).  The reference forms
// THREE segments per box, corners 0-1, 2-3 and 3-0 (bev_lines, :244-246): the edge 1-2 stays open, here too.
// The rasterisation is this project's own (cv2.line is not pinned): pixel p takes a segment's ink when 4 d^2 <= t^2, d the
// distance from p to the integer segment ab, exact in int64: with u = ap . ab and L = |ab|^2, u <= 0 (or L == 0) tests
// 4 |ap|^2 <= t^2, u >= L tests 4 |bp|^2 <= t^2, otherwise 4 cross(ap, ab)^2 <= t^2 L.
//   Bounds: endpoints are clamped to [-kClamp, kClamp] = +-8191 and W, H <= kMaxSide = 8192, so pixels lie in [0, 8191] and every
//   component of ap, bp and ab is at most 16382 < 2^14 in size; a dot or cross product is below 2 * 2^28 = 2^29, 4 cross^2 below
//   2^60, and with t <= kMaxThick = 255, t^2 L < 2^16 * 2^29 = 2^45: nothing leaves int64.
// Where segments of different inks meet the larger ink index wins: an unsigned atomic max on an ink plane, then the compose pass.
// Each workgroup walks the clipped bounding rectangles of ONE box's segments.
//
// Built with -ffp-contract=off: the corner arithmetic is the reference's operation by operation.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kBlk = 256;
constexpr int kMaxSide = 8192;      // W, H
constexpr int kClamp = 8191;        // |endpoint coordinate|
constexpr int kMaxThick = 255;
constexpr int kMaxTableRows = 1 << 20;

struct View {
    float lo_x, lo_y, lo_z, sz_x, sz_y, sz_z;
    float g_x, g_y, g_z;            // the grid as floats: the reference compares the floored quotient with it
    double zlo, zsize, sc_x, sc_y;  // double(lo_z), double(sz_z); W / (hi_x - lo_x), H / (hi_y - lo_y)
    int W, H;
};

struct Table {
    const float *boxes;             // [B, P, stride]
    const int32_t *count;           // [B] or null
    const float *scores;            // [B, P] or null
    const long long *labels;        // [B, P] or null
    float thresh;
    int P, stride, ink;             // ink of a row: ink + label (label 0 without labels)
};

__global__ void __launch_bounds__(kBlk) k_clear(uint32_t *__restrict__ a, uint32_t *__restrict__ b, int32_t *__restrict__ c, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlk) {
        a[i] = 0u;
        b[i] = 0u;
        c[i] = 0;
    }
}

// one thread per point row; the frame of row i is the f with off[f] <= i < off[f + 1]
__global__ void __launch_bounds__(kBlk) k_points(const float *__restrict__ pts, int n, int stride, int col, const int32_t *__restrict__ off,
                                                 int B, View v, uint32_t *__restrict__ height, int32_t *__restrict__ count) {
    const int i = blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = B;                                   // the last f in [0, B) with off[f] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const int f = lo;
    if (i < off[f] || i >= off[f + 1]) return;            // a row no frame owns
    const float *p = pts + (size_t)i * stride + col;
    const float x = p[0], y = p[1], z = p[2];
    const float cx = floorf((x - v.lo_x) / v.sz_x), cy = floorf((y - v.lo_y) / v.sz_y), cz = floorf((z - v.lo_z) / v.sz_z);
    // written so that a NaN fails every test: a non-finite point is dropped
    if (!(cx >= 0.f && cx < v.g_x && cy >= 0.f && cy < v.g_y && cz >= 0.f && cz < v.g_z)) return;
    const size_t cell = ((size_t)f * v.H + (int)cy) * v.W + (int)cx;
    const float h = (float)(((double)z - v.zlo) / v.zsize);
    atomicAdd(count + cell, 1);
    atomicMax(height + cell, __float_as_uint(h));
}

__device__ __forceinline__ bool to_pixel(double c, double lo, double scale, int *out) {
    const float t = (float)((double)c - lo);              // bev_corners -= coors_range[:2]: float64 loop, float32 array
    const float s = (float)((double)t * scale);           // bev_corners *= (W, H) / (hi - lo)
    if (s != s) return false;
    *out = s >= (float)kClamp ? kClamp : (s <= (float)-kClamp ? -kClamp : (int)s);
    return true;
}

__device__ __forceinline__ bool inked(long long px, long long py, long long ax, long long ay, long long bx, long long by, long long tt) {
    const long long abx = bx - ax, aby = by - ay, apx = px - ax, apy = py - ay;
    const long long L = abx * abx + aby * aby, u = apx * abx + apy * aby;
    if (u <= 0 || L == 0) return 4 * (apx * apx + apy * apy) <= tt;
    if (u >= L) {
        const long long bpx = px - bx, bpy = py - by;
        return 4 * (bpx * bpx + bpy * bpy) <= tt;
    }
    const long long cr = apx * aby - apy * abx;
    return 4 * cr * cr <= tt * L;
}

// blockIdx.x: a row of table 0, then of table 1; blockIdx.y: the frame
__global__ void __launch_bounds__(kBlk) k_boxes(Table t0, Table t1, View v, int n_ink, int thick, int sign, uint32_t *__restrict__ ink_plane) {
    const bool second = (int)blockIdx.x >= t0.P;
    const Table &t = second ? t1 : t0;
    const int r = second ? blockIdx.x - t0.P : blockIdx.x, f = blockIdx.y;
    if (t.count && r >= t.count[f]) return;
    const size_t row = (size_t)f * t.P + r;
    if (t.scores && !(t.scores[row] >= t.thresh)) return;
    const long long ink = (long long)t.ink + (t.labels ? t.labels[row] : 0ll);
    if (ink < 1 || ink >= n_ink) return;
    const float *b = t.boxes + row * t.stride;
    const float bx = b[0], by = b[1], bz = b[2], dx = b[3], dy = b[4], dz = b[5], ang = b[6];
    if (!(isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(dx) && isfinite(dy) && isfinite(dz) && isfinite(ang))) return;
    const float a = sign > 0 ? ang : -ang;
    const float sn = sinf(a), cs = cosf(a);
    const float nx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, ny[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
    int qx[4], qy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float x = dx * nx[k], y = dy * ny[k];
        const float rx = x * cs + y * sn, ry = x * -sn + y * cs;
        if (!to_pixel(rx + bx, (double)v.lo_x, v.sc_x, &qx[k]) || !to_pixel(ry + by, (double)v.lo_y, v.sc_y, &qy[k])) return;
    }
    const int s0[3] = {0, 2, 3}, s1[3] = {1, 3, 0};
    const int rad = thick / 2;                            // 4 d^2 <= t^2 reaches floor(t / 2) pixels from the segment
    const long long tt = (long long)thick * thick;
    uint32_t *plane = ink_plane + (size_t)f * v.H * v.W;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int ax = qx[s0[s]], ay = qy[s0[s]], ex = qx[s1[s]], ey = qy[s1[s]];
        const int x0 = max(0, min(ax, ex) - rad), x1 = min(v.W - 1, max(ax, ex) + rad);
        const int y0 = max(0, min(ay, ey) - rad), y1 = min(v.H - 1, max(ay, ey) + rad);
        if (x0 > x1 || y0 > y1) continue;
        const int w = x1 - x0 + 1, area = w * (y1 - y0 + 1);          // at most kMaxSide^2 = 2^26
        for (int i = threadIdx.x; i < area; i += kBlk) {
            const int px = x0 + i % w, py = y0 + i / w;
            if (inked(px, py, ax, ay, ex, ey, tt)) atomicMax(plane + (size_t)py * v.W + px, (uint32_t)ink);
        }
    }
}

__device__ __forceinline__ uint32_t grey_of(uint32_t bits) {
    const float g = __uint_as_float(bits) * 255.0f;
    return g >= 255.0f ? 255u : (uint32_t)(int)g;
}

// four pixels (twelve bytes, three 32-bit stores) per thread; the last n % 4 pixels byte by byte
__global__ void __launch_bounds__(kBlk) k_compose(const uint32_t *__restrict__ height, const uint32_t *__restrict__ ink_plane,
                                                  const uint8_t *__restrict__ palette, size_t n, uint8_t *__restrict__ image, int aligned) {
    const size_t q = ((size_t)blockIdx.x * kBlk + threadIdx.x) * 4;
    if (q >= n) return;
    uint8_t px[12];
    const int m = (int)min((size_t)4, n - q);
    for (int k = 0; k < m; ++k) {
        const uint32_t ink = ink_plane[q + k];
        if (ink) {
            px[3 * k] = palette[3 * ink]; px[3 * k + 1] = palette[3 * ink + 1]; px[3 * k + 2] = palette[3 * ink + 2];
        } else {
            px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = (uint8_t)grey_of(height[q + k]);
        }
    }
    if (m == 4 && aligned) {
        uint32_t *o = reinterpret_cast<uint32_t *>(image + q * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * m; ++k) image[q * 3 + k] = px[k];
    }
}

struct Ws { uint32_t *height, *ink; int32_t *count; size_t bytes; };

Ws carve(void *base, size_t cells) {
    hvpr_carver cv(base);
    Ws w;
    w.height = cv.take<uint32_t>(cells);
    w.ink = cv.take<uint32_t>(cells);
    w.count = cv.take<int32_t>(cells);
    w.bytes = cv.off;
    return w;
}

// round((hi - lo) / size) in float32, np.round's ties to even; 0 when it is not a side this file takes
int side_of(float lo, float hi, float size) {
    const float d = hi - lo;
    const float q = d / size;
    const float r = nearbyintf(q);
    if (!(r >= 1.f)) return 0;
    return r > (float)kMaxSide ? kMaxSide + 1 : (int)r;
}

bool table_ok(const float *boxes, int P, int stride) { return !boxes || (P >= 0 && stride >= 7); }

}  // namespace

extern "C" size_t hvpr_render_bev_workspace_bytes(int batch, int height, int width) {
    if (batch < 1 || height < 1 || width < 1 || height > kMaxSide || width > kMaxSide) return 0;
    if ((long long)batch * height * width > 0x7fffffffLL) return 0;
    return carve(nullptr, (size_t)batch * height * width).bytes;
}

extern "C" int hvpr_render_bev_u8(const float *points, long long n_points, int point_stride, int xyz_col, const int32_t *frame_offsets,
                                  int batch, const float *range, float pixel, const float *boxes0, int rows0, int box_stride0,
                                  const int32_t *count0, const float *scores0, float thresh0, const long long *labels0, int ink0,
                                  const float *boxes1, int rows1, int box_stride1, const int32_t *count1, const float *scores1,
                                  float thresh1, const long long *labels1, int ink1, const uint8_t *palette, int n_ink,
                                  int thickness, int heading_sign, uint8_t *image, int32_t *counts, void *workspace,
                                  size_t workspace_bytes, hvpr_stream_t stream) {
    if (batch < 1 || n_points < 0 || !frame_offsets || !range || !image || !palette || n_ink < 1 || (n_points > 0 && !points) ||
        point_stride < 3 || xyz_col < 0 || xyz_col + 3 > point_stride || thickness < 1 || (heading_sign != 1 && heading_sign != -1) ||
        !table_ok(boxes0, rows0, box_stride0) || !table_ok(boxes1, rows1, box_stride1))
        return HVPR_ERR_INVALID_ARG;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(range[k])) return HVPR_ERR_INVALID_ARG;
    if (!(pixel > 0.f) || !std::isfinite(pixel) || !(range[3] > range[0]) || !(range[4] > range[1]) || !(range[5] > range[2]))
        return HVPR_ERR_INVALID_ARG;
    View v;
    v.lo_x = range[0]; v.lo_y = range[1]; v.lo_z = range[2];
    v.sz_x = pixel; v.sz_y = pixel; v.sz_z = range[5] - range[2];          // one height slice (point_to_vis_bev, :117)
    v.W = side_of(range[0], range[3], pixel);
    v.H = side_of(range[1], range[4], pixel);
    if (v.W < 1 || v.H < 1 || !(v.sz_z > 0.f) || !std::isfinite(v.sz_z)) return HVPR_ERR_INVALID_ARG;
    const int P0 = boxes0 ? rows0 : 0, P1 = boxes1 ? rows1 : 0;
    if (v.W > kMaxSide || v.H > kMaxSide || thickness > kMaxThick || n_points > 0x7fffffffLL || batch > 65535 ||
        (long long)batch * v.H * v.W > 0x7fffffffLL || P0 > kMaxTableRows || P1 > kMaxTableRows || n_ink > (1 << 24))
        return HVPR_ERR_UNSUPPORTED;
    v.g_x = (float)v.W; v.g_y = (float)v.H; v.g_z = nearbyintf((range[5] - range[2]) / v.sz_z);
    v.zlo = (double)range[2]; v.zsize = (double)v.sz_z;
    v.sc_x = (double)v.W / ((double)range[3] - (double)range[0]);
    v.sc_y = (double)v.H / ((double)range[4] - (double)range[1]);
    if (!workspace) return HVPR_ERR_INVALID_ARG;
    const size_t cells = (size_t)batch * v.H * v.W;
    const Ws w = carve(workspace, cells);
    if (workspace_bytes < w.bytes) return HVPR_ERR_WORKSPACE;
    int32_t *cnt = counts ? counts : w.count;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_clear, dim3(std::min<long long>(hvpr_cdiv(cells, kBlk), 4096)), dim3(kBlk), 0, s, w.height, w.ink, cnt, cells);
    HVPR_CHECK_LAUNCH();
    if (n_points > 0) {
        hipLaunchKernelGGL(k_points, dim3(hvpr_cdiv(n_points, kBlk)), dim3(kBlk), 0, s, points, (int)n_points, point_stride, xyz_col,
                           frame_offsets, batch, v, w.height, cnt);
        HVPR_CHECK_LAUNCH();
    }
    if (P0 + P1 > 0) {
        const Table t0 = {boxes0, count0, scores0, labels0, thresh0, P0, box_stride0, ink0};
        const Table t1 = {boxes1, count1, scores1, labels1, thresh1, P1, box_stride1, ink1};
        hipLaunchKernelGGL(k_boxes, dim3(P0 + P1, batch), dim3(kBlk), 0, s, t0, t1, v, n_ink, thickness, heading_sign, w.ink);
        HVPR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_compose, dim3(hvpr_cdiv(hvpr_cdiv(cells, 4), kBlk)), dim3(kBlk), 0, s, w.height, w.ink, palette, cells, image,
                       (int)(((uintptr_t)image & 3) == 0));
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
