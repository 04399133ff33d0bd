// The rotated-BEV geometry shared by the kernels that test boxes against boxes: iou3d_nms.hip (pairwise tables, NMS),
// augment.hip (the collision test of GT sampling) and eval_tail.hip (the recall record).  ONE copy: the fp32 sequence below is the one the CPU oracle
// (oracle/iou3d_nms_ref.c) runs, and every file that includes this header is compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace {

constexpr float kEps = 1e-8f;
constexpr float kMargin = 1e-2f;

struct P2 { float x, y; };

__device__ __forceinline__ float cross3(P2 a, P2 b, P2 o) { return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y); }

__device__ __forceinline__ bool rect_overlap(P2 p1, P2 p2, P2 q1, P2 q2) {
    return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
           fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

__device__ __forceinline__ bool seg_intersect(P2 p1, P2 p0, P2 q1, P2 q0, P2 &out) {
    if (!rect_overlap(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0.0f && s3 * s4 > 0.0f)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > kEps) {
        out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        out.x = (b0 * c1 - b1 * c0) / D;
        out.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

struct Box {
    float x, y, dx, dy, r;   // BEV part
    float cs, sn;            // cos/sin(heading)
    float ncs, nsn;          // cos/sin(-heading)
    P2 c[5];                 // rotated corners, closed
};

__device__ __forceinline__ void make_box(const float *__restrict__ b, Box &B) {
    B.x = b[0]; B.y = b[1]; B.dx = b[3]; B.dy = b[4]; B.r = b[6];
    B.cs = cosf(B.r); B.sn = sinf(B.r);
    B.ncs = cosf(-B.r); B.nsn = sinf(-B.r);
    const float hx = B.dx / 2, hy = B.dy / 2;
    const float x1 = B.x - hx, y1 = B.y - hy, x2 = B.x + hx, y2 = B.y + hy;
    const float rx[4] = {x1, x2, x2, x1}, ry[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        B.c[k].x = (rx[k] - B.x) * B.cs + (ry[k] - B.y) * (-B.sn) + B.x;
        B.c[k].y = (rx[k] - B.x) * B.sn + (ry[k] - B.y) * B.cs + B.y;
    }
    B.c[4] = B.c[0];
}

__device__ __forceinline__ bool in_box(const Box &B, P2 p) {
    const float rx = (p.x - B.x) * B.ncs + (p.y - B.y) * (-B.nsn);
    const float ry = (p.x - B.x) * B.nsn + (p.y - B.y) * B.ncs;
    return fabsf(rx) < B.dx / 2 + kMargin && fabsf(ry) < B.dy / 2 + kMargin;
}

// Exact reject: if the centres are farther apart than the two circum-radii plus the in-box margin, no edge pair can
// intersect and no corner can pass the margin test, so the polygon routine would return exactly 0.
__device__ __forceinline__ bool far_apart(const Box &A, const Box &B) {
    const float ra = 0.5f * sqrtf(A.dx * A.dx + A.dy * A.dy), rb = 0.5f * sqrtf(B.dx * B.dx + B.dy * B.dy);
    const float ddx = A.x - B.x, ddy = A.y - B.y;
    const float lim = ra + rb + 0.05f;
    return ddx * ddx + ddy * ddy > lim * lim * 1.0001f;
}

// What the two rejects need of a box, for the sweeps that run them over a whole table (assign_common.h); rad is far_apart's ra / rb,
// the same expression.
struct BoxLite { float x, y, hx, hy, cs, sn, rad, pad; };   // 32 bytes: two broadcast 16-byte LDS reads

__device__ __forceinline__ BoxLite lite_of(const Box &B) {
    return BoxLite{B.x, B.y, 0.5f * B.dx, 0.5f * B.dy, B.cs, B.sn, 0.5f * sqrtf(B.dx * B.dx + B.dy * B.dy), 0.f};
}

// far_apart on the BoxLite records.  A sweep counts a rejected pair as IoU +0, which holds only while this IS the test above: change
// them together (tests/test_gpu_assign3d.py and tests/test_gpu_atss.py compare the sweeps with hvpr_boxes_pairwise_f32's table, which
// runs the Box form).
__device__ __forceinline__ bool far_apart(const BoxLite &A, const BoxLite &B) {
    const float ddx = A.x - B.x, ddy = A.y - B.y;
    const float lim = A.rad + B.rad + 0.05f;
    return ddx * ddx + ddy * ddy > lim * lim * 1.0001f;
}

// Exact reject no. 2, separating axes: if the two rectangles are more than 5 cm apart along one of their four edge
// normals, no edges cross and no corner passes the 1 cm in-box margin (that margin widens a box by at most 1.42 cm in any
// direction), so the polygon routine would return exactly 0.  About half of the pairs the circum-circle test lets through
// (cars: circum-radius 2.1 m around a 3.9 x 1.6 m box) end here, for ~35 flops instead of the ~18 k-cycle clip.
// branch-free (all lanes run it on densely packed pairs)
__device__ __forceinline__ bool axes_separate(const BoxLite &A, const BoxLite &B) {
    const float ddx = B.x - A.x, ddy = B.y - A.y;
    const float c = fabsf(A.cs * B.cs + A.sn * B.sn), sn = fabsf(B.sn * A.cs - B.cs * A.sn);   // |cos|, |sin| of the heading difference
    const float m = 0.05f;
    const bool s0 = fabsf(ddx * A.cs + ddy * A.sn) > A.hx + B.hx * c + B.hy * sn + m;
    const bool s1 = fabsf(ddy * A.cs - ddx * A.sn) > A.hy + B.hx * sn + B.hy * c + m;
    const bool s2 = fabsf(ddx * B.cs + ddy * B.sn) > B.hx + A.hx * c + A.hy * sn + m;
    const bool s3 = fabsf(ddy * B.cs - ddx * B.sn) > B.hy + A.hx * sn + A.hy * c + m;
    return s0 | s1 | s2 | s3;
}

// Per-lane polygon scratch in LDS: up to 24 candidate vertices (16 edge crossings + 8 corners), lane-minor so that
// dynamic indexing is a conflict-free ds access.  (As a private array this spills to scratch memory: 300 B/lane and
// an order of magnitude slower.)
struct PolyStore {
    float x[24][64], y[24][64], a[24][64];
};

__device__ float box_overlap(const Box &A, const Box &B, PolyStore &ps, int ln) {
    if (far_apart(A, B)) return 0.0f;
    int cnt = 0;
    P2 ctr = {0.0f, 0.0f};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            P2 o;
            if (seg_intersect(A.c[i + 1], A.c[i], B.c[j + 1], B.c[j], o)) {
                ps.x[cnt][ln] = o.x; ps.y[cnt][ln] = o.y; ctr.x += o.x; ctr.y += o.y; ++cnt;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (in_box(A, B.c[k])) { ctr.x += B.c[k].x; ctr.y += B.c[k].y; ps.x[cnt][ln] = B.c[k].x; ps.y[cnt][ln] = B.c[k].y; ++cnt; }
        if (in_box(B, A.c[k])) { ctr.x += A.c[k].x; ctr.y += A.c[k].y; ps.x[cnt][ln] = A.c[k].x; ps.y[cnt][ln] = A.c[k].y; ++cnt; }
    }
    if (cnt == 0) return 0.0f;
    ctr.x /= (float)cnt; ctr.y /= (float)cnt;
    // bubble sort by polar angle: the angle of a vertex does not change while it is moved around, so it is computed
    // once per vertex instead of twice per comparison (identical comparisons, identical order)
    for (int i = 0; i < cnt; ++i) ps.a[i][ln] = atan2f(ps.y[i][ln] - ctr.y, ps.x[i][ln] - ctr.x);
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i) {
            const float a0 = ps.a[i][ln], a1 = ps.a[i + 1][ln];
            if (a0 > a1) {
                const float tx = ps.x[i][ln], ty = ps.y[i][ln];
                ps.x[i][ln] = ps.x[i + 1][ln]; ps.y[i][ln] = ps.y[i + 1][ln]; ps.a[i][ln] = a1;
                ps.x[i + 1][ln] = tx; ps.y[i + 1][ln] = ty; ps.a[i + 1][ln] = a0;
            }
        }
    float area = 0.0f;
    const float x0 = ps.x[0][ln], y0 = ps.y[0][ln];
    for (int k = 0; k < cnt - 1; ++k) {
        const float ux = ps.x[k][ln] - x0, uy = ps.y[k][ln] - y0;
        const float wx = ps.x[k + 1][ln] - x0, wy = ps.y[k + 1][ln] - y0;
        area += ux * wy - uy * wx;
    }
    return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev(const Box &A, const Box &B, PolyStore &ps, int ln) {
    const float sa = A.dx * A.dy, sb = B.dx * B.dy;
    const float so = box_overlap(A, B, ps, ln);
    return so / fmaxf(sa + sb - so, kEps);
}

// 3-D IoU of the rows pa / pb that A / B were made from: BEV overlap times the common height over the union volume (the
// upstream boxes_iou3d_gpu).  ONE copy for the pairwise table (iou3d_nms.hip) and the recall record (eval_tail.hip).
__device__ __forceinline__ float iou_3d(const float *__restrict__ pa, const float *__restrict__ pb, const Box &A, const Box &B,
                                        PolyStore &ps, int ln) {
    const float a_top = pa[2] + pa[5] / 2, a_bot = pa[2] - pa[5] / 2;
    const float b_top = pb[2] + pb[5] / 2, b_bot = pb[2] - pb[5] / 2;
    const float va = pa[3] * pa[4] * pa[5], vb = pb[3] * pb[4] * pb[5];
    const float ob = box_overlap(A, B, ps, ln);
    const float oh = fmaxf(fminf(a_top, b_top) - fmaxf(a_bot, b_bot), 0.0f);
    const float o3 = ob * oh;
    return o3 / fmaxf(va + vb - o3, 1e-6f);
}

}  // namespace
