// "Point inside a rotated box", shared by augment.hip (the scene points under a pasted candidate) and gt_database.hip (the
// points that become a database object), so that a database built by one and pasted by the other decides alike on every point:
// the fp32 operations of csrc_cpu/gt_sampling.cpp:95-107 in their order.
// Every including file is compiled with -ffp-contract=off: no product below may fuse with its sum.
#pragma once
#include <hip/hip_runtime.h>

struct hvpr_cut { float x, y, z, hx, hy, hz, cs, sn; };

// b: a box row (x, y, z, dx, dy, dz, heading), each size enlarged by its extra width (box_utils.enlarge_box3d)
__device__ __forceinline__ hvpr_cut hvpr_make_cut(const float *b, float ex, float ey, float ez) {
    hvpr_cut c;                                    // cosf / sinf first: they need the most registers, nothing else is live yet
    c.cs = cosf(-b[6]); c.sn = sinf(-b[6]);
    c.x = b[0]; c.y = b[1]; c.z = b[2];
    c.hx = (b[3] + ex) / 2.0f; c.hy = (b[4] + ey) / 2.0f; c.hz = (b[5] + ez) / 2.0f;
    return c;
}

__device__ __forceinline__ bool hvpr_cut_inside(const hvpr_cut &c, float x, float y, float z) {
    if (!(fabsf(z - c.z) <= c.hz)) return false;
    const float sx = x - c.x, sy = y - c.y;
    const float lx = sx * c.cs - sy * c.sn, ly = sx * c.sn + sy * c.cs;
    return fabsf(lx) < c.hx && fabsf(ly) < c.hy;
}
