// a2 (plain) — the pillar encoder of plain PointPillars, eval mode: PillarVFE.forward (pcdet/models/backbones_3d/vfe/pillar_vfe.py:94-124)
// with ONE PFNLayer (:29-49), BatchNorm folded into w / b by the caller, USE_ABSLOTE_XYZ=True, WITH_DISTANCE=False, 4 raw features.
//
// A pillar per wave (the separate-call precedent: k_vfe_rows, vfe.hip), in two lane roles:
//   lane = slot      loads its point (lanes >= P hold zeros), so one round trip brings the pillar in.
//     mean           the sum over ALL P slots (the padding is zeros, :97) by the DPP tree of hvpr_reduce_sum<64>, divided by float(n).
//     decoration     raw 4, xyz - mean, xyz - (cell * voxel + offset); the ten of them times (slot < n) (:98-118).  This file is built
//                    without FMA contraction, so every one of these roundings is the reference's; only the order of the mean's sum
//                    differs.
//   lane = channel   keeps row `lane` of the layer (rows lane and lane + 64 at c_out = 128; at c_out = 32 the upper half repeats
//                    the lower one) in registers for the whole kernel: ten weights and the bias.
//     layer          the LIVE slots one after the other: slot s's ten features leave lane s by v_readlane and reach every lane's
//                    ten fmaf as scalar operands.  A KITTI pillar holds 4.4 points on average: the work follows the points, not P.
//     maximum        in the lane, starting from 0 (that is the ReLU).  The reference takes it over ALL P slots (:42), padded ones
//                    included; a padded slot's features are zeros, so it contributes ReLU(b[c]): one
//                    max(y, b[c]) for a pillar with n < P.  Nothing crosses lanes, and a row leaves in one coalesced store.
// The words of the wave's next pillar are requested before the current one is worked on.  A row with num_points == 0 divides by zero
// as the reference does, uses none of it and comes out as ReLU(b); every address depends only on the row index and the lane, never on
// num_points.
#include "common.h"

namespace {

constexpr int CIN = 10;   // x y z r + cluster(3) + center(3)

struct PillarIn {
    float4 pt;
    int n;
    int4 cd;
};

__device__ __forceinline__ PillarIn fetch(const float4 *__restrict__ voxels, const int *__restrict__ num_points,
                                          const int4 *__restrict__ coords, int p, int M, int P, int lane) {
    PillarIn in{make_float4(0.f, 0.f, 0.f, 0.f), 1, make_int4(0, 0, 0, 0)};
    if (p < M) {
        in.n = num_points[p];
        in.cd = coords[p];
        if (lane < P) in.pt = voxels[(size_t)p * P + lane];
    }
    return in;
}

__device__ __forceinline__ float bcast(float v, int src_lane) {   // src_lane: uniform over the wave
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

template <int C>
__global__ void __launch_bounds__(256) k_vfe_plain(const float4 *__restrict__ voxels, const int *__restrict__ num_points,
                                                   const int4 *__restrict__ coords, int M, int P, const int *__restrict__ m_device,
                                                   float vsx, float vsy, float vsz, float offx, float offy, float offz,
                                                   const float *__restrict__ w, const float *__restrict__ b,
                                                   float *__restrict__ pillar_features, float *__restrict__ pillar_mask) {
    constexpr int PER = C > 64 ? C / 64 : 1;   // rows of the layer per lane
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    if (m_device) M = min(M, *m_device);
    const int ch = C >= 64 ? lane : (lane & (C - 1));
    float wr[PER][CIN], br[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        br[j] = b[ch + 64 * j];
#pragma unroll
        for (int k = 0; k < CIN; ++k) wr[j][k] = w[(ch + 64 * j) * CIN + k];
    }
    PillarIn in = fetch(voxels, num_points, coords, wave, M, P, lane);
    for (int p = wave; p < M; p += n_waves) {
        const PillarIn next = fetch(voxels, num_points, coords, p + n_waves, M, P, lane);
        const float4 pt = in.pt;
        const int n = __builtin_amdgcn_readfirstlane(in.n);
        const int4 cd = in.cd;
        const float live = (lane < n && lane < P) ? 1.f : 0.f;
        if (pillar_mask && lane < P) pillar_mask[(size_t)p * P + lane] = live;
        const float fn = (float)n;
        const float mx = hvpr_reduce_sum<64>(pt.x) / fn, my = hvpr_reduce_sum<64>(pt.y) / fn, mz = hvpr_reduce_sum<64>(pt.z) / fn;
        float f[CIN];
        f[0] = pt.x * live; f[1] = pt.y * live; f[2] = pt.z * live; f[3] = pt.w * live;
        f[4] = (pt.x - mx) * live; f[5] = (pt.y - my) * live; f[6] = (pt.z - mz) * live;
        f[7] = (pt.x - ((float)cd.w * vsx + offx)) * live;
        f[8] = (pt.y - ((float)cd.z * vsy + offy)) * live;
        f[9] = (pt.z - ((float)cd.y * vsz + offz)) * live;
        float y[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) y[j] = 0.f;
        const int n_live = n < 0 ? 0 : (n > P ? P : n);
        for (int s = 0; s < n_live; ++s) {
            float fs[CIN];
#pragma unroll
            for (int k = 0; k < CIN; ++k) fs[k] = bcast(f[k], s);
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                float acc = br[j];
#pragma unroll
                for (int k = 0; k < CIN; ++k) acc = fmaf(wr[j][k], fs[k], acc);
                y[j] = fmaxf(y[j], acc);
            }
        }
        if (n < P) {   // the padded slots: all-zero features, bias alone
#pragma unroll
            for (int j = 0; j < PER; ++j) y[j] = fmaxf(y[j], br[j]);
        }
        if (C >= 64 || lane < C) {
#pragma unroll
            for (int j = 0; j < PER; ++j) pillar_features[(size_t)p * C + ch + 64 * j] = y[j];
        }
        in = next;
    }
}

template <int C>
void launch(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P, const int32_t *m_device, float vs_x,
            float vs_y, float vs_z, float off_x, float off_y, float off_z, const float *w, const float *b, float *pillar_features,
            float *pillar_mask, hipStream_t s) {
    int blocks = hvpr_cdiv(M, 4);   // four waves, a pillar each
    if (blocks > 2048) blocks = 2048;   // beyond eight workgroups per CU the waves stride over the rows
    hipLaunchKernelGGL(k_vfe_plain<C>, dim3(blocks), dim3(256), 0, s, (const float4 *)voxels, num_points, (const int4 *)coords, M, P,
                       m_device, vs_x, vs_y, vs_z, off_x, off_y, off_z, w, b, pillar_features, pillar_mask);
}

}  // namespace

extern "C" int hvpr_pillar_vfe_plain_fwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P,
                                             const int32_t *m_device, float vs_x, float vs_y, float vs_z, float off_x, float off_y,
                                             float off_z, const float *w, const float *b, int c_out, float *pillar_features,
                                             float *pillar_mask, hvpr_stream_t stream) {
    if (M < 0 || P < 1 || c_out < 1) return HVPR_ERR_INVALID_ARG;
    if (P > 32 || (c_out != 32 && c_out != 64 && c_out != 128)) return HVPR_ERR_UNSUPPORTED;
    if (M == 0) return HVPR_OK;
    if (!voxels || !num_points || !coords || !w || !b || !pillar_features) return HVPR_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
#define HVPR_PLAIN_ARGS voxels, num_points, coords, M, P, m_device, vs_x, vs_y, vs_z, off_x, off_y, off_z, w, b, pillar_features, pillar_mask, s
    if (c_out == 32) launch<32>(HVPR_PLAIN_ARGS);
    else if (c_out == 64) launch<64>(HVPR_PLAIN_ARGS);
    else launch<128>(HVPR_PLAIN_ARGS);
#undef HVPR_PLAIN_ARGS
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
