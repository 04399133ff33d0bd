// "Attend over k rows" of the training scatter: the second half of get_score,
// pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:76-81, and the aggregation of the memory's training branch,
// map_to_bev/memory_module.py:53-57 —
//
//     w[m, :] = softmax_j( <q[m], rows[r(m, j)]> )      j = 0 .. k-1       (the weights are constants for autograd)
//     out[m]  = sum_j w[m, j] * rows[r(m, j)]
//
// with r(m, j) = idx[m*k + j] (rows picked from one (N, 64) table) or, idx == NULL, r(m, j) = m*k + j (the caller's dense (M, k, 64)
// tensor).  The gathered (M, k, 64) tensor is never written: a pillar's k rows live in registers between the logit pass and the
// weighted sum, so every picked row is fetched once.
//
// Layout: a row is 256 B = one float4 per lane of a 16-lane group; a group owns one pillar, a wave four, a 256-thread block sixteen.
// The 64-term dot product is 4 fmaf per lane (channels 4l .. 4l+3 in ascending order) and an all-lanes sum over the group's 16
// lanes through DPP (two quad permutes, row_half_mirror, row_mirror: a DPP row IS the group, no LDS).  Every lane of the group then
// holds all k logits and evaluates the softmax redundantly (k expf per lane: a fraction of the time the k row loads take), maximum
// subtracted, partition sum and `out` accumulated in ascending j.  The arithmetic of a row depends on its VALUES only — the address
// form (indexed / dense) selects a pointer and nothing else, and every multiply-add is an explicit fmaf — so the dense and the
// indexed call give the same bits for the same rows, and two runs give the same bits.  An index outside [0, N) reads as a row of
// zeros (logit 0, adds nothing), as hvpr_gather_rows_f32 followed by the torch expression did.
//
// KMAX (the unrolled pick count: logits and rows are register arrays with compile-time subscripts, no scratch) is the next of
// 4 / 8 / 16 / 24 / 32 at or above k; picks j >= k are skipped by a wave-uniform test and never enter the arithmetic.
// Bytes to price it by: M*k*256 B of rows + q, idx, out, w.  Backward needs no kernel of its own: the weights are constants, so
// d rows = hvpr_segment_sum_rows_f32(src = d out, edge_row = pick / k, edge_w = w) over the picks sorted by row.
#include "common.h"

namespace {

constexpr int kC = 64;               // channels: one float4 per lane of a 16-lane group
constexpr int kGroup = 16;
constexpr int kBlock = 256;
constexpr int kPillarsPerBlock = kBlock / kGroup;

template <int KMAX>
__global__ void __launch_bounds__(kBlock) k_attend_rows(const float *__restrict__ q, int M, const float *__restrict__ rows, long long N,
                                                        const int *__restrict__ idx, int k, float *__restrict__ out,
                                                        float *__restrict__ w) {
    const int l = threadIdx.x & (kGroup - 1);
    const long long m = (long long)blockIdx.x * kPillarsPerBlock + (threadIdx.x >> 4);
    if (m >= M) return;                                  // a whole 16-lane group leaves together
    const float4 qv = *(const float4 *)(q + (size_t)m * kC + 4 * l);
    const long long e0 = m * k;

    float4 r[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        r[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < k) {
            const long long row = idx ? (long long)idx[e0 + j] : e0 + j;
            if (row >= 0 && row < N) r[j] = *(const float4 *)(rows + (size_t)row * kC + 4 * l);
        }
    }

    float lg[KMAX];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
            float d = qv.x * r[j].x;
            d = fmaf(qv.y, r[j].y, d);
            d = fmaf(qv.z, r[j].z, d);
            d = fmaf(qv.w, r[j].w, d);
            lg[j] = hvpr_reduce_sum<16>(d);
            mx = fmaxf(mx, lg[j]);
        } else {
            lg[j] = 0.f;
        }
    }

    float s = 0.f;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) {
            lg[j] = expf(lg[j] - mx);
            s += lg[j];
        }

    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) {
            const float wj = lg[j] / s;
            acc.x = fmaf(wj, r[j].x, acc.x);
            acc.y = fmaf(wj, r[j].y, acc.y);
            acc.z = fmaf(wj, r[j].z, acc.z);
            acc.w = fmaf(wj, r[j].w, acc.w);
            if ((j & (kGroup - 1)) == l) w[e0 + j] = wj;      // lane j mod 16 writes weight j: 16 consecutive floats per store
        }
    *(float4 *)(out + (size_t)m * kC + 4 * l) = acc;
}

template <int KMAX>
void launch(const float *q, int M, const float *rows, long long N, const int32_t *idx, int k, float *out, float *w, hipStream_t s) {
    hipLaunchKernelGGL(k_attend_rows<KMAX>, dim3(hvpr_cdiv(M, kPillarsPerBlock)), dim3(kBlock), 0, s, q, M, rows, N, idx, k, out, w);
}

}  // namespace

extern "C" int hvpr_attend_rows_fwd_f32(const float *q, int M, const float *rows, long long N, const int32_t *idx, int k, int C,
                                        float *out, float *w, hvpr_stream_t stream) {
    if (M < 0 || N < 0 || k < 0 || C < 0) return HVPR_ERR_INVALID_ARG;
    if (C != kC || k < 1 || k > 32) return HVPR_ERR_UNSUPPORTED;
    if (M == 0) return HVPR_OK;
    if (!q || !rows || !out || !w) return HVPR_ERR_INVALID_ARG;
    if (!idx && N != (long long)M * k) return HVPR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (k <= 4) launch<4>(q, M, rows, N, idx, k, out, w, s);
    else if (k <= 8) launch<8>(q, M, rows, N, idx, k, out, w, s);
    else if (k <= 16) launch<16>(q, M, rows, N, idx, k, out, w, s);
    else if (k <= 24) launch<24>(q, M, rows, N, idx, k, out, w, s);
    else launch<32>(q, M, rows, N, idx, k, out, w, s);
    HVPR_CHECK_LAUNCH();
    return HVPR_OK;
}
