// Shared device/host helpers for the hvpr_amd HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hvpr_amd.h"

#define HVPR_WAVE 64

#include "wave.h"

#define HVPR_CHECK_LAUNCH()                                   \
    do {                                                      \
        if (hipGetLastError() != hipSuccess) return HVPR_ERR_LAUNCH; \
    } while (0)

static inline int hvpr_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// SyncBatchNorm (abi.hip): sums buf[0..n) over the ranks through the caller's hook, ordered on `s`; 0 without a hook / on success
int hvpr_i_bn_allreduce(double *buf, int n, hipStream_t s);

// 256-byte aligned carve helper for workspaces
struct hvpr_carver {
    char *base;
    size_t off;
    explicit hvpr_carver(void *p) : base((char *)p), off(0) {}
    template <typename T>
    T *take(size_t n) {
        T *r = (T *)(base + off);
        off += ((n * sizeof(T) + 255) / 256) * 256;
        return r;
    }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device only: remember it per device (bit d of a
// per-call-site mask), not once per process.  The call is idempotent, so a lost update only repeats it.
static inline int hvpr_ensure_dyn_lds(const void *fn, int bytes, unsigned long long *done_mask) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev >= 0 && dev < 64 && ((__atomic_load_n(done_mask, __ATOMIC_RELAXED) >> dev) & 1ull)) return 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return -1;
    if (dev >= 0 && dev < 64) __atomic_fetch_or(done_mask, 1ull << dev, __ATOMIC_RELAXED);
    return 0;
}

__device__ __forceinline__ int hvpr_lane() { return threadIdx.x & 63; }

// One workgroup (a multiple of 64 threads): dst[i] = base + get(0) + ... + get(i - 1) for i in [0, n); with `total`, dst[n] = base
// + the sum of all.  A contiguous piece per thread, the pieces' sums scanned over the wave (hvpr_wave_scan_incl) and over the waves
// through `wave_sum`, the caller's LDS array of one int per wave.  Ends with a barrier: the workgroup may read dst and use
// `wave_sum` again.
template <typename Get>
__device__ __forceinline__ void hvpr_block_scan(Get get, int n, int base, int32_t *dst, bool total, int *wave_sum) {
    const int T = blockDim.x, t = threadIdx.x, ln = t & 63, wv = t >> 6, per = (n + T - 1) / T;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += get(i);
    const int inc = hvpr_wave_scan_incl(s);
    if (ln == 63) wave_sum[wv] = inc;
    __syncthreads();
    int run = base + inc - s;
    for (int w = 0; w < wv; ++w) run += wave_sum[w];
    for (int i = lo; i < hi; ++i) { const int v = get(i); dst[i] = run; run += v; }
    if (total && t == T - 1) dst[n] = run;                             // the last piece ends at n
    __syncthreads();
}

// All-lanes reductions over the 64-lane wave, within its 32-lane halves or within its 16-lane rows (the first four steps of the
// same tree), without the LDS crossbar: two quad permutes, the two row mirrors (after the quad steps every lane of a quad holds
// the same value, so mirroring combines exactly the groups an xor butterfly would), then v_permlane16_swap / v_permlane32_swap
// (gfx950) across the 16-lane rows.  Same reduction tree as the __shfl_xor butterfly — bit-identical results, commutativity aside
// nothing changes — at a few VALU cycles per step instead of a ds_bpermute round trip (~60+ cycles each: 95 of them were 3 us of
// the pillar VFE).  The two quad permutes are the control words of hvpr_xchg<1> / hvpr_xchg<2> (wave.h), which hands back the
// partner's value; the mirrors have no exchange form, so the steps stay spelled out here.
template <int CTRL>
__device__ __forceinline__ float hvpr_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
struct hvpr_op_sum { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct hvpr_op_max { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
template <int WIDTH, typename Op>
__device__ __forceinline__ float hvpr_reduce(float v, Op op) {
    static_assert(WIDTH == 16 || WIDTH == 32 || WIDTH == 64, "a 16-lane row, a wave half or the whole wave");
    v = op(v, hvpr_dpp<0xB1>(v));    // quad_perm [1,0,3,2]
    v = op(v, hvpr_dpp<0x4E>(v));    // quad_perm [2,3,0,1]
    v = op(v, hvpr_dpp<0x141>(v));   // row_half_mirror
    v = op(v, hvpr_dpp<0x140>(v));   // row_mirror
    if (WIDTH >= 32) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    if (WIDTH == 64) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    return v;
}
template <int WIDTH>
__device__ __forceinline__ float hvpr_reduce_sum(float v) { return hvpr_reduce<WIDTH>(v, hvpr_op_sum()); }
template <int WIDTH>
__device__ __forceinline__ float hvpr_reduce_max(float v) { return hvpr_reduce<WIDTH>(v, hvpr_op_max()); }
