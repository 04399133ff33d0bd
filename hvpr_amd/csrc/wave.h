// Wave-level building blocks, ONE copy of each (included from common.h): ordered float keys, the raw maximum, lane exchanges, the
// bitonic network, the inclusive scan, the xor butterflies, the frame of a row and the stamps of the timing build.  They decide
// bits the tests pin exactly — tie order of the top-k, selection in the read-out and FPS, point order inside a pillar, the NMS pair
// lists — so a correction has to reach every kernel from here.  Included from files built with and without -ffp-contract=off:
// nothing in here multiplies and then adds.  The first part also compiles for the host (tools/check_wave_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HVPR_WAVE_HD __host__ __device__ __forceinline__
#else
#define HVPR_WAVE_HD inline
#endif

// Order-preserving map float -> unsigned: a < b  <=>  hvpr_ord_of(a) < hvpr_ord_of(b) for every pair that is not NaN, key 0 lies
// below every float (the "empty" value of the atomicMax planes and of idle lanes), hvpr_of_ord inverts it.  -0.0 gets the key just
// below +0.0's, although the two compare equal: the assigners and the read-out compare keys only with keys of the same map and
// read values back through hvpr_of_ord, so the step that merges the two zeros does NOT belong here (it would lose the sign on the
// way back).  The one caller whose tie order needs it wraps this map: topk_ord in postprocess.hip.
HVPR_WAVE_HD unsigned hvpr_ord_of_bits(unsigned b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }   // b: the float's bits
HVPR_WAVE_HD unsigned hvpr_ord_of(float v) { return hvpr_ord_of_bits(__builtin_bit_cast(unsigned, v)); }
HVPR_WAVE_HD float hvpr_of_ord(unsigned o) { return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// Frame of a row: the largest b in [0, B) with off[b] <= row, for off[0] <= row < off[B] (an empty frame repeats its offset and is
// never found).
HVPR_WAVE_HD int hvpr_frame_of(const int32_t *off, int B, int row) {
    int lo = 0, hi = B;   // invariant: off[lo] <= row
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

#if defined(__HIPCC__)

// timing build (python -m hvpr_amd.build --timing): in-kernel stamps; in every other build the arguments vanish.  HVPR_STAMP waits
// for the memory counters, then reads the cycle counter into array[i].
#ifdef HVPR_EXP_TIMING
#define HVPR_IF_TIMING(...) __VA_ARGS__
#else
#define HVPR_IF_TIMING(...)
#endif
#define HVPR_STAMP(array, i) \
    HVPR_IF_TIMING(do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); (array)[i] = __builtin_readcyclecounter(); } while (0))

// v_max_f32 as is: fmaxf() first quiets both operands (two more instructions per max under the IEEE mode bit)
__device__ __forceinline__ float hvpr_vmax_raw(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
struct hvpr_op_max_raw { __device__ __forceinline__ float operator()(float a, float b) const { return hvpr_vmax_raw(a, b); } };

// Lane l <-> lane l ^ J on a 32-bit value without the LDS crossbar: quad permutes (1, 2), two row shifts into alternating banks
// (4: row_shl:4 into banks 0 and 2, row_shr:4 into banks 1 and 3), row_ror:8, then v_permlane16_swap / v_permlane32_swap (gfx950).
// The swaps exchange the odd rows (halves) of their first operand with the even ones of their second: with the same value in both,
// result 0 holds the even side's value and result 1 the odd side's on BOTH sides, so the partner's is result 1 for an even-side
// lane and result 0 for an odd-side one.
template <int J, typename T>
__device__ __forceinline__ T hvpr_xchg(T v) {
    static_assert(sizeof(T) == 4 && (J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32), "a 32-bit value, one lane bit");
    const int iv = __builtin_bit_cast(int, v);
    if (J == 1) return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, iv, 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    if (J == 2) return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, iv, 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    if (J == 4) {
        const int r = __builtin_amdgcn_update_dpp(0, iv, 0x104, 0xf, 0x5, false);
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(r, iv, 0x114, 0xf, 0xa, false));
    }
    if (J == 8) return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, iv, 0x128, 0xf, 0xf, true));   // row_ror:8
    if (J == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)iv, (unsigned)iv, false, false);
        return __builtin_bit_cast(T, (threadIdx.x & 16) ? r[0] : r[1]);
    }
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)iv, (unsigned)iv, false, false);
    return __builtin_bit_cast(T, (threadIdx.x & 32) ? r[0] : r[1]);
}

// Ascending bitonic sort of one key per lane inside every aligned group of `width` lanes, 32 or 64 (`lane`: the lane's index in its
// group or in the wave), exchanging through __shfl_xor.  `width` is an argument, not a template parameter, and the loops carry no
// unroll pragma: k_vfe_gather keeps its instruction stream only in this form (profiles/NOTES_r25.md, section 2) ...
__device__ __forceinline__ int hvpr_bitonic_asc(int v, int lane, int width) {
    for (int k = 2; k <= width; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = __shfl_xor(v, j, 64);
            const bool up = (lane & k) == 0;
            const bool lower = (lane & j) == 0;
            v = (lower == up) ? min(v, o) : max(v, o);
        }
    }
    return v;
}
// ... and the same network for the 32-lane halves on hvpr_xchg
__device__ __forceinline__ unsigned hvpr_bitonic32_asc_dpp(unsigned v, int col) {
#pragma unroll
    for (int k = 2; k <= 32; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned o = j == 1 ? hvpr_xchg<1>(v) : j == 2 ? hvpr_xchg<2>(v) : j == 4 ? hvpr_xchg<4>(v) : j == 8 ? hvpr_xchg<8>(v)
                                                                                                          : hvpr_xchg<16>(v);
            const bool up = (col & k) == 0;
            const bool lower = (col & j) == 0;
            v = (lower == up) ? min(v, o) : max(v, o);
        }
    }
    return v;
}

// Inclusive add-scan of a 32-bit integer over the 64 lanes on DPP moves (row_shr inside the 16-lane rows, row_bcast across them):
// ~10 instructions per value instead of six ds_bpermute round trips.
template <typename T>
__device__ __forceinline__ T hvpr_wave_scan_incl(T x) {
    static_assert(sizeof(T) == 4 && __is_integral(T), "a 32-bit integer");
    unsigned v = (unsigned)x;
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);     // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);     // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);     // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);     // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);    // row_bcast:15 -> rows 1, 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);    // row_bcast:31 -> rows 2, 3
    return (T)v;
}
// The same scan on __shfl_up, two values at a time and as a MACRO (see the butterflies below for why), for k2_scan (voxelize.hip)
// alone: with either scan as a function its register allocation comes out 38 -> 39 (ITEMS = 2) and 74 -> 82 (ITEMS = 8) VGPRs,
// whichever body the function has (profiles/NOTES_r25.md, section 3).  Every other site calls hvpr_wave_scan_incl.
#define HVPR_WAVE_SCAN_INCL2_SHFL(a, b, lane)                                             \
    do {                                                                                  \
        _Pragma("unroll") for (int o_ = 1; o_ < 64; o_ <<= 1) {                           \
            const unsigned ua_ = __shfl_up((a), o_, 64), ub_ = __shfl_up((b), o_, 64);    \
            if ((lane) >= o_) { (a) += ua_; (b) += ub_; }                                 \
        }                                                                                 \
    } while (0)

// The xor butterflies over the wave, in place: every lane ends with the result in v (an lvalue, evaluated more than once).
// Each is one statement (do { } while (0)): it needs its semicolon and is safe under an unbraced if / else.
// MACROS, not functions, on purpose: a force-inlined helper is simplified on its own before it is inlined (its shuffles share one
// lane id by then), and the kernels around it then schedule and allocate differently; the macro leaves every kernel the token
// stream it had (profiles/NOTES_r25.md, section 2).
//   HVPR_WAVE_SUM_XOR(v, ...)    32-to-1 sums of one to four ints, unsigneds, long longs, floats or doubles, all of them advancing
//                                step by step together.  For float and double THIS order of additions is what the tests pin:
//                                hvpr_reduce_sum adds the same pairs in another order and is no substitute.
//   HVPR_GROUP_SUM_XOR(v, width) one sum inside aligned groups of `width` lanes, a power of two up to 64 (may be a run-time value)
//   HVPR_WAVE_MAX_XOR(v)         maximum of an int
//   HVPR_WAVE_MAX_XOR_U64(v)     maximum of a 64-bit key, which travels as its two 32-bit halves
#define HVPR_SX1_(a) (a) += __shfl_xor((a), o_, 64);
#define HVPR_SX2_(a, b) HVPR_SX1_(a) HVPR_SX1_(b)
#define HVPR_SX3_(a, b, c) HVPR_SX2_(a, b) HVPR_SX1_(c)
#define HVPR_SX4_(a, b, c, d) HVPR_SX2_(a, b) HVPR_SX2_(c, d)
#define HVPR_SX_PICK_(a, b, c, d, n, ...) n
#define HVPR_WAVE_SUM_XOR(...)                                                                \
    do {                                                                                      \
        _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) {                               \
            HVPR_SX_PICK_(__VA_ARGS__, HVPR_SX4_, HVPR_SX3_, HVPR_SX2_, HVPR_SX1_)(__VA_ARGS__) \
        }                                                                                     \
    } while (0)
#define HVPR_GROUP_SUM_XOR(v, width) \
    do { for (int o_ = (width) >> 1; o_ > 0; o_ >>= 1) (v) += __shfl_xor((v), o_, 64); } while (0)
#define HVPR_WAVE_MAX_XOR(v) \
    do { _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) (v) = max((v), __shfl_xor((v), o_, 64)); } while (0)
#define HVPR_WAVE_MAX_XOR_U64(v)                                                              \
    do {                                                                                      \
        _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) {                               \
            const unsigned lo_ = __shfl_xor((unsigned)((v) & 0xffffffffull), o_, 64);         \
            const unsigned hi_ = __shfl_xor((unsigned)((v) >> 32), o_, 64);                   \
            const unsigned long long ob_ = ((unsigned long long)hi_ << 32) | lo_;             \
            (v) = ob_ > (v) ? ob_ : (v);                                                      \
        }                                                                                     \
    } while (0)

// the sum as a value, for the call sites that always took it from a function (conv_train.hip)
template <typename T>
__device__ __forceinline__ T hvpr_wave_sum_xor(T v) {
    HVPR_WAVE_SUM_XOR(v);
    return v;
}

#endif  // __HIPCC__
