// What the eval convolution kernels share (conv_igemm.hip k_conv, conv_wino.hip k_wino, conv_bf3.hip k_conv3): LDS-DMA staging,
// the scalar load of a walk-table entry and the sizing of the persistent grid (the timing build's HVPR_IF_TIMING: wave.h).
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int KC = 8;   // input channels per K chunk

// One LDS-DMA piece: 16 B per lane, global (per-lane address) -> LDS (M0 = wave-uniform base, + lane * 16).
// Issued through inline asm on purpose: hipcc would otherwise put s_waitcnt vmcnt(0) in front of the next ds_read (it
// must assume the DMA write aliases it), which serialises the stream behind the multiply.  The wait is placed by hand
// in front of the per-chunk barrier instead (cdna_hip_programming.md §5.7 recipe).
// Address form: SGPR base + 32-bit VGPR byte offset.  Everything that changes from chunk to chunk lives in the SGPR base
// and in M0, so the steady-state loop issues NO vector-ALU instruction: measured on this chip, v_mfma_f32_32x32x2_f32
// runs on the f32 vector lanes (it is rated at the vector FMA rate), and a co-resident wave that needs VALU slots for
// address arithmetic is starved for as long as its neighbour multiplies.
__device__ __forceinline__ void lds_dma16(const void *sbase_uniform, unsigned voff_bytes, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff_bytes), "s"(sbase_uniform), "s"(lds_dst_uniform)
                 : "memory");
}

__device__ __forceinline__ unsigned lds_addr_of(const void *p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void *)p;
}

// word `step` of a walk table (8-byte entries) through the constant address space: the address is uniform, so this is one scalar
// 8-byte load.  The second form: an entry type of two 32-bit words lo, hi (WinoTabEntry).
__device__ __forceinline__ unsigned long long tab_load(const unsigned long long *tab, int step) {
    return *((const __attribute__((address_space(4))) unsigned long long *)(size_t)tab + step);
}
template <class Entry>
__device__ __forceinline__ Entry tab_load(const Entry *tab, int step) {
    static_assert(sizeof(Entry) == 8, "a walk-table entry is 8 bytes");
    const unsigned long long w = tab_load((const unsigned long long *)tab, step);
    Entry e;
    e.lo = (unsigned)w; e.hi = (unsigned)(w >> 32);
    return e;
}

// Workgroups of a persistent walk of KERNEL (threads, dynamic LDS bytes) over `tiles` items: the workgroups of this instantiation
// that fit the chip at once (found once per process), or the items rounded up when they are fewer — a multiple of 8 either way:
// workgroup id % 8 = its XCD.  The dynamic-LDS limit is raised on the current device first.  -1: that failed.
template <auto KERNEL>
int conv_walk_blocks(int threads, int lds_bytes, long long tiles) {
    static unsigned long long lds_set = 0ull;
    if (lds_bytes > 0 && hvpr_ensure_dyn_lds((const void *)KERNEL, lds_bytes, &lds_set) != 0) return -1;
    static int resident = 0;
    if (resident == 0) {
        int per_cu = 0, dev = 0, cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, threads, lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
        resident = per_cu * cus;
    }
    long long blocks = tiles < resident ? (tiles + 7) / 8 * 8 : resident;
    if (blocks > resident && resident >= 8) blocks = resident / 8 * 8;
    return (int)blocks;
}

}  // namespace
