// The persistent, XCD-aware walk every eval convolution kernel runs (conv_igemm.hip, conv_bf3.hip, conv_wino.hip) and the direct
// kernel's walk table, in plain integer arithmetic so that a host program can check them (tools/check_wino_walk.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HVPR_WALK_HD __host__ __device__ __forceinline__
#else
#define HVPR_WALK_HD inline
#endif

// Step `it` of the persistent walk over round_up(items, 8) * n_ct steps -> channel tile `ct` and item (may be >= items: a hole of
// the last round).  Consecutive workgroup ids land on consecutive XCDs (8 of them, each with its own L2), so eight consecutive steps
// are the eight XCDs': they take eight neighbouring items of the same channel tile, and an XCD's next step is the next channel tile
// of the same item — the n_ct channel tiles of one item run at the same time behind one L2 and its input patch comes from HBM once.
HVPR_WALK_HD int conv_walk_step(int it, int n_ct, int &ct) {
    const int xcd = it & 7, j = it >> 3;
    ct = j % n_ct;
    return (j / n_ct) * 8 + xcd;
}

// The direct kernel's items are the tiles of N images, row-major.  Its walk as a TABLE, one 8-byte entry per step, built once per
// shape so that a workgroup reads its item instead of dividing for it:
//     lo = tx [0..15] | ty [16..30] | hole [31]      hi = ct [0..11] | n [12..31]      entry = lo | hi << 32
// A hole is a step of the last round that has no item.  (k_conv unpacks with the shifts written out: conv_igemm.hip.)
typedef unsigned long long ConvTabEntry;
enum { CONV_TAB_MAX_TX = 1 << 16, CONV_TAB_MAX_TY = 1 << 15, CONV_TAB_MAX_CT = 1 << 12, CONV_TAB_MAX_N = 1 << 20 };

HVPR_WALK_HD ConvTabEntry conv_tab_entry(int N, int tiles_x, int tiles_y, int n_ct, int it) {
    int ct;
    int pt = conv_walk_step(it, n_ct, ct);
    if (pt >= tiles_x * tiles_y * N) return 1ull << 31;
    const int tx = pt % tiles_x; pt /= tiles_x;
    const int ty = pt % tiles_y, n = pt / tiles_y;
    return (ConvTabEntry)((unsigned)tx | (unsigned)ty << 16) | (ConvTabEntry)((unsigned)ct | (unsigned)n << 12) << 32;
}
