// The persistent walk of conv_wino.hip over 8 x 16 pixel tiles with PAIRED RAGGED EDGE TILES, in plain integer arithmetic so that a
// host program can check it (tools/check_wino_walk.cpp).
//
// A tile is 4 x 8 blocks of 2 x 2 output pixels.  An image whose width leaves the last tile column at most 4 live block columns
// (right pairing) has the right-edge tiles of tile rows 2r and 2r + 1 computed by ONE workgroup item: the two 10-column halves of
// their patches lie side by side in the 20 column slots of one LDS patch row.  An image whose height leaves the last tile row at
// most 2 live block rows (bottom pairing) has the bottom-edge tiles of tile columns 2c and 2c + 1 computed by one item: their two
// 6-row halves fill 12 patch rows.  The corner tile belongs to the right pairing; an odd count leaves one tile unpaired.
//
// Items of one image, in walk order:   [hi x wi plain tiles, row-major] [right column: ceil(tiles_y / 2)] [bottom row: ceil(wi / 2)]
// with wi = tiles_x - 1 under right pairing (else tiles_x) and hi = tiles_y - 1 under bottom pairing (else tiles_y).
#pragma once

#include "conv_walk.h"      // HVPR_WALK_HD, conv_walk_step: step -> (channel tile, item)

enum { WINO_SINGLE = 0, WINO_PAIR_RIGHT = 1, WINO_PAIR_BOTTOM = 2 };

struct WinoWalk {
    int tiles_x, tiles_y;   // 16-px tile columns, 8-px tile rows of the image
    int wi, hi;             // extent of the plain (never paired) tile rectangle
    int n_plain, n_right;   // items of the plain rectangle / of the right column
    int per_image;          // items of one image
};

struct WinoItem {
    int n;                  // image
    int mode;               // WINO_SINGLE: tile (ty, tx).  WINO_PAIR_RIGHT: (ty, tx) and (ty + 1, tx).  WINO_PAIR_BOTTOM: (ty, tx) and (ty, tx + 1)
    int ty, tx;
};

// pairing != 0 (tile_h == 8 only): pair where the shape allows it; 0: one item per tile of tile_h x 16 px, row-major (the
// statistics, px_groups 2 and 4 variants)
HVPR_WALK_HD WinoWalk wino_walk_make(int H, int W, int tile_h, int pairing) {
    WinoWalk w;
    w.tiles_x = (W + 15) / 16;
    w.tiles_y = (H + tile_h - 1) / tile_h;
    const int live_bcols = (W - 16 * (w.tiles_x - 1) + 1) / 2;      // live block columns of the last tile column: 1..8
    const int live_brows = (H - tile_h * (w.tiles_y - 1) + 1) / 2;  // live block rows of the last tile row: 1..4 (tile_h 8)
    const int rp = pairing && tile_h == 8 && live_bcols <= 4, bp = pairing && tile_h == 8 && live_brows <= 2;
    w.wi = rp ? w.tiles_x - 1 : w.tiles_x;
    w.hi = bp ? w.tiles_y - 1 : w.tiles_y;
    w.n_plain = w.wi * w.hi;
    w.n_right = rp ? (w.tiles_y + 1) / 2 : 0;
    w.per_image = w.n_plain + w.n_right + (bp ? (w.wi + 1) / 2 : 0);
    return w;
}

// item `pt` of 0 .. N * per_image - 1
HVPR_WALK_HD WinoItem wino_walk_item(const WinoWalk &w, int pt) {
    WinoItem it;
    it.n = pt / w.per_image;
    int q = pt - it.n * w.per_image;
    if (q < w.n_plain) {
        it.ty = q / w.wi; it.tx = q - it.ty * w.wi; it.mode = WINO_SINGLE;
    } else if ((q -= w.n_plain) < w.n_right) {
        it.ty = 2 * q; it.tx = w.tiles_x - 1;
        it.mode = it.ty + 1 < w.tiles_y ? WINO_PAIR_RIGHT : WINO_SINGLE;
    } else {
        q -= w.n_right;
        it.ty = w.tiles_y - 1; it.tx = 2 * q;
        it.mode = it.tx + 1 < w.wi ? WINO_PAIR_BOTTOM : WINO_SINGLE;
    }
    return it;
}

// The walk as a TABLE, one 8-byte entry per step, built once per (N, H, W, cout) so that a workgroup reads its item instead of
// dividing for it:   lo = tx [0..11] | ty [12..23] | mode [24..25] | hole [31]      hi = ct [0..11] | n [12..31]
// A hole is a step of the last round that has no item.
struct WinoTabEntry {
    unsigned lo, hi;
};
enum { WINO_TAB_MAX_TILES = 4096, WINO_TAB_MAX_CT = 4096, WINO_TAB_MAX_N = 1 << 20 };

HVPR_WALK_HD int wino_walk_steps(const WinoWalk &w, int N, int n_ct) { return (N * w.per_image + 7) / 8 * 8 * n_ct; }

HVPR_WALK_HD WinoTabEntry wino_tab_entry(const WinoWalk &w, int N, int n_ct, int it) {
    WinoTabEntry e;
    int ct;
    const int pt = conv_walk_step(it, n_ct, ct);
    if (pt >= N * w.per_image) {
        e.lo = 1u << 31; e.hi = 0u;
        return e;
    }
    const WinoItem i = wino_walk_item(w, pt);
    e.lo = (unsigned)i.tx | (unsigned)i.ty << 12 | (unsigned)i.mode << 24;
    e.hi = (unsigned)ct | (unsigned)i.n << 12;
    return e;
}
HVPR_WALK_HD bool wino_tab_hole(WinoTabEntry e) { return (e.lo >> 31) != 0u; }
HVPR_WALK_HD int wino_tab_tx(WinoTabEntry e) { return (int)(e.lo & 4095u); }
HVPR_WALK_HD int wino_tab_ty(WinoTabEntry e) { return (int)(e.lo >> 12 & 4095u); }
HVPR_WALK_HD int wino_tab_mode(WinoTabEntry e) { return (int)(e.lo >> 24 & 3u); }
HVPR_WALK_HD int wino_tab_ct(WinoTabEntry e) { return (int)(e.hi & 4095u); }
HVPR_WALK_HD int wino_tab_n(WinoTabEntry e) { return (int)(e.hi >> 12); }
