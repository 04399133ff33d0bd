// Host check of hvpr_amd/csrc/wino_walk.h, the tile walk of the Winograd convolution with paired ragged edge tiles: replays the
// kernel's persistent walk on the CPU and verifies that every (image, tile, channel tile) is produced exactly once, that only
// tiles that fit side by side are paired, and that a pair stays inside one image — for all H, W in 1..80, N in 1..3.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_wino_walk.cpp -o check_wino_walk && ./check_wino_walk
#include <cstdio>
#include <vector>

#include "../hvpr_amd/csrc/wino_walk.h"

static int fails = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++fails <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                   \
    } while (0)

static long long replay(int N, int H, int W, int tile_h, int pairing, int n_ct) {
    const WinoWalk w = wino_walk_make(H, W, tile_h, pairing);
    const int TX = (W + 15) / 16, TY = (H + tile_h - 1) / tile_h;
    CHECK(w.tiles_x == TX && w.tiles_y == TY, "grid H %d W %d", H, W);
    const int live_bcols = (W - 16 * (TX - 1) + 1) / 2, live_brows = (H - tile_h * (TY - 1) + 1) / 2;
    std::vector<int> seen((size_t)N * TY * TX * n_ct, 0);
    auto mark = [&](int n, int ty, int tx, int ct) {
        CHECK(n >= 0 && n < N && ty >= 0 && ty < TY && tx >= 0 && tx < TX && ct >= 0 && ct < n_ct, "range H %d W %d: n %d ty %d tx %d ct %d", H, W, n, ty, tx, ct);
        if (n >= 0 && n < N && ty >= 0 && ty < TY && tx >= 0 && tx < TX && ct >= 0 && ct < n_ct) ++seen[(((size_t)n * TY + ty) * TX + tx) * n_ct + ct];
    };
    const int n_pt = w.per_image * N;
    const int total_walk = (n_pt + 7) / 8 * 8 * n_ct;
    long long items = 0;
    for (int it = 0; it < total_walk; ++it) {
        int ct;
        const int pt = conv_walk_step(it, n_ct, ct);
        if (pt >= n_pt) continue;
        ++items;
        const WinoItem m = wino_walk_item(w, pt);
        mark(m.n, m.ty, m.tx, ct);
        if (!pairing) {                       // the unpaired variants keep their row-major tile order
            CHECK(m.mode == WINO_SINGLE && (m.n * TY + m.ty) * TX + m.tx == pt, "row-major H %d W %d pt %d", H, W, pt);
        }
        if (m.mode == WINO_PAIR_RIGHT) {
            CHECK(pairing && live_bcols <= 4 && m.tx == TX - 1 && m.ty % 2 == 0 && m.ty + 1 < TY, "right pair H %d W %d ty %d tx %d", H, W, m.ty, m.tx);
            mark(m.n, m.ty + 1, m.tx, ct);
        } else if (m.mode == WINO_PAIR_BOTTOM) {
            // both tiles in the bottom row, and neither is the column the right pairing consumes
            CHECK(pairing && live_brows <= 2 && m.ty == TY - 1 && m.tx % 2 == 0 && m.tx + 1 < (live_bcols <= 4 ? TX - 1 : TX), "bottom pair H %d W %d ty %d tx %d", H, W, m.ty, m.tx);
            mark(m.n, m.ty, m.tx + 1, ct);
        } else {
            CHECK(m.mode == WINO_SINGLE, "mode %d", m.mode);
        }
    }
    for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "H %d W %d N %d n_ct %d pairing %d: tile slot %zu produced %d times", H, W, N, n_ct, pairing, i, seen[i]);
    CHECK(items == (long long)n_pt * n_ct, "item count H %d W %d", H, W);
    // pairing saves exactly the pairs: floor(TY / 2) on the right, floor(wi / 2) at the bottom
    if (pairing && tile_h == 8) {
        const int rp = live_bcols <= 4, bp = live_brows <= 2, wi = rp ? TX - 1 : TX;
        CHECK(w.per_image == TX * TY - (rp ? TY / 2 : 0) - (bp ? wi / 2 : 0), "closed form H %d W %d: %d", H, W, w.per_image);
    } else {
        CHECK(w.per_image == TX * TY, "plain count H %d W %d", H, W);
    }
    return items;
}

int main() {
    long long cases = 0;
    for (int H = 1; H <= 80; ++H)
        for (int W = 1; W <= 80; ++W)
            for (int N = 1; N <= 3; ++N)
                for (int n_ct = 1; n_ct <= 3; ++n_ct) {
                    replay(N, H, W, 8, 1, n_ct);
                    replay(N, H, W, 8, 0, n_ct);
                    replay(N, H, W, 16, 0, n_ct);
                    cases += 3;
                }
    // the three levels of the hvpr_car backbone
    CHECK(replay(1, 248, 296, 8, 1, 2) == 574 * 2, "level 0");
    CHECK(replay(1, 124, 148, 8, 1, 4) == 148 * 4, "level 1");
    CHECK(replay(1, 62, 74, 8, 1, 8) == 40 * 8, "level 2");
    std::printf("%s: %lld walks replayed, %d failures\n", fails ? "FAILED" : "ok", cases + 3, fails);
    return fails ? 1 : 0;
}
