// Host check of the host-compilable part of hvpr_amd/csrc/wave.h: the ordered float keys (with the score top-k's wrapper, whose
// lines tests/test_wave_host.py cuts out of csrc/postprocess.hip into topk_ord.inc) and the frame of a row.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <dir of topk_ord.inc> tools/check_wave_host.cpp
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hvpr_amd/csrc/wave.h"
#include "topk_ord.inc"

static int fails = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++fails <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                   \
    } while (0)

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// a and b are not NaN.  The bare map orders by (value, then -0 before +0); the wrapper orders by value alone.
static void check_pair(float a, float b) {
    const unsigned ka = hvpr_ord_of(a), kb = hvpr_ord_of(b);
    if (a < b) CHECK(ka < kb, "%a %a", a, b);
    if (a > b) CHECK(ka > kb, "%a %a", a, b);
    if (a == b) CHECK((ka == kb) == (bits_of(a) == bits_of(b)), "%a %a", a, b);     // only the two zeros are equal with other bits
    CHECK((topk_ord(a) < topk_ord(b)) == (a < b) && (topk_ord(a) == topk_ord(b)) == (a == b), "wrapper %a %a", a, b);
}

static long long check_keys() {
    const float denorm = from_bits(1u), inf = INFINITY;
    std::vector<float> v = {0.f, -0.f, denorm, -denorm, FLT_MIN, -FLT_MIN, 1.f, -1.f, FLT_MAX, -FLT_MAX, inf, -inf};
    uint32_t s = 0x9e3779b9u;
    while (v.size() < 12 + 4000) {
        s ^= s << 13; s ^= s >> 17; s ^= s << 5;            // xorshift32: every bit pattern but 0 in its cycle
        const float f = from_bits(s);
        if (f == f) v.push_back(f);
    }
    for (const float f : v) {
        CHECK(bits_of(hvpr_of_ord(hvpr_ord_of(f))) == bits_of(f), "inverse %a", f);
        CHECK(hvpr_ord_of(f) > 0u, "key 0 below %a", f);
    }
    long long pairs = 0;
    for (size_t i = 0; i < v.size(); ++i)
        for (size_t j = 0; j < v.size(); j += (i < 12 || j < 12) ? 1 : 7) { check_pair(v[i], v[j]); ++pairs; }
    CHECK(hvpr_ord_of(-0.f) != hvpr_ord_of(0.f) && hvpr_ord_of(-0.f) + 1u == hvpr_ord_of(0.f), "the bare map keeps the zeros apart");
    CHECK(topk_ord(-0.f) == topk_ord(0.f) && topk_ord(0.f) == hvpr_ord_of(0.f), "the top-k wrapper merges them");
    CHECK(hvpr_ord_of(-inf) == 0x007fffffu && hvpr_ord_of(inf) == 0xff800000u, "ends");
    return pairs;
}

// the first and the last row of every non-empty frame map to it, whatever empty frames lie around it
static long long check_frames() {
    const std::vector<std::vector<int32_t>> sets = {
        {0, 5},                                // one frame
        {0, 0, 0, 3, 3, 3, 9, 10, 10, 10},     // empty at the front, in the middle, at the end
        {7, 7, 8, 8, 8, 20, 20},               // a non-zero base, single-row frame
        {0, 1, 2, 3, 4, 5, 6, 7, 8},           // one row each
        {0, 0, 0, 0, 4},                       // only the last frame has rows
        {0, 4, 4, 4, 4},                       // only the first
    };
    long long rows = 0;
    for (const auto &off : sets) {
        const int B = (int)off.size() - 1;
        for (int b = 0; b < B; ++b) {
            if (off[b] == off[b + 1]) continue;
            for (const int row : {off[b], off[b + 1] - 1}) {
                const int f = hvpr_frame_of(off.data(), B, row);
                CHECK(f == b, "B %d row %d: frame %d, expected %d", B, row, f, b);
                ++rows;
            }
        }
        for (int row = off[0]; row < off[B]; ++row) {      // and every row in between lands in a frame that holds it
            const int f = hvpr_frame_of(off.data(), B, row);
            CHECK(f >= 0 && f < B && off[f] <= row && row < off[f + 1], "B %d row %d: frame %d", B, row, f);
        }
    }
    return rows;
}

int main() {
    const long long pairs = check_keys(), rows = check_frames();
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok: %lld key pairs, %lld frame rows\n", pairs, rows);
    return 0;
}
