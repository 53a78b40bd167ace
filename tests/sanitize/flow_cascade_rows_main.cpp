// TEST INFRASTRUCTURE ONLY.  A program of its own (tests/test_flow_cascade_rows.py builds it plain and with ASan + UBSan; csrc/Makefile, target
// ../flow-cascade-rows-asan): the row-group functions of csrc/flow_cascade_geom.h, by which a thread of k_flow_cascade shares the horizontal half of the
// interpolation between its ROWS pixels.  Over every padded height 32 .. 4096 (step 32), every level and every wave row group yw:
//   * group_first, group_rel and group_count are up_coeff's cell rows (csrc/elementwise.h, restated here in its float form) for each of the four rows, and the
//     rows they name lie inside the span fcg::span stages for the tile;
//   * for a group that fcg::group_inner accepts, the kernel's scheme is restated on one column of cell values (cascade_sample_rows of csrc/flow_cascade.h: the
//     cell rows first + j for j < group_rows, then per pixel row the constant pair group_rel_inner): each row must come out with the cell rows and the b0, b1 of
//     up_coeff - compared as indices and as the value v[s0] * b0 + v[s0 + 1] * b1 over distinct v.  The cell rows are read from a heap array that holds exactly
//     the rows staged for the tile, so a touched row outside the staged span is a heap overflow the sanitizer sees;
//   * every row group but the image's first and last is an inner one (the other two take the kernel's pixel-by-pixel path, which
//     flow_cascade_geom_main.cpp covers).
// Exit status 0 and a last line "flow_cascade_rows: N checks, 0 mismatches".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/flow_cascade_geom.h"

// csrc/elementwise.h up_coeff
static void up_coeff(int d, int S, int in, int& s0, float& a0, float& a1) {
    float f = ((float)d + 0.5f) * (1.0f / (float)S) - 0.5f;
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= in - 1) { s = in - 2; f = 1.f; }
    s0 = s; a0 = 1.f - f; a1 = f;
}

static long long g_checks = 0, g_wrong = 0;
static void want(bool cond, const char* what, int hp, int l, int y) {
    g_checks++;
    if (!cond && g_wrong++ < 20) std::printf("MISMATCH %s (height %d, level %d, row %d)\n", what, hp, l, y);
}

// the value of cell row c: distinct, and no two pairs (c, c + 1) blend to the same number with the same weights
static float cell_value(int c) { return 3.0f + 1.25f * (float)c + 0.001f * (float)(c * c % 97); }

template <int L>
static int sweep_level(int hp) {
    constexpr int S = fcg::scale(L), NR = fcg::group_rows(L);
    const int in = hp / S;
    int inner_groups = 0;
    for (int y0 = 0; y0 < hp; y0 += fcg::TILE_H) {
        const fcg::Span sy = fcg::span(y0, fcg::TILE_H, hp, S);
        std::vector<float> staged((size_t)sy.n);                                  // the tile's LDS rows of this level, one column
        for (int i = 0; i < sy.n; i++) staged[(size_t)i] = cell_value(sy.lo + i);
        for (int yw = y0; yw < y0 + fcg::TILE_H && yw < hp; yw += fcg::ROWS) {
            const bool inner = fcg::group_inner(yw, hp);
            inner_groups += inner;
            const int first = fcg::group_first(yw, L, hp), count = fcg::group_count(yw, L, hp);
            want(count >= 2 && count <= NR, "a row group touches more cell rows than the kernel keeps", hp, L, yw);
            want(first >= sy.lo && first + count <= sy.lo + sy.n, "a row group's cell rows leave the staged span", hp, L, yw);
            if (count < 2 || count > NR || first < sy.lo) continue;
            for (int k = 0; k < fcg::ROWS; k++) {
                int s0; float b0, b1;
                up_coeff(yw + k, S, in, s0, b0, b1);
                want(first + fcg::group_rel(yw, k, L, hp) == s0, "group_rel is not up_coeff's cell row", hp, L, yw + k);
            }
            if (!inner) continue;
            want(count == NR, "an inner group is shorter than the inner pattern", hp, L, yw);
            std::vector<float> h((size_t)NR);
            for (int j = 0; j < NR; j++) h[(size_t)j] = staged.at((size_t)(first + j - sy.lo));      // the horizontal stage (a0 = 1, a1 = 0 here): one read per cell row
            for (int k = 0; k < fcg::ROWS; k++) {
                const int y = yw + k, r = fcg::group_rel_inner(k, L);
                int s0; float b0, b1;
                up_coeff(y, S, in, s0, b0, b1);
                want(r >= 0 && r + 1 < NR, "the constant pair is outside the kept cell rows", hp, L, y);
                if (r < 0 || r + 1 >= NR) continue;
                want(first + r == s0, "the constant cell rows are not up_coeff's", hp, L, y);
                const float got = h[(size_t)r] * b0 + h[(size_t)r + 1] * b1;
                const float ref = cell_value(s0) * b0 + cell_value(s0 + 1) * b1;
                want(std::memcmp(&got, &ref, 4) == 0, "the blended value differs", hp, L, y);
            }
        }
    }
    return inner_groups;
}

int main() {
    static_assert(fcg::TILE_H % fcg::ROWS == 0 && fcg::LEVELS == 3, "row groups tile the tile; three levels");
    for (int hp = 32; hp <= 4096; hp += 32) {
        const int g0 = sweep_level<0>(hp), g1 = sweep_level<1>(hp), g2 = sweep_level<2>(hp);
        // every row group but the image's first and last takes the constant pattern
        want(g0 == hp / fcg::ROWS - 2 && g1 == g0 && g2 == g0, "inner row groups: all but the first and the last", hp, -1, 0);
    }
    std::printf("flow_cascade_rows: %lld checks, %lld mismatches\n", g_checks, g_wrong);
    return g_wrong ? 1 : 0;
}
