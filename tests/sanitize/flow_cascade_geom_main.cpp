// TEST INFRASTRUCTURE ONLY.  A program of its own (tests/test_flow_cascade_geom.py builds it plain and with ASan + UBSan; csrc/Makefile, target
// ../flow-cascade-geom-asan): csrc/flow_cascade_geom.h, the tile geometry of k_flow_cascade, over every padded frame size 32 .. 4096 (step 32) per axis, every
// scale 8 / 4 / 2 and every tile origin.  up_coeff of csrc/elementwise.h is restated here in its float form; for every pixel of every tile its cell pair
// (s0, s0 + 1) must lie inside the range the tile stages, the range inside the flow's cells, and the range inside the LDS rows the kernel allocates.  The
// staged cells are touched in a heap array of exactly `in` cells and the pixel's pair in one of exactly pitch / rows cells, so that an index outside either is
// a heap overflow the sanitizer sees.  Then every (wp, hp) pair: the records of a tile against the kernel's LDS allocation.
// Exit status 0 and a last line "flow_cascade_geom: N checks, 0 wrong".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/flow_cascade_geom.h"

// csrc/elementwise.h up_coeff, the index only
static int up_coeff_s0(int d, int S, int in) {
    float f = ((float)d + 0.5f) * (1.0f / (float)S) - 0.5f;
    int s = (int)floorf(f);
    if (s < 0) s = 0;
    if (s >= in - 1) s = in - 2;
    return s;
}

static long long g_checks = 0, g_wrong = 0;
static void want(bool cond, const char* what, int full, int S, int d) {
    g_checks++;
    if (!cond && g_wrong++ < 20) std::printf("WRONG %s (axis of %d pixels, scale %d, at %d)\n", what, full, S, d);
}

// one axis: tiles of `tile` pixels over `full` pixels, level l; returns the largest staged count
static int sweep_axis(int full, int tile, int l, int lds_cells) {
    const int S = fcg::scale(l), in = full / S;
    int most = 0;
    std::vector<unsigned char> cells((size_t)in, 0);              // the flow's cells along this axis
    for (int t = 0; t < fcg::tiles(full, tile); t++) {
        const int d0 = t * tile;
        const fcg::Span sp = fcg::span(d0, tile, full, S);
        want(sp.lo >= 0 && sp.n >= 2 && sp.lo + sp.n - 1 <= in - 1, "the staged range leaves [0, in - 1]", full, S, d0);
        want(sp.n <= lds_cells, "the staged range is longer than its LDS row", full, S, d0);
        if (sp.lo < 0 || sp.n < 2 || sp.lo + sp.n > in || sp.n > lds_cells) continue;
        for (int i = 0; i < sp.n; i++) cells[(size_t)sp.lo + i]++;                       // the staging loads
        std::vector<unsigned char> lds((size_t)lds_cells, 0);
        for (int d = d0; d < d0 + tile && d < full; d++) {
            const int s0 = up_coeff_s0(d, S, in);
            want(s0 == fcg::up_s0(d, S, in), "up_s0 is not up_coeff's index", full, S, d);
            const bool inside = s0 >= sp.lo && s0 + 1 <= sp.lo + sp.n - 1;
            want(inside, "a pixel's cell pair lies outside the staged range", full, S, d);
            if (inside) { lds[(size_t)(s0 - sp.lo)]++; lds[(size_t)(s0 + 1 - sp.lo)]++; }      // the LDS reads
        }
        if (sp.n > most) most = sp.n;
    }
    want(fcg::tiles(full, tile) * tile >= full && (fcg::tiles(full, tile) - 1) * tile < full, "the tiles do not cover the axis once", full, S, 0);
    return most;
}

int main() {
    static_assert(fcg::THREADS % 64 == 0 && fcg::TILE_W == 64 && fcg::TILE_H % (fcg::THREADS / 64) == 0, "one wave per row of 64 pixels");
    static_assert(fcg::lds_records(2) == fcg::records(0) + fcg::records(1) && fcg::lds_records(3) == fcg::lds_records(2) + fcg::records(2), "levels are laid end to end");
    static_assert(fcg::lds_records(3) * 32 <= 64 * 1024, "static LDS of one workgroup");
    const int N = 4096 / 32;
    std::vector<int> nx((size_t)(N + 1) * fcg::LEVELS, 0), ny((size_t)(N + 1) * fcg::LEVELS, 0);
    for (int k = 1; k <= N; k++)
        for (int l = 0; l < fcg::LEVELS; l++) {
            nx[(size_t)k * fcg::LEVELS + l] = sweep_axis(32 * k, fcg::TILE_W, l, fcg::pitch(l));
            ny[(size_t)k * fcg::LEVELS + l] = sweep_axis(32 * k, fcg::TILE_H, l, fcg::rows(l));
        }
    // every frame: the most records any tile stages, per level inside the level's block and in all inside the kernel's allocation
    for (int kx = 1; kx <= N; kx++)
        for (int ky = 1; ky <= N; ky++) {
            int total = 0;
            for (int l = 0; l < fcg::LEVELS; l++) {
                const int r = nx[(size_t)kx * fcg::LEVELS + l] * ny[(size_t)ky * fcg::LEVELS + l];
                want(r <= fcg::records(l), "a level's records exceed its LDS block", 32 * kx, fcg::scale(l), 32 * ky);
                total += r;
                if (l == 1) want(total <= fcg::lds_records(2), "two levels exceed the LDS allocation", 32 * kx, fcg::scale(l), 32 * ky);
            }
            want(total <= fcg::lds_records(3), "three levels exceed the LDS allocation", 32 * kx, 0, 32 * ky);
        }
    std::printf("flow_cascade_geom: %lld checks, %lld wrong\n", g_checks, g_wrong);
    return g_wrong ? 1 : 0;
}
