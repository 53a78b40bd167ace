// flow_cascade_geom.h: tile geometry of k_flow_cascade (flow_cascade.h) - which coarse flow cells the pixels of one tile can touch.
// Plain integer functions without HIP types: the kernel, its launcher and a host-only test program (tests/sanitize/flow_cascade_geom_main.cpp, built by g++)
// include the same text.
#pragma once

#if defined(__HIPCC__)
#define FCG_HD __host__ __device__
#else
#define FCG_HD
#endif

namespace fcg {

// A workgroup of THREADS threads owns TILE_W x TILE_H full-resolution pixels: one wave per row of 64 pixels, TILE_H / 4 rows per wave.
constexpr int TILE_W = 64;
constexpr int TILE_H = 16;
constexpr int THREADS = 256;
constexpr int LEVELS = 3;                                  // level l holds flow_l, upsampled by scale(l) = 8, 4, 2 (rife-v4.6 blocks 0, 1, 2)

FCG_HD constexpr int scale(int l) { return 8 >> l; }
// LDS footprint of one level: a tile whose origin is a multiple of S touches at most T / S + 2 cells per axis (one before the first pixel's cell pair starts,
// one after the last pixel's): 10 x 4, 18 x 6, 34 x 10 records of 32 bytes
FCG_HD constexpr int pitch(int l) { return TILE_W / scale(l) + 2; }
FCG_HD constexpr int rows(int l) { return TILE_H / scale(l) + 2; }
FCG_HD constexpr int records(int l) { return pitch(l) * rows(l); }
FCG_HD constexpr int offset(int l) { return l == 0 ? 0 : offset(l - 1) + records(l - 1); }      // first record of level l
FCG_HD constexpr int lds_records(int levels) { return offset(levels); }                         // 148 for two levels, 488 for three
// a thread's share of staging level l: 16-byte halves of the level's records, one per thread and round: 1, 1, 3
FCG_HD constexpr int stage_loads(int l) { return (records(l) * 2 + THREADS - 1) / THREADS; }

// s0 of up_coeff(d, S, in, ...) (elementwise.h) in integers: floor((d + 0.5) / S - 0.5) = floor((2 d + 1 - S) / (2 S)), clamped to [0, in - 2].
// The numerator is above -2 S, so a negative one means -1 and is clamped to 0.  Monotonic in d.
FCG_HD constexpr int up_s0(int d, int S, int in) {
    const int num = 2 * d + 1 - S;
    int s = num < 0 ? 0 : num / (2 * S);
    if (s >= in - 1) s = in - 2;
    return s;
}

// Cells [lo, lo + n) of one axis of a flow with `full / S` cells that the pixels d0 .. min(d0 + tile, full) - 1 read: every pixel reads cells s0 and s0 + 1,
// and s0 is monotonic, so the range follows from the first and the last pixel.
struct Span { int lo, n; };
FCG_HD inline Span span(int d0, int tile, int full, int S) {
    const int in = full / S;
    const int d1 = (d0 + tile < full ? d0 + tile : full) - 1;
    Span r;
    r.lo = up_s0(d0, S, in);
    r.n = up_s0(d1, S, in) + 2 - r.lo;
    return r;
}

FCG_HD inline int tiles(int full, int tile) { return (full + tile - 1) / tile; }

// A thread owns one column of its wave's ROWS consecutive rows yw .. yw + ROWS - 1 (yw a multiple of ROWS) and forms the horizontal half of the interpolation
// once per cell row that these rows touch, not once per pixel.  up_s0 is monotonic, so per level the rows touch the cell rows group_first .. group_first +
// group_count - 1 of an axis of `full` pixels, and row yw + k has its upper cell row at group_first + group_rel and its lower one right after it.
// (The kernel itself uses group_first, group_rel_inner, group_rows and group_inner; group_rel and group_count define the last three, and the host check
// tests/sanitize/flow_cascade_rows_main.cpp holds them against up_coeff for every row group, the clamped ones included.)
constexpr int ROWS = TILE_H / (THREADS / 64);
FCG_HD constexpr int group_first(int yw, int l, int full) { return up_s0(yw, scale(l), full / scale(l)); }
FCG_HD constexpr int group_rel(int yw, int k, int l, int full) { return up_s0(yw + k, scale(l), full / scale(l)) - group_first(yw, l, full); }
FCG_HD constexpr int group_count(int yw, int l, int full) { return group_rel(yw, ROWS - 1, l, full) + 2; }
// Away from up_s0's two clamps (every row group but the first and the last of the image) the pattern is the same for every yw: 2, 3, 4 cell rows with the
// rows' upper cell rows at {0, 0, 0, 0}, {0, 0, 1, 1}, {0, 1, 1, 2}.  A clamp only shortens it, so group_rows is also the most cell rows a group touches.
constexpr int INNER_YW = 64, INNER_FULL = 4096;
FCG_HD constexpr int group_rel_inner(int k, int l) { return group_rel(INNER_YW, k, l, INNER_FULL); }
FCG_HD constexpr int group_rows(int l) { return group_count(INNER_YW, l, INNER_FULL); }
FCG_HD constexpr bool group_inner(int yw, int l, int full) {
    bool same = true;
    for (int k = 0; k < ROWS; k++) same = same && group_rel(yw, k, l, full) == group_rel_inner(k, l);
    return same;
}
FCG_HD constexpr bool group_inner(int yw, int full) { return group_inner(yw, 0, full) && group_inner(yw, 1, full) && group_inner(yw, 2, full); }
static_assert(ROWS == 4 && group_rows(0) == 2 && group_rows(1) == 3 && group_rows(2) == 4, "cell rows of a row group per level");
static_assert(group_rel_inner(3, 0) == 0 && group_rel(INNER_YW + ROWS, 3, 0, INNER_FULL) == 0, "level 0: one cell row pair per group, at either phase of yw");
static_assert(group_rel_inner(1, 1) == 0 && group_rel_inner(2, 1) == 1 && group_rel_inner(1, 2) == 1 && group_rel_inner(2, 2) == 1 && group_rel_inner(3, 2) == 2, "");

}  // namespace fcg
