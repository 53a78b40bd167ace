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

// s0 of up_coeff(d, S, in, ...) (elementwise.h) in integers: floor((d + 0.5) / S - 0.5) = floor((2 d + 1 - S) / (2 S)), clamped to [0, in - 2].
// The numerator is above -2 S, so a negative one means -1 and is clamped to 0.  Monotonic in d.
FCG_HD inline int up_s0(int d, int S, int in) {
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

}  // namespace fcg
