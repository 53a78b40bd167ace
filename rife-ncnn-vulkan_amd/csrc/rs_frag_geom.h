// rs_frag_geom.h: where the operands of the consumer waves of conv_rs_kernel / conv_rs2_kernel (conv_rs.h, conv_rs2.h) live - the lane maps of
// v_mfma_f32_16x16x32_f16 over the LDS ring rows, conv_t64's weight image (pack_t64_image) and the fp32 staging rows.
// Plain integer functions without HIP types: the kernels and a host-only test program (tests/sanitize/rs_frag_geom_main.cpp, built by g++) include the same
// text; the device code takes every operand address from here.
//
// One matrix instruction is a 16 x 16 output tile over K = 32: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k][column l & 15], j = 0 .. 7 (16 bytes), and
// afterwards D[row 4 (l >> 4) + r][column l & 15], r = 0 .. 3.  Here: A = weights, row i of tile (N, half) = output channel 32 N + 16 half + i; B = pixels,
// column = pixel p0 + (l & 15) of the 32-pixel strip (p0 = 16 ph, + the tap's dx); K = the 32 input channels of a PAIR of 16-channel chunks: the lane's k group
// g = l >> 4 is chunk 2 cp + (g >> 1), 8-channel half g & 1.  A lane's four results are channels 4 g .. 4 g + 3 of its pixel: quad g of the 64-byte staging record.
#pragma once

#if defined(__HIPCC__)
#define RSG_HD __host__ __device__
#else
#define RSG_HD
#endif

namespace rsg {

constexpr int SEG = 34 * 32;                               // one (chunk, hi | lo) segment of a ring row: 34 pixels x 16 channels of f16, pixel-major, NO half swap
constexpr int ROWB = 8 * SEG;                              // ring row: [chunk 4][hi | lo] segments
constexpr int WCH = 9 * 2 * 64 * 16;                       // weight image, one K chunk: [tap 9][k half 2][64 rows][8 f16]
constexpr int IMG_W = 4 * WCH;                             // the weights of the image (bias and slope follow)
constexpr int STG_ROW = 8 * 1024;                          // staged output row: [chunk 4][32 px][16 fp32], quads XOR-swizzled by (px >> 1) & 3
constexpr int NUNIT = 38;                                  // units of a row: (chunk pair, tap | identity, pixel half), four (FAST: two, identity four) instructions each

// conv_t64.h's s16_row_channel (image row i of a 32-row block holds output channel row_channel(i)) and its inverse
RSG_HD constexpr int row_channel(int i) { return 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3); }
RSG_HD constexpr int channel_row(int ch) { return 8 * ((ch >> 2) & 3) + 4 * (ch >> 4) + (ch & 3); }

RSG_HD constexpr int lane_col(int l) { return l & 15; }    // pixel column / weight row of the tile
RSG_HD constexpr int lane_kg(int l) { return l >> 4; }     // k group: k = 8 kg .. 8 kg + 7
RSG_HD constexpr int kg_chunk(int kg) { return kg >> 1; }  // chunk within the pair
RSG_HD constexpr int kg_half(int kg) { return kg & 1; }    // 8-channel half of the chunk

// The fixed sequence of a row's units for output block N: per chunk pair the nine taps, pixel half 0 then 1, then - if the pair carries the input channels of
// block N - the identity step of the skip connection (centre tap) for both pixel halves.  Every tile therefore sums: pair 0 taps 0 - 8 (+ identity if N = 0),
// pair 1 taps 0 - 8 (+ identity if N = 1).
struct Unit { int cp, t, ph; bool idn; };
RSG_HD constexpr Unit unit(int N, int m) {
    for (int cp = 0; cp < 2; cp++) {
        const int cnt = 18 + (cp == N ? 2 : 0);
        if (m < cnt) return m < 18 ? Unit{cp, m >> 1, m & 1, false} : Unit{cp, 4, m & 1, true};
        m -= cnt;
    }
    return Unit{0, 0, 0, false};
}

// pixel fragment: byte offset in a ring row; lane part (tap column dx) + fragment part (chunk pair, plane hi 0 | lo 1, pixel half)
RSG_HD constexpr int pix_lane(int l, int dx) { return (lane_col(l) + dx) * 32 + kg_chunk(lane_kg(l)) * (2 * SEG) + kg_half(lane_kg(l)) * 16; }
RSG_HD constexpr int pix_frag(int cp, int plane, int ph) { return cp * (4 * SEG) + plane * SEG + ph * 512; }
RSG_HD constexpr int pix_offset(int l, int dx, int cp, int plane, int ph) { return pix_lane(l, dx) + pix_frag(cp, plane, ph); }

// weight fragment of tile (N, half): byte offset in the weight image; lane part + fragment part (chunk pair, tap)
RSG_HD constexpr int w_lane(int l, int N, int half) {
    return kg_chunk(lane_kg(l)) * WCH + kg_half(lane_kg(l)) * 1024 + (32 * N + channel_row(16 * half + lane_col(l))) * 16;
}
RSG_HD constexpr int w_frag(int cp, int t) { return 2 * cp * WCH + t * 2048; }
RSG_HD constexpr int w_offset(int l, int N, int cp, int t, int half) { return w_lane(l, N, half) + w_frag(cp, t); }

// identity fragment of channel half `half` (one K = 32 step over chunk pair N): element j of lane l is 1 where k = 8 kg + j is the tile row's own channel 16 half + i
RSG_HD constexpr bool id_one(int l, int half, int j) { return 8 * lane_kg(l) + j == 16 * half + lane_col(l); }

// staging: byte offset in a staged row of the lane's quad of tile (N, half, ph); lane part + tile part
RSG_HD constexpr int stg_lane(int l, int N) { return (2 * N * 32 + lane_col(l)) * 64 + ((lane_kg(l) ^ ((lane_col(l) >> 1) & 3)) << 4); }
RSG_HD constexpr int stg_tile(int half, int ph) { return half * 2048 + ph * 1024; }
RSG_HD constexpr int stg_offset(int l, int N, int half, int ph) { return stg_lane(l, N) + stg_tile(half, ph); }

static_assert((2 * SEG) % 256 == 128, "the second chunk of a pair sits in the other half of the LDS banks");
static_assert(unit(0, 18).idn && unit(0, 19).ph == 1 && unit(0, 20).cp == 1 && !unit(0, 37).idn && unit(1, 36).idn && unit(1, 37).idn, "unit order");
static_assert(channel_row(row_channel(13)) == 13 && row_channel(channel_row(29)) == 29, "inverse");

}  // namespace rsg
