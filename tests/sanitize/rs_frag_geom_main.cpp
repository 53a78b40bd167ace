// TEST INFRASTRUCTURE ONLY.  A program of its own (tests/test_rs_frag_geom.py builds it plain and with ASan + UBSan; csrc/Makefile, target
// ../rs-frag-geom-asan): csrc/rs_frag_geom.h, the operand lane maps of the conv_rs / conv_rs2 consumer waves (v_mfma_f32_16x16x32_f16), over every lane, tap,
// chunk pair, plane, pixel half, channel half and output block N.  The ring row, the weight image and the staged row are heap arrays of exactly their sizes and
// every 16-byte operand access is made on them, so that an offset outside is a heap overflow the sanitizer sees.
//   (i)   every pixel fragment inside its (chunk, plane) segment of the ring row, every weight fragment inside the weights of the image
//   (ii)  the fragments of a (tap, chunk pair, plane) hold every (pixel, channel of the pair) exactly once, the weight fragments every (output channel, input
//         channel of the pair) exactly once, at the bytes the ring image / pack_t64_image put them, with the SAME k in element j of lane l on both sides
//   (iii) through row_channel the weight rows of tile (N, half) are the channels 32 N + 16 half + 0 .. 15 in order
//   (iv)  the 16 lanes of every ds_read_b128 lane group read 16 distinct 16-byte slots mod 256
//   (v)   the 8 lanes of every ds_write_b128 group of the staging writes hit 8 distinct slots mod 128; the staged row is covered once, each quad where the
//         epilogue waves read it
//   (vi)  the identity fragment has exactly one 1 per tile row, at k = 16 half + i
//   and the unit sequence: 38 units, 152 instructions, every (chunk pair, tap, pixel half) once, the identity step after the taps of pair N.
// Exit status 0 and a last line "rs_frag_geom: N checks, 0 wrong".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/rs_frag_geom.h"

static long long g_checks = 0, g_wrong = 0;
static void want(bool cond, const char* what, int a, int b, int c, int d) {
    g_checks++;
    if (!cond && g_wrong++ < 20) std::printf("WRONG %s (%d, %d, %d, %d)\n", what, a, b, c, d);
}

// the lane groups the LDS serves together: ds_read_b128 four of 16 lanes, ds_write_b128 eight of 8 lanes
static const int READ_GROUP[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};

// ring image: [chunk 4][plane 2][34 px][16 channels] f16; weight image (pack_t64_image): [chunk][tap][k half][64 rows][8] f16, row = block + channel_row(channel)
static int ring_byte(int chunk, int plane, int px, int ch) { return (2 * chunk + plane) * rsg::SEG + px * 32 + ch * 2; }
static int image_byte(int oc, int ic, int t) { return (ic >> 4) * rsg::WCH + t * 2048 + ((ic >> 3) & 1) * 1024 + ((oc & ~31) + rsg::channel_row(oc & 31)) * 16 + (ic & 7) * 2; }

int main() {
    std::vector<unsigned char> ring((size_t)rsg::ROWB), image((size_t)rsg::IMG_W), staged((size_t)rsg::STG_ROW);
    unsigned char frag[16];

    // (i), (ii) pixel side, (iv)
    for (int dx = 0; dx < 3; dx++)
        for (int cp = 0; cp < 2; cp++)
            for (int plane = 0; plane < 2; plane++) {
                std::vector<int> seen(34 * 32, 0);
                for (int ph = 0; ph < 2; ph++) {
                    for (int l = 0; l < 64; l++) {
                        const int off = rsg::pix_offset(l, dx, cp, plane, ph), kg = rsg::lane_kg(l);
                        const int seg = 2 * (2 * cp + rsg::kg_chunk(kg)) + plane;
                        const bool in = off >= seg * rsg::SEG && off + 16 <= (seg + 1) * rsg::SEG && off % 16 == 0;
                        want(in, "a pixel fragment leaves its ring segment", l, dx, cp * 2 + plane, ph);
                        if (!in) continue;
                        std::memcpy(frag, ring.data() + off, 16);
                        const int px = 16 * ph + rsg::lane_col(l) + dx;
                        for (int j = 0; j < 8; j++) {
                            const int k = 8 * kg + j;                    // channel of the pair
                            want(off + 2 * j == ring_byte(2 * cp + (k >> 4), plane, px, k & 15), "a pixel fragment element is not (pixel, k) of the ring image", l, dx, cp, j);
                            seen[px * 32 + k]++;
                        }
                    }
                    for (int grp = 0; grp < 4; grp++) {
                        unsigned slots = 0;
                        for (int i = 0; i < 16; i++) slots |= 1u << ((rsg::pix_offset(READ_GROUP[grp & 1][i] + 32 * (grp >> 1), dx, cp, plane, ph) / 16) % 16);
                        want(slots == 0xffffu, "a ds_read_b128 lane group has a bank conflict", grp, dx, cp * 2 + plane, ph);
                    }
                }
                for (int px = 0; px < 34; px++)
                    for (int k = 0; k < 32; k++) want(seen[px * 32 + k] == (px >= dx && px < dx + 32 ? 1 : 0), "pixel coverage of a tap", dx, cp, px, k);
            }

    // (i), (ii) weight side, (iii)
    for (int N = 0; N < 2; N++)
        for (int cp = 0; cp < 2; cp++)
            for (int t = 0; t < 9; t++) {
                std::vector<int> seen(32 * 32, 0);
                for (int half = 0; half < 2; half++)
                    for (int l = 0; l < 64; l++) {
                        const int off = rsg::w_offset(l, N, cp, t, half), kg = rsg::lane_kg(l), i = rsg::lane_col(l);
                        const bool in = off >= 0 && off + 16 <= rsg::IMG_W && off % 16 == 0;
                        want(in, "a weight fragment leaves the image", l, N, cp * 9 + t, half);
                        if (!in) continue;
                        std::memcpy(frag, image.data() + off, 16);
                        const int row = (off % 1024) / 16;
                        want((row & ~31) + rsg::row_channel(row & 31) == 32 * N + 16 * half + i, "tile row i is not channel 32 N + 16 half + i", l, N, half, row);
                        for (int j = 0; j < 8; j++) {
                            const int k = 8 * kg + j;
                            want(off + 2 * j == image_byte(32 * N + 16 * half + i, 32 * cp + k, t), "a weight fragment element is not (row, k) of the image", l, N, cp * 9 + t, j);
                            seen[(16 * half + i) * 32 + k]++;
                        }
                    }
                for (int e = 0; e < 32 * 32; e++) want(seen[e] == 1, "weight coverage of a tap", N, cp, t, e);
            }

    // (v) staging: the consumers' writes against the epilogue waves' reads (quad q of pixel px of chunk cc at (cc * 32 + px) * 64 + ((q ^ ((px >> 1) & 3)) << 4))
    {
        std::vector<int> seen(rsg::STG_ROW / 16, 0);
        for (int N = 0; N < 2; N++)
            for (int half = 0; half < 2; half++)
                for (int ph = 0; ph < 2; ph++) {
                    for (int l = 0; l < 64; l++) {
                        const int off = rsg::stg_offset(l, N, half, ph), px = 16 * ph + rsg::lane_col(l), q = rsg::lane_kg(l);
                        const bool in = off >= 0 && off + 16 <= rsg::STG_ROW && off % 16 == 0;
                        want(in, "a staging write leaves the staged row", l, N, half, ph);
                        if (!in) continue;
                        std::memcpy(staged.data() + off, frag, 16);
                        want(off == ((2 * N + half) * 32 + px) * 64 + ((q ^ ((px >> 1) & 3)) << 4), "a tile's quad is not where the epilogue reads channels 4 q .. 4 q + 3", l, N, half, ph);
                        seen[off / 16]++;
                    }
                    for (int grp = 0; grp < 8; grp++) {
                        unsigned slots = 0;
                        for (int i = 0; i < 8; i++) slots |= 1u << ((rsg::stg_offset(8 * grp + i, N, half, ph) / 16) % 8);
                        want(slots == 0xffu, "a ds_write_b128 lane group has a bank conflict", grp, N, half, ph);
                    }
                }
        for (int e = 0; e < rsg::STG_ROW / 16; e++) want(seen[e] == 1, "staging coverage", e, 0, 0, 0);
    }

    // (vi) identity
    for (int half = 0; half < 2; half++)
        for (int i = 0; i < 16; i++) {
            int ones = 0, at = -1;
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++)
                    if (rsg::lane_col(l) == i && rsg::id_one(l, half, j)) { ones++; at = 8 * rsg::lane_kg(l) + j; }
            want(ones == 1 && at == 16 * half + i, "identity fragment: one 1 per tile row at k = 16 half + i", half, i, ones, at);
        }

    // unit sequence
    for (int N = 0; N < 2; N++) {
        int seen[2][10][2] = {}, instr = 0, last_tap[2] = {-1, -1};
        for (int m = 0; m < rsg::NUNIT; m++) {
            const rsg::Unit u = rsg::unit(N, m);
            const bool ok = u.cp >= 0 && u.cp < 2 && u.t >= 0 && u.t < 9 && u.ph >= 0 && u.ph < 2;
            want(ok, "unit out of range", N, m, 0, 0);
            if (!ok) continue;
            seen[u.cp][u.idn ? 9 : u.t][u.ph]++;
            instr += 4;
            if (u.idn) want(u.cp == N && u.t == 4 && last_tap[u.cp] == 8, "the identity step follows the nine taps of chunk pair N, on the centre tap", N, m, u.cp, u.t);
            else { want(u.t >= last_tap[u.cp] && (u.cp == 0 || last_tap[0] == 8), "taps in order, chunk pair 0 first", N, m, u.cp, u.t); last_tap[u.cp] = u.t; }
        }
        want(instr == 152, "152 instructions per row", N, instr, 0, 0);
        for (int cp = 0; cp < 2; cp++)
            for (int t = 0; t < 10; t++)
                for (int ph = 0; ph < 2; ph++) want(seen[cp][t][ph] == (t < 9 || cp == N ? 1 : 0), "every (chunk pair, tap, pixel half) once", N, cp, t, ph);
    }

    std::printf("rs_frag_geom: %lld checks, %lld wrong\n", g_checks, g_wrong);
    return g_wrong ? 1 : 0;
}
