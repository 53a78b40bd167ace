// rife-hip — the reference's command line (src/main.cpp:102-121 usage, 442-917 main) on top of `class RIFE` (rife.h):
//
//     rife-hip -0 in0.png -1 in1.png -o out.png [options]
//     rife-hip -i indir -o outdir [options]
//
// Same flags, defaults, validation order and messages, frame / timestep schedule (src/main.cpp:705-731) and three-stage
// pipeline (load -> proc -> save over bounded queues, one RIFE per -g id, -j load:proc[,proc..]:save; src/main.cpp:248-436,
// 819-904), re-hosted on std::thread.  Codecs: PNG (8-bit, non-interlaced) through zlib, binary PPM, and WebP through the
// system libwebp (its stable simple API, declared below because the image ships the library without headers; lossless encoding
// like src/webp_image.h:66-68), and baseline JPEG through jpeg_codec.h (quality 100 on output like src/main.cpp:215).
// -a (absent in the reference, whose readers drop alpha): PNG, WebP and 32-bit BMP are read WITH their alpha, the frames cross the boundary as RGBA
// Mats (include/rife_hip.h RIFE_HIP_PIX_RGBA8) and leave as RGBA PNG or WebP.  Without -a nothing changes.
// Video mode (absent in the reference, whose frames are stills):  rife-hip -i in.y4m -o out.y4m|- -m .../rife-v4.6 [-n N] [-c MATRIX[:RANGE]]
// A YUV4MPEG2 file goes through the same pipeline as 4:2:0 frames (include/rife_hip.h RIFE_HIP_PIX_I420 / I420P10): no image codec and no colour conversion
// on the host, every input frame uploaded once (stream mode), output frames written in order.
// Host glue only: every pixel of arithmetic happens in librife_hip.so.
#include <dirent.h>
#include <fcntl.h>
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rife_hip.h"
#include "jpeg_codec.h"
#include "rife.h"

#ifdef RIFE_HIP_WITH_WEBP
extern "C" {      // libwebp simple API (webp/decode.h, webp/encode.h)
uint8_t* WebPDecodeRGB(const uint8_t* data, size_t data_size, int* width, int* height);
size_t WebPEncodeLosslessRGB(const uint8_t* rgb, int width, int height, int stride, uint8_t** output);
uint8_t* WebPDecodeRGBA(const uint8_t* data, size_t data_size, int* width, int* height);
size_t WebPEncodeLosslessRGBA(const uint8_t* rgba, int width, int height, int stride, uint8_t** output);
void WebPFree(void* ptr);
}
#endif

// ---------------------------------------------------------------------------------------------------------------
// image files: PNG (zlib) and PPM (P6)
// ---------------------------------------------------------------------------------------------------------------
static bool read_file(const std::string& path, std::vector<unsigned char>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

static uint32_t be32(const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

static int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// PNG (every colour type, bit depth and interlace mode stb_image reads) -> tightly packed 8-bit RGB
// `wide` != null (-b 10): a 16-bit file also leaves its full samples there (w x h x 3, host order); it stays empty for every other depth
// `alpha` != null (-a): the file's alpha as w x h bytes - the alpha channel of colour types 4 / 6 (16-bit: its high byte, like the colour), the tRNS chunk of a
// palette file (entries beyond it are opaque) or the tRNS colour key of a grey / RGB file (the pixel that equals the key in every bit is clear, all others
// opaque); it stays EMPTY for a file that has neither
// `wide_alpha` != null (-b 16 -a, with `wide`): the alpha channel of a 16-bit file of colour type 4 / 6 with its full samples (w x h, host order); empty otherwise
static bool decode_png(const std::vector<unsigned char>& d, int& w, int& h, std::vector<unsigned char>& rgb, std::vector<uint16_t>* wide = nullptr,
                       std::vector<unsigned char>* alpha = nullptr, std::vector<uint16_t>* wide_alpha = nullptr) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (d.size() < 33 || memcmp(d.data(), sig, 8)) return false;
    size_t pos = 8;
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<unsigned char> idat, pal, trns;
    while (pos + 12 <= d.size()) {
        const uint32_t len = be32(&d[pos]);
        const unsigned char* typ = &d[pos + 4];
        if (pos + 12 + (size_t)len > d.size()) return false;
        const unsigned char* body = &d[pos + 8];
        if (!memcmp(typ, "IHDR", 4)) {
            if (len != 13 || pos != 8) return false;          // IHDR is 13 bytes and the first chunk (a short one would be read past its end)
            w = (int)be32(body); h = (int)be32(body + 4); depth = body[8]; ctype = body[9]; interlace = body[12];
        }
        else if (!memcmp(typ, "PLTE", 4)) pal.assign(body, body + len);
        else if (!memcmp(typ, "tRNS", 4)) trns.assign(body, body + len);
        else if (!memcmp(typ, "IDAT", 4)) idat.insert(idat.end(), body, body + len);
        else if (!memcmp(typ, "IEND", 4)) break;
        pos += 12 + (size_t)len;
    }
    // every colour type / bit depth / interlace mode stb_image reads in the reference (1-, 2-, 4-, 8-, 16-bit; Adam7); like stb with
    // 3 requested channels: 16-bit samples keep their high byte, low-depth grey is scaled to 0..255, alpha (and tRNS) is dropped
    if (w <= 0 || h <= 0 || interlace > 1) return false;
    const int ch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!ch || (ctype == 3 && pal.empty())) return false;
    if (!(depth == 8 || depth == 16 || ((ctype == 0 || ctype == 3) && (depth == 1 || depth == 2 || depth == 4))) || (ctype == 3 && depth == 16)) return false;
    const int bpp = depth * ch, fb = std::max(1, bpp / 8);               // bits per pixel, bytes per filter unit
    auto row_bytes = [&](int pw) { return ((size_t)pw * bpp + 7) / 8; };
    // pass geometry: one pass for non-interlaced files, the seven Adam7 passes otherwise
    static const int X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
    const int npass = interlace ? 7 : 1;
    size_t total = 0;
    for (int p = 0; p < npass; p++) {
        const int pw = interlace ? (w - X0[p] + DX[p] - 1) / DX[p] : w, ph = interlace ? (h - Y0[p] + DY[p] - 1) / DY[p] : h;
        if (pw > 0 && ph > 0) total += (row_bytes(pw) + 1) * ph;
    }
    // a header that promises more pixels than the compressed data can hold (deflate expands at most ~1032 : 1) or than any frame has
    // (2^28 pixels = 16K x 16K) is refused before anything of that size is allocated
    if ((size_t)w * h > ((size_t)1 << 28) || total > idat.size() * 1100 + 65536) return false;
    std::vector<unsigned char> raw(total);
    uLongf rawlen = (uLongf)raw.size();
    if (uncompress(raw.data(), &rawlen, idat.data(), (uLong)idat.size()) != Z_OK || rawlen != raw.size()) return false;
    rgb.assign((size_t)w * h * 3, 0);
    if (alpha) alpha->clear();
    // a colour key is two bytes per channel whatever the depth (PNG 11.3.2.1); a short chunk is not a key
    const bool keyed = alpha && ((ctype == 0 && trns.size() >= 2) || (ctype == 2 && trns.size() >= 6));
    const bool has_alpha = alpha && (ctype == 4 || ctype == 6 || keyed || (ctype == 3 && !trns.empty()));
    if (has_alpha) alpha->assign((size_t)w * h, 255);
    if (wide) wide->clear();
    if (wide && depth == 16) wide->assign((size_t)w * h * 3, 0);
    if (wide_alpha) wide_alpha->clear();
    if (wide_alpha && wide && depth == 16 && (ctype == 4 || ctype == 6)) wide_alpha->assign((size_t)w * h, 0);
    const int gscale = depth == 1 ? 255 : depth == 2 ? 85 : depth == 4 ? 17 : 1;
    size_t off = 0;
    for (int p = 0; p < npass; p++) {
        const int pw = interlace ? (w - X0[p] + DX[p] - 1) / DX[p] : w, ph = interlace ? (h - Y0[p] + DY[p] - 1) / DY[p] : h;
        if (pw <= 0 || ph <= 0) continue;
        const size_t stride = row_bytes(pw);
        std::vector<unsigned char> img(stride * ph);
        for (int y = 0; y < ph; y++) {
            const unsigned char* src = &raw[off + (stride + 1) * y];
            unsigned char* cur = &img[stride * y];
            const unsigned char* up = y ? &img[stride * (y - 1)] : nullptr;
            const int ft = src[0];
            if (ft > 4) return false;
            const size_t F = (size_t)fb, head = std::min(F, stride);
            // the first pixel of a row has no left neighbour; after it one tight loop per filter type (this is 1/4 of the decode time)
            for (size_t x = 0; x < head; x++) {
                const int b = up ? up[x] : 0;
                cur[x] = (unsigned char)(src[1 + x] + (ft == 2 ? b : ft == 3 ? b >> 1 : ft == 4 ? paeth(0, b, 0) : 0));
            }
            const unsigned char* in = src + 1;
            switch (ft) {
                case 0: std::memcpy(cur + head, in + head, stride - head); break;
                case 1: for (size_t x = head; x < stride; x++) cur[x] = (unsigned char)(in[x] + cur[x - F]); break;
                case 2: if (up) { for (size_t x = head; x < stride; x++) cur[x] = (unsigned char)(in[x] + up[x]); } else std::memcpy(cur + head, in + head, stride - head); break;
                case 3: for (size_t x = head; x < stride; x++) cur[x] = (unsigned char)(in[x] + ((cur[x - F] + (up ? up[x] : 0)) >> 1)); break;
                default: for (size_t x = head; x < stride; x++) cur[x] = (unsigned char)(in[x] + paeth(cur[x - F], up ? up[x] : 0, up ? up[x - F] : 0)); break;
            }
        }
        off += (stride + 1) * ph;
        if (!interlace && depth == 8 && ctype == 2 && !keyed) { std::memcpy(rgb.data(), img.data(), img.size()); continue; }      // 8-bit RGB rows are the output rows
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                const unsigned char* row = &img[stride * y];
                auto sample = [&](int c) -> int {          // channel c of pixel x as 8 bits (index for palette images)
                    if (depth == 8) return row[(size_t)x * ch + c];
                    if (depth == 16) return row[((size_t)x * ch + c) * 2];
                    const int per = 8 / depth, sh = (per - 1 - x % per) * depth;
                    return (row[x / per] >> sh) & ((1 << depth) - 1);
                };
                const int ox = interlace ? X0[p] + x * DX[p] : x, oy = interlace ? Y0[p] + y * DY[p] : y;
                unsigned char* o = &rgb[((size_t)oy * w + ox) * 3];
                if (wide && depth == 16) {                  // grey / grey + alpha / rgb / rgb + alpha: big-endian samples
                    uint16_t* o16 = &(*wide)[((size_t)oy * w + ox) * 3];
                    for (int c = 0; c < 3; c++) {
                        const unsigned char* s16 = &row[((size_t)x * ch + (ch >= 3 ? c : 0)) * 2];
                        o16[c] = (uint16_t)((s16[0] << 8) | s16[1]);
                    }
                    if (wide_alpha && !wide_alpha->empty()) {
                        const unsigned char* s16 = &row[((size_t)x * ch + (ch - 1)) * 2];
                        (*wide_alpha)[(size_t)oy * w + ox] = (uint16_t)((s16[0] << 8) | s16[1]);
                    }
                }
                if (has_alpha) {
                    unsigned char& al = (*alpha)[(size_t)oy * w + ox];
                    if (ctype == 4 || ctype == 6) al = (unsigned char)sample(ch - 1);
                    else if (ctype == 3) { const size_t k = (size_t)sample(0); if (k < trns.size()) al = trns[k]; }
                    else {                                      // colour key: every bit of every channel (the raw sample, before any scaling)
                        bool same = true;
                        for (int c = 0; c < ch && same; c++) {
                            const int key = (trns[2 * c] << 8) | trns[2 * c + 1];
                            const int v = depth == 16 ? ((row[((size_t)x * ch + c) * 2] << 8) | row[((size_t)x * ch + c) * 2 + 1]) : sample(c);
                            same = v == key;
                        }
                        if (same) al = 0;
                    }
                }
                if (ctype == 2 || ctype == 6) { o[0] = (unsigned char)sample(0); o[1] = (unsigned char)sample(1); o[2] = (unsigned char)sample(2); }
                else if (ctype == 0 || ctype == 4) { o[0] = o[1] = o[2] = (unsigned char)(sample(0) * (depth < 8 ? gscale : 1)); }
                else {
                    const size_t k = (size_t)sample(0) * 3;
                    if (k + 2 >= pal.size()) return false;
                    o[0] = pal[k]; o[1] = pal[k + 1]; o[2] = pal[k + 2];
                }
            }
    }
    return true;
}

// BMP as stb_image reads it in the reference: uncompressed 24- / 32-bit (BI_RGB, or BI_BITFIELDS with the standard masks) and 8-bit palette
// `alpha` != null (-a): a 32-bit file's alpha as w x h bytes - the fourth byte of BI_RGB pixels, or the alpha mask of a BI_BITFIELDS header that has one;
// like stb_image, a file whose alpha is zero in EVERY pixel is read as opaque (writers that leave the fourth byte unused).  Empty for 24- and 8-bit files.
static bool decode_bmp(const std::vector<unsigned char>& d, int& w, int& h, std::vector<unsigned char>& rgb, std::vector<unsigned char>* alpha = nullptr) {
    if (d.size() < 54 || d[0] != 'B' || d[1] != 'M') return false;
    auto le32 = [&](size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24); };
    const uint32_t dataoff = le32(10), hsz = le32(14);
    if (hsz < 40 || 14 + (size_t)hsz > d.size()) return false;
    const int bw = (int)le32(18), bh = (int)le32(22), bits = d[28] | (d[29] << 8);
    const uint32_t comp = le32(30);
    if (bw <= 0 || bh == 0 || (d[26] | (d[27] << 8)) != 1) return false;
    if (!((bits == 24 && comp == 0) || (bits == 32 && (comp == 0 || comp == 3)) || (bits == 8 && comp == 0))) return false;
    const bool flip = bh > 0;                                 // positive height = bottom-up rows
    w = bw; h = bh > 0 ? bh : -bh;
    const size_t stride = ((size_t)w * bits / 8 + 3) & ~(size_t)3;
    if ((size_t)dataoff + stride * h > d.size()) return false;
    const unsigned char* pal = &d[14 + hsz];
    uint32_t ncol = le32(46);
    if (bits == 8) { if (!ncol) ncol = 256; if (14 + (size_t)hsz + 4 * (size_t)ncol > d.size()) return false; }
    if (alpha) alpha->clear();
    int rs = 16, gs = 8, bs = 0, as = bits == 32 && comp == 0 ? 24 : -1;      // 32-bit BI_RGB is B, G, R, X (A with -a)
    if (bits == 32 && comp == 3) {
        if (hsz < 52 && 14 + (size_t)hsz + 12 > d.size()) return false;
        const uint32_t rm = le32(54), gm = le32(58), bm = le32(62);
        auto shift_of = [](uint32_t m) { int sft = 0; while (m && !(m & 1)) { m >>= 1; sft++; } return m == 0xff ? sft : -1; };
        rs = shift_of(rm); gs = shift_of(gm); bs = shift_of(bm);
        if (rs < 0 || gs < 0 || bs < 0) return false;
        if (hsz >= 56 && le32(66)) { as = shift_of(le32(66)); if (as < 0) return false; }      // V3+ header: alpha mask (14 + hsz <= d.size() was checked)
    }
    if (alpha && as >= 0) alpha->assign((size_t)w * h, 0);
    bool any_alpha = false;
    rgb.resize((size_t)w * h * 3);
    for (int y = 0; y < h; y++) {
        const unsigned char* row = &d[dataoff + stride * (size_t)(flip ? h - 1 - y : y)];
        unsigned char* o = &rgb[(size_t)y * w * 3];
        for (int x = 0; x < w; x++, o += 3) {
            if (bits == 24) { o[0] = row[3 * x + 2]; o[1] = row[3 * x + 1]; o[2] = row[3 * x]; }
            else if (bits == 32) {
                const uint32_t v = (uint32_t)row[4 * x] | ((uint32_t)row[4 * x + 1] << 8) | ((uint32_t)row[4 * x + 2] << 16) | ((uint32_t)row[4 * x + 3] << 24);
                o[0] = (unsigned char)(v >> rs); o[1] = (unsigned char)(v >> gs); o[2] = (unsigned char)(v >> bs);
                if (alpha && as >= 0) { const unsigned char al = (unsigned char)(v >> as); (*alpha)[(size_t)y * w + x] = al; any_alpha |= al != 0; }
            } else {
                if (row[x] >= ncol) return false;
                const unsigned char* e = pal + 4 * (size_t)row[x];
                o[0] = e[2]; o[1] = e[1]; o[2] = e[0];
            }
        }
    }
    if (alpha && as >= 0 && !any_alpha) alpha->assign((size_t)w * h, 255);
    return true;
}

static void put_chunk(std::vector<unsigned char>& out, const char* typ, const unsigned char* body, size_t len) {
    const unsigned char l[4] = {(unsigned char)(len >> 24), (unsigned char)(len >> 16), (unsigned char)(len >> 8), (unsigned char)len};
    out.insert(out.end(), l, l + 4);
    const size_t start = out.size();
    out.insert(out.end(), typ, typ + 4);
    if (len) out.insert(out.end(), body, body + len);
    const uint32_t crc = (uint32_t)crc32(0L, &out[start], (uInt)(len + 4));
    const unsigned char c[4] = {(unsigned char)(crc >> 24), (unsigned char)(crc >> 16), (unsigned char)(crc >> 8), (unsigned char)crc};
    out.insert(out.end(), c, c + 4);
}

// Helper threads one encode_png() call may use besides its own (set in main() from the core count and the -j settings).
static int g_png_helpers = 0;

// One band of rows: filter "up" (cheap and effective on video frames; the first row of the image has no row above) and raw deflate.
// Every band but the last ends with a sync flush, i.e. on a byte boundary, so the bands concatenate into one valid deflate stream -
// the bands share no history, which costs a little ratio and lets them run on separate cores.
static bool png_deflate_band(const unsigned char* rgb, size_t stride, int y0, int y1, bool last, std::vector<unsigned char>& comp, uLong& adler) {
    std::vector<unsigned char> raw((stride + 1) * (size_t)(y1 - y0));
    for (int y = y0; y < y1; y++) {
        unsigned char* dst = &raw[(stride + 1) * (size_t)(y - y0)];
        const unsigned char* cur = rgb + stride * y;
        const unsigned char* up = y ? rgb + stride * (y - 1) : nullptr;
        dst[0] = up ? 2 : 0;
        if (up) for (size_t x = 0; x < stride; x++) dst[1 + x] = (unsigned char)(cur[x] - up[x]);
        else std::memcpy(dst + 1, cur, stride);
    }
    adler = adler32(adler32(0L, Z_NULL, 0), raw.data(), (uInt)raw.size());
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 3, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    comp.resize(deflateBound(&z, (uLong)raw.size()) + 16);
    z.next_in = raw.data(); z.avail_in = (uInt)raw.size();
    z.next_out = comp.data(); z.avail_out = (uInt)comp.size();
    const int rc = deflate(&z, last ? Z_FINISH : Z_SYNC_FLUSH);
    const bool ok = last ? rc == Z_STREAM_END : (rc == Z_OK && z.avail_in == 0 && z.avail_out != 0);
    comp.resize(comp.size() - z.avail_out);
    deflateEnd(&z);
    return ok;
}

// depth 8: rgb = w x h x 3 bytes; depth 16 (-b 10): w x h x 3 big-endian 16-bit samples; ch = 4 (-a): w x h x 4 bytes R G B A, colour type 6
static bool encode_png(const std::string& path, int w, int h, const unsigned char* rgb, int depth = 8, int ch = 3) {
    const size_t stride = (size_t)w * ch * (depth / 8);
    // bands of about 1 MB of pixels, at most 64 (a band must stay below the 4 GB zlib counts in any case)
    int nband = (int)std::min<size_t>(64, std::max<size_t>(1, stride * h >> 20));
    nband = std::min(nband, h);
    std::vector<std::vector<unsigned char>> comp(nband);
    std::vector<uLong> adler(nband);
    std::vector<size_t> rawlen(nband);
    std::vector<char> good(nband, 0);
    std::atomic<int> next(0);
    auto work = [&]() {
        for (int b; (b = next.fetch_add(1)) < nband;) {
            const int y0 = (int)((long long)h * b / nband), y1 = (int)((long long)h * (b + 1) / nband);
            rawlen[b] = (stride + 1) * (size_t)(y1 - y0);
            good[b] = png_deflate_band(rgb, stride, y0, y1, b == nband - 1, comp[b], adler[b]);
        }
    };
    std::vector<std::thread> helpers;
    for (int i = 0; i < std::min(g_png_helpers, nband - 1); i++) helpers.emplace_back(work);
    work();
    for (auto& t : helpers) t.join();
    std::vector<unsigned char> zs = {0x78, 0x5e};                       // zlib header: deflate, 32 KB window, "fast" level hint
    uLong ad = adler32(0L, Z_NULL, 0);
    for (int b = 0; b < nband; b++) {
        if (!good[b]) return false;
        zs.insert(zs.end(), comp[b].begin(), comp[b].end());
        ad = adler32_combine(ad, adler[b], (z_off_t)rawlen[b]);
    }
    for (int i = 3; i >= 0; i--) zs.push_back((unsigned char)(ad >> (8 * i)));
    const unsigned char* const comp_data = zs.data();
    const size_t clen = zs.size();
    std::vector<unsigned char> out = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    unsigned char ihdr[13] = {(unsigned char)(w >> 24), (unsigned char)(w >> 16), (unsigned char)(w >> 8), (unsigned char)w,
                              (unsigned char)(h >> 24), (unsigned char)(h >> 16), (unsigned char)(h >> 8), (unsigned char)h, (unsigned char)depth, (unsigned char)(ch == 4 ? 6 : 2), 0, 0, 0};
    put_chunk(out, "IHDR", ihdr, 13);
    put_chunk(out, "IDAT", comp_data, clen);
    put_chunk(out, "IEND", nullptr, 0);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

// `wide` != null (-b 10): files with maxval 1023 or 65535 (two bytes per sample, big-endian) are read too, their samples go to *wide (host order) and
// *maxval says which; a maxval-255 file is read as always and leaves *wide empty
static bool decode_ppm(const std::vector<unsigned char>& d, int& w, int& h, std::vector<unsigned char>& rgb, std::vector<uint16_t>* wide = nullptr, int* maxval = nullptr) {
    if (wide) wide->clear();
    if (d.size() < 7 || d[0] != 'P' || (d[1] != '6' && d[1] != '5')) return false;      // P6 = rgb, P5 = grey (stb_image's pnm reader takes both)
    const bool grey = d[1] == '5';
    size_t pos = 2;
    int vals[3], n = 0;
    while (n < 3 && pos < d.size()) {
        while (pos < d.size() && (isspace(d[pos]) || d[pos] == '#')) { if (d[pos] == '#') while (pos < d.size() && d[pos] != '\n') pos++; else pos++; }
        int v = 0; bool any = false;
        while (pos < d.size() && isdigit(d[pos])) { v = v * 10 + (d[pos] - '0'); pos++; any = true; }
        if (!any) return false;
        vals[n++] = v;
    }
    if (n != 3 || pos >= d.size()) return false;
    if (wide && !grey && (vals[2] == 1023 || vals[2] == 65535)) {
        pos++;
        w = vals[0]; h = vals[1];
        if (w <= 0 || h <= 0 || (size_t)w * h > ((size_t)1 << 28) || d.size() - pos < (size_t)w * h * 6) return false;
        wide->resize((size_t)w * h * 3);
        for (size_t i = 0; i < wide->size(); i++) {
            const unsigned v = ((unsigned)d[pos + 2 * i] << 8) | d[pos + 2 * i + 1];
            if (v > (unsigned)vals[2]) return false;                     // a sample above maxval: not a valid file
            (*wide)[i] = (uint16_t)v;
        }
        if (maxval) *maxval = vals[2];
        return true;
    }
    if (vals[2] != 255) return false;
    pos++;                                       // the single whitespace after maxval
    w = vals[0]; h = vals[1];
    if (w <= 0 || h <= 0 || d.size() - pos < (size_t)w * h * (grey ? 1 : 3)) return false;
    if (!grey) { rgb.assign(d.begin() + pos, d.begin() + pos + (size_t)w * h * 3); return true; }
    rgb.resize((size_t)w * h * 3);
    for (size_t i = 0; i < (size_t)w * h; i++) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = d[pos + i];
    return true;
}

static bool encode_ppm(const std::string& path, int w, int h, const unsigned char* rgb) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    const bool ok = fwrite(rgb, 1, (size_t)w * h * 3, f) == (size_t)w * h * 3;
    fclose(f);
    return ok;
}

// -b 10: P6 with maxval 1023, two bytes per sample, most significant first (Netpbm)
static bool encode_ppm10(const std::string& path, int w, int h, const uint16_t* codes) {
    std::vector<unsigned char> be((size_t)w * h * 6);
    for (size_t i = 0; i < (size_t)w * h * 3; i++) { const unsigned c = std::min<unsigned>(codes[i], 1023u); be[2 * i] = (unsigned char)(c >> 8); be[2 * i + 1] = (unsigned char)c; }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n1023\n", w, h);
    const bool ok = fwrite(be.data(), 1, be.size(), f) == be.size();
    fclose(f);
    return ok;
}

static bool decode_webp(const std::vector<unsigned char>& d, int& w, int& h, std::vector<unsigned char>& rgb) {
#ifdef RIFE_HIP_WITH_WEBP
    if (d.size() < 12 || memcmp(d.data(), "RIFF", 4) || memcmp(d.data() + 8, "WEBP", 4)) return false;
    uint8_t* px = WebPDecodeRGB(d.data(), d.size(), &w, &h);
    if (!px) return false;
    rgb.assign(px, px + (size_t)w * h * 3);
    WebPFree(px);
    return true;
#else
    (void)d; (void)w; (void)h; (void)rgb;
    return false;
#endif
}

static bool encode_webp(const std::string& path, int w, int h, const unsigned char* rgb) {
#ifdef RIFE_HIP_WITH_WEBP
    uint8_t* out = nullptr;
    const size_t n = WebPEncodeLosslessRGB(rgb, w, h, w * 3, &out);
    if (!n || !out) return false;
    FILE* f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(out, 1, n, f) == n;
    if (f) fclose(f);
    WebPFree(out);
    return ok;
#else
    (void)path; (void)w; (void)h; (void)rgb;
    return false;
#endif
}

static bool decode_webp_rgba(const std::vector<unsigned char>& d, int& w, int& h, std::vector<unsigned char>& rgba) {
#ifdef RIFE_HIP_WITH_WEBP
    if (d.size() < 12 || memcmp(d.data(), "RIFF", 4) || memcmp(d.data() + 8, "WEBP", 4)) return false;
    uint8_t* px = WebPDecodeRGBA(d.data(), d.size(), &w, &h);      // a file without alpha comes back opaque
    if (!px) return false;
    rgba.assign(px, px + (size_t)w * h * 4);
    WebPFree(px);
    return true;
#else
    (void)d; (void)w; (void)h; (void)rgba;
    return false;
#endif
}

// lossless, but libwebp's simple API does not keep the colour under fully transparent pixels (its `exact` option is off)
static bool encode_webp_rgba(const std::string& path, int w, int h, const unsigned char* rgba) {
#ifdef RIFE_HIP_WITH_WEBP
    uint8_t* out = nullptr;
    const size_t n = WebPEncodeLosslessRGBA(rgba, w, h, w * 4, &out);
    if (!n || !out) return false;
    FILE* f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(out, 1, n, f) == n;
    if (f) fclose(f);
    WebPFree(out);
    return ok;
#else
    (void)path; (void)w; (void)h; (void)rgba;
    return false;
#endif
}

static bool encode_image(const std::string& path, int w, int h, const unsigned char* rgb);

static std::string ext_of(const std::string& p) {
    const size_t dot = p.rfind('.');
    if (dot == std::string::npos || p.find('/', dot) != std::string::npos) return "";
    std::string e = p.substr(dot + 1);
    std::transform(e.begin(), e.end(), e.begin(), ::tolower);
    return e;
}

static bool decode_image(const std::string& path, int& w, int& h, std::vector<unsigned char>& rgb) {
    std::vector<unsigned char> d;
    if (!read_file(path, d)) return false;
    if (decode_png(d, w, h, rgb) || decode_ppm(d, w, h, rgb) || decode_webp(d, w, h, rgb) || decode_bmp(d, w, h, rgb)) return true;
    std::string why;
    if (jpeg::decode(d, w, h, rgb, &why)) return true;
    if (d.size() > 2 && d[0] == 0xFF && d[1] == 0xD8) fprintf(stderr, "%s: %s\n", path.c_str(), why.c_str());
    return false;
}

static bool encode_image(const std::string& path, int w, int h, const unsigned char* rgb) {
    const std::string e = ext_of(path);
    if (e == "ppm") return encode_ppm(path, w, h, rgb);
    if (e == "webp") return encode_webp(path, w, h, rgb);
    if (e == "jpg" || e == "jpeg") return jpeg::encode(path, w, h, rgb, g_png_helpers);      // same spare cores as the PNG writer
    return encode_png(path, w, h, rgb);
}

// ---- -a: frames as RGBA (u8 x 4 per pixel; include/rife_hip.h RIFE_HIP_PIX_RGBA8): a file without alpha is read as opaque ----
static bool decode_image_rgba(const std::string& path, int& w, int& h, std::vector<unsigned char>& rgba) {
    std::vector<unsigned char> d, rgb, al;
    if (!read_file(path, d)) return false;
    if (decode_webp_rgba(d, w, h, rgba)) return true;
    if (!(decode_png(d, w, h, rgb, nullptr, &al) || decode_ppm(d, w, h, rgb) || decode_bmp(d, w, h, rgb, &al))) {
        std::string why;
        al.clear();
        if (!jpeg::decode(d, w, h, rgb, &why)) {
            if (d.size() > 2 && d[0] == 0xFF && d[1] == 0xD8) fprintf(stderr, "%s: %s\n", path.c_str(), why.c_str());
            return false;
        }
    }
    const size_t n = (size_t)w * h;
    if (rgb.size() != n * 3 || (!al.empty() && al.size() != n)) return false;
    rgba.resize(n * 4);
    for (size_t i = 0; i < n; i++) { rgba[4 * i] = rgb[3 * i]; rgba[4 * i + 1] = rgb[3 * i + 1]; rgba[4 * i + 2] = rgb[3 * i + 2]; rgba[4 * i + 3] = al.empty() ? 255 : al[i]; }
    return true;
}

// .png: colour type 6, 8 bits; .webp: lossless with alpha; jpg and ppm have no alpha (refused at start-up)
static bool encode_image_rgba(const std::string& path, int w, int h, const unsigned char* rgba) {
    const std::string e = ext_of(path);
    if (e == "webp") return encode_webp_rgba(path, w, h, rgba);
    if (e == "ppm" || e == "jpg" || e == "jpeg") return false;
    return encode_png(path, w, h, rgba, 8, 4);
}

// ---- -b 10: frames as 10-bit codes (u16 x 3 per pixel, 0..1023; include/rife_hip.h RIFE_HIP_PIX_RGB10_U16) ----
// a 16-bit PNG or a PPM with maxval 65535: code = v >> 6; a PPM with maxval 1023: its codes; every 8-bit file: (v << 2) | (v >> 6)
static bool decode_image10(const std::string& path, int& w, int& h, std::vector<uint16_t>& codes) {
    std::vector<unsigned char> d, rgb;
    if (!read_file(path, d)) return false;
    std::vector<uint16_t> wide;
    int maxval = 0;
    if (decode_png(d, w, h, rgb, &wide)) {
        if (!wide.empty()) { codes.resize(wide.size()); for (size_t i = 0; i < wide.size(); i++) codes[i] = (uint16_t)(wide[i] >> 6); return true; }
    } else if (decode_ppm(d, w, h, rgb, &wide, &maxval)) {
        if (!wide.empty()) { codes.resize(wide.size()); for (size_t i = 0; i < wide.size(); i++) codes[i] = (uint16_t)(maxval == 1023 ? wide[i] : wide[i] >> 6); return true; }
    } else if (!(decode_webp(d, w, h, rgb) || decode_bmp(d, w, h, rgb))) {
        std::string why;
        if (!jpeg::decode(d, w, h, rgb, &why)) {
            if (d.size() > 2 && d[0] == 0xFF && d[1] == 0xD8) fprintf(stderr, "%s: %s\n", path.c_str(), why.c_str());
            return false;
        }
    }
    codes.resize(rgb.size());
    for (size_t i = 0; i < rgb.size(); i++) codes[i] = (uint16_t)((rgb[i] << 2) | (rgb[i] >> 6));
    return true;
}

// .png: 16-bit RGB, v = (code << 6) | (code >> 4) - the code's bits repeated into the low six, so that full scale maps to full scale and reading the file back
// with -b 10 (v >> 6) returns the codes; .ppm: P6 with maxval 1023
static bool encode_image10(const std::string& path, int w, int h, const uint16_t* codes) {
    const std::string e = ext_of(path);
    if (e == "ppm") return encode_ppm10(path, w, h, codes);
    if (e == "webp" || e == "jpg" || e == "jpeg") return false;          // 8-bit containers (refused at start-up)
    std::vector<unsigned char> be((size_t)w * h * 6);
    for (size_t i = 0; i < (size_t)w * h * 3; i++) {
        const unsigned c = std::min<unsigned>(codes[i], 1023u), v = (c << 6) | (c >> 4);
        be[2 * i] = (unsigned char)(v >> 8); be[2 * i + 1] = (unsigned char)v;
    }
    return encode_png(path, w, h, be.data(), 16);
}

// ---- -b 16 [-a]: frames as 16-bit samples (u16 x 3 or x 4 per pixel, R G B (A) interleaved; include/rife_hip.h rife_hip_packed_t) ----
// a 16-bit PNG (colour types 0, 2, 4, 6) or a PPM with maxval 65535: the full samples; a PPM with maxval 1023: (c << 6) | (c >> 4); every 8-bit file: v * 257.
// ch = 4 (-a): a 16-bit alpha channel in full, 8-bit alpha (and a tRNS colour key or palette entry, 0 / 255 / the entry) as a * 257, a file without alpha opaque
static bool decode_image16(const std::string& path, int& w, int& h, int ch, std::vector<uint16_t>& px) {
    std::vector<unsigned char> d, rgb, al;
    if (!read_file(path, d)) return false;
    std::vector<uint16_t> wide, wal;
    int maxval = 0;
    if (decode_png(d, w, h, rgb, &wide, ch == 4 ? &al : nullptr, ch == 4 ? &wal : nullptr)) {
    } else if (decode_ppm(d, w, h, rgb, &wide, &maxval)) {
        al.clear(); wal.clear();
        if (maxval == 1023) for (uint16_t& c : wide) c = (uint16_t)((c << 6) | (c >> 4));
    } else {
        wide.clear(); wal.clear();
        if (ch == 4) {                                                   // WebP, BMP, JPEG: the 8-bit readers of -a
            std::vector<unsigned char> rgba;
            if (!decode_image_rgba(path, w, h, rgba)) return false;
            px.resize(rgba.size());
            for (size_t i = 0; i < rgba.size(); i++) px[i] = (uint16_t)(rgba[i] * 257);
            return true;
        }
        if (!(decode_webp(d, w, h, rgb) || decode_bmp(d, w, h, rgb))) {
            std::string why;
            if (!jpeg::decode(d, w, h, rgb, &why)) {
                if (d.size() > 2 && d[0] == 0xFF && d[1] == 0xD8) fprintf(stderr, "%s: %s\n", path.c_str(), why.c_str());
                return false;
            }
        }
    }
    const size_t n = (size_t)w * h;
    if ((wide.empty() ? rgb.size() : wide.size()) != n * 3 || (!wal.empty() && wal.size() != n) || (!al.empty() && al.size() != n)) return false;
    px.resize(n * ch);
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) px[i * ch + c] = wide.empty() ? (uint16_t)(rgb[3 * i + c] * 257) : wide[3 * i + c];
        if (ch == 4) px[i * 4 + 3] = !wal.empty() ? wal[i] : !al.empty() ? (uint16_t)(al[i] * 257) : (uint16_t)65535;
    }
    return true;
}

// .png: 16-bit RGB, or colour type 6 for ch = 4, the samples as they are; .ppm: P6 with maxval 65535, ch = 3 only
static bool encode_image16(const std::string& path, int w, int h, int ch, const uint16_t* px) {
    const std::string e = ext_of(path);
    if (e == "webp" || e == "jpg" || e == "jpeg" || (e == "ppm" && ch != 3)) return false;      // refused at start-up
    std::vector<unsigned char> be((size_t)w * h * ch * 2);
    for (size_t i = 0; i < (size_t)w * h * ch; i++) { be[2 * i] = (unsigned char)(px[i] >> 8); be[2 * i + 1] = (unsigned char)px[i]; }
    if (e != "ppm") return encode_png(path, w, h, be.data(), 16, ch);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n65535\n", w, h);
    const bool ok = fwrite(be.data(), 1, be.size(), f) == be.size();
    fclose(f);
    return ok;
}

// ---------------------------------------------------------------------------------------------------------------
// tasks and queues (src/main.cpp:231-295)
// ---------------------------------------------------------------------------------------------------------------
// A decoded frame plus its copies in device memory, one per engine that has needed it so far (uploaded by the first proc thread
// that does).  The reference uploads both frames in every process() call (src/rife.cpp:2490-2530); in a sequence each frame serves
// two pairs and, with -n, several timesteps per pair, so the upload happens once here.
struct SharedFrame {
    int w = 0, h = 0;
    std::vector<unsigned char> px;
    std::vector<uint16_t> px10;                                       // -b 10: the frame as 10-bit codes instead of px
    std::vector<uint16_t> px16;                                       // -b 16: the frame as 16-bit samples, three or (-a) four per pixel, instead of px; never resident
    bool rgba = false;                                                // -a: px holds four bytes per pixel, R G B A
    int yuv = 0;                                                      // video mode: px holds one 4:2:0 frame of this pixfmt (RIFE_HIP_PIX_I420 / I420P10 | RIFE_HIP_CSP_*)
    const rife_hip_frame* on(const RIFE* r) {
        std::lock_guard<std::mutex> g(mu);
        for (auto& e : resident) if (e.first == r) return e.second;
        rife_hip_frame* f = yuv          ? r->upload_yuv(px.data(), w, h, yuv)
                            : rgba       ? r->upload(ncnn::Mat(w, h, (void*)px.data(), (size_t)4, 4))      // elemsize 4, elempack 4 = RGBA8 (rife.cpp)
                            : px10.empty() ? r->upload(ncnn::Mat(w, h, (void*)px.data(), (size_t)3, 3))
                                         : r->upload(ncnn::Mat(w, h, (void*)px10.data(), (size_t)6, 3));      // elemsize 6, elempack 3 = RGB10_U16 (rife.cpp)
        if (f) resident.emplace_back(r, f);
        return f;
    }
    ~SharedFrame() { for (auto& e : resident) RIFE::release(e.second); }
private:
    std::mutex mu;
    std::vector<std::pair<const RIFE*, rife_hip_frame*>> resident;
};

struct Task {
    int id = 0;
    float timestep = 0.5f;
    std::string in0path, in1path, outpath;
    std::shared_ptr<SharedFrame> fr0, fr1;                            // decoded frames are shared between the tasks that use them
    std::vector<unsigned char> out;
    std::vector<uint16_t> out10;                                      // -b 10
    std::vector<uint16_t> out16;                                      // -b 16
    int w = 0, h = 0;
};

// Decoded-frame cache: in directory mode consecutive tasks use the same files (output i takes frames sx, sx + 1; with the default
// -n every input frame is needed by about four tasks), and decoding is the slowest stage of the whole program.  The reference
// decodes per task (src/main.cpp:315-334); this keeps the last few decoded frames.
class FrameCache {
public:
    typedef std::shared_ptr<SharedFrame> Frame;
    // decode(path, frame) fills the frame's size and pixels
    template <class Decode>
    bool get(const std::string& path, Frame& f, Decode decode) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (auto& e : entries) if (e.first == path) { f = e.second; return true; }
        }
        Frame n = std::make_shared<SharedFrame>();
        if (!decode(path, *n)) return false;
        std::lock_guard<std::mutex> g(mu);
        for (auto& e : entries) if (e.first == path) { f = e.second; return true; }     // another loader decoded it meanwhile: keep one copy
        entries.emplace_back(path, n);
        if (entries.size() > 6) entries.erase(entries.begin());
        f = n;
        return true;
    }
    void clear() { std::lock_guard<std::mutex> g(mu); entries.clear(); }
private:
    std::mutex mu;
    std::vector<std::pair<std::string, Frame>> entries;
};

class TaskQueue {
public:
    void put(Task&& t) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return q.size() < 8; });          // bounded at 8 like the reference (main.cpp:260)
        q.push(std::move(t));
        cv.notify_all();
    }
    Task get() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q.empty(); });
        Task t = std::move(q.front());
        q.pop();
        cv.notify_all();
        return t;
    }
private:
    std::mutex mu;
    std::condition_variable cv;
    std::queue<Task> q;
};

// ---------------------------------------------------------------------------------------------------------------
// YUV4MPEG2 (video mode)
// ---------------------------------------------------------------------------------------------------------------
// The frame / timestep schedule of directory mode (src/main.cpp:705-731): output i of numframe over `count` input frames takes frames sx, sx + 1 at fx.
static void schedule_step(int i, int count, int numframe, int& sx, float& fx) {
    const double scale = (double)count / numframe;                          // double product rounded to float, like src/main.cpp:713-718
    fx = (float)(i * scale);
    sx = (int)std::floor(fx);
    fx -= sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= count - 1) { sx = count - 2; fx = 1.f; }
}

struct Y4m {
    int fd = -1;
    int w = 0, h = 0;
    long long fnum = 0, fden = 0;
    bool p10 = false;                                                 // C420p10: u16 little-endian samples, the code in the low ten bits
    int range = -1;                                                   // XCOLORRANGE: 1 FULL, 0 LIMITED, -1 absent
    std::vector<std::string> other;                                   // every header field but W, H, F, verbatim and in order (I, A, C, X...)
    size_t hdr_len = 0, frame_bytes = 0;
    long long count = 0;
    ~Y4m() { if (fd >= 0) close(fd); }
    // frame k: the bytes after its "FRAME\n" marker
    bool read_frame(long long k, std::vector<unsigned char>& px) const {
        px.resize(frame_bytes);
        const off_t at = (off_t)hdr_len + (off_t)k * (off_t)(frame_bytes + 6) + 6;
        size_t got = 0;
        while (got < frame_bytes) {
            const ssize_t n = pread(fd, px.data() + got, frame_bytes - got, at + (off_t)got);
            if (n <= 0) return false;
            got += (size_t)n;
        }
        return true;
    }
};

// Header: "YUV4MPEG2 W H F [I] [A] [C] [X...]" and a newline within the first 256 bytes; progressive 4:2:0 at 8 or 10 bits only.  The frame count comes from the
// file size; every frame starts with a plain "FRAME\n".
static bool y4m_open(const std::string& path, Y4m& y, std::string& err) {
    y.fd = open(path.c_str(), O_RDONLY);
    struct stat st;
    if (y.fd < 0 || fstat(y.fd, &st) != 0 || !S_ISREG(st.st_mode)) { err = "cannot open " + path; return false; }
    char buf[256];
    const ssize_t n = pread(y.fd, buf, sizeof buf, 0);
    const char* nl = n > 0 ? (const char*)memchr(buf, '\n', (size_t)n) : nullptr;
    if (!nl) { err = "no YUV4MPEG2 header line in the first 256 bytes"; return false; }
    const std::string line(buf, (size_t)(nl - buf));
    y.hdr_len = (size_t)(nl - buf) + 1;
    if (line.compare(0, 9, "YUV4MPEG2") != 0 || (line.size() > 9 && line[9] != ' ')) { err = "not a YUV4MPEG2 file"; return false; }
    bool have_c = false;
    size_t pos = 9;
    while (pos < line.size()) {
        while (pos < line.size() && line[pos] == ' ') pos++;
        const size_t e = std::min(line.find(' ', pos), line.size());
        if (e == pos) break;
        const std::string tok = line.substr(pos, e - pos);
        pos = e;
        const std::string val = tok.substr(1);
        auto number = [&](long long& v) {
            if (val.empty() || val.size() > 9 || val.find_first_not_of("0123456789") != std::string::npos) return false;
            v = atoll(val.c_str());
            return true;
        };
        if (tok[0] == 'W' || tok[0] == 'H') {
            long long v = 0;
            if (!number(v) || v < 1 || v > 65535) { err = "bad frame size field '" + tok + "'"; return false; }
            (tok[0] == 'W' ? y.w : y.h) = (int)v;
        } else if (tok[0] == 'F') {
            const size_t c = val.find(':');
            const std::string a = val.substr(0, c), b = c == std::string::npos ? "" : val.substr(c + 1);
            if (a.empty() || b.empty() || a.size() > 9 || b.size() > 9 || a.find_first_not_of("0123456789") != std::string::npos ||
                b.find_first_not_of("0123456789") != std::string::npos || atoll(a.c_str()) < 1 || atoll(b.c_str()) < 1) { err = "bad frame rate field '" + tok + "'"; return false; }
            y.fnum = atoll(a.c_str()); y.fden = atoll(b.c_str());
        } else {
            if (tok[0] == 'I' && tok != "Ip") { err = "interlacing '" + tok + "' is not served (progressive frames, Ip, only)"; return false; }
            if (tok[0] == 'C') {
                have_c = true;
                if (tok == "C420p10") y.p10 = true;
                else if (tok != "C420" && tok != "C420jpeg" && tok != "C420mpeg2" && tok != "C420paldv") {
                    err = "colourspace '" + tok + "' is not served (C420, C420jpeg, C420mpeg2, C420paldv, C420p10 only)"; return false;
                }
            }
            if (tok == "XCOLORRANGE=FULL") y.range = 1;
            if (tok == "XCOLORRANGE=LIMITED") y.range = 0;
            y.other.push_back(tok);
        }
    }
    (void)have_c;                                                     // no C field: 4:2:0 at 8 bits, the format's default
    if (y.w < 1 || y.h < 1) { err = "the header has no W / H field"; return false; }
    if (y.fnum < 1) { err = "the header has no F (frame rate) field"; return false; }
    if ((long long)y.w * y.h > (1ll << 27)) { err = "frame too large"; return false; }
    y.frame_bytes = ((size_t)y.w * y.h + 2 * (size_t)((y.w + 1) / 2) * ((y.h + 1) / 2)) * (y.p10 ? 2 : 1);
    const long long body = (long long)st.st_size - (long long)y.hdr_len, rec = (long long)y.frame_bytes + 6;
    y.count = body / rec;
    for (long long k = 0; k < y.count + (body % rec >= 6 ? 1 : 0); k++) {
        char m[6];
        if (pread(y.fd, m, 6, (off_t)y.hdr_len + (off_t)(k * rec)) != 6 || memcmp(m, "FRAME\n", 6) != 0) {
            err = "no plain FRAME marker where frame " + std::to_string(k) + " should start"; return false;
        }
    }
    if (body % rec) { err = "truncated: " + std::to_string(body % rec) + " stray byte(s) after the last whole frame (" + std::to_string(y.count) + " whole frames)"; return false; }
    if (y.count < 2) { err = "a video needs at least two frames"; return false; }
    return true;
}

// The one save stage that must emit in order: frames arrive from the save threads in any order and leave by output index.  The loaders keep at most `window`
// outputs in flight past the next one to be written (wait_turn), which bounds this buffer.
struct Y4mWriter {
    FILE* f = nullptr;
    std::mutex mu;
    std::condition_variable cv;
    std::map<int, std::vector<unsigned char>> pending;
    int next = 0;
    bool failed = false;
    void submit(int id, std::vector<unsigned char>&& px) {
        std::lock_guard<std::mutex> g(mu);
        if (failed) return;
        pending.emplace(id, std::move(px));
        for (auto it = pending.find(next); it != pending.end(); it = pending.find(next)) {
            if (fwrite("FRAME\n", 1, 6, f) != 6 || fwrite(it->second.data(), 1, it->second.size(), f) != it->second.size()) { failed = true; pending.clear(); break; }
            pending.erase(it);
            next++;
        }
        cv.notify_all();
    }
    void fail() { std::lock_guard<std::mutex> g(mu); failed = true; pending.clear(); cv.notify_all(); }
    bool wait_turn(int id, int window) {      // false: the run has failed, issue nothing more
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || id < next + window; });
        return !failed;
    }
};

static void print_usage() {
    fprintf(stderr, "Usage: rife-hip -0 infile -1 infile1 -o outfile [options]...\n");
    fprintf(stderr, "       rife-hip -i indir -o outdir [options]...\n");
    fprintf(stderr, "       rife-hip -i in.y4m -o out.y4m|- [-n num-frame] [-c matrix[:range]] -m rife-v4.6-model-path ...\n\n");
    fprintf(stderr, "  -h                   show this help\n");
    fprintf(stderr, "  -v                   verbose output\n");
    fprintf(stderr, "  -0 input0-path       input image0 path (jpg/png/webp/bmp/pnm)\n");
    fprintf(stderr, "  -1 input1-path       input image1 path (jpg/png/webp/bmp/pnm)\n");
    fprintf(stderr, "  -i input-path        input image directory (jpg/png/webp/bmp/pnm)\n");
    fprintf(stderr, "  -o output-path       output image path (jpg/png/webp/ppm) or directory\n");
    fprintf(stderr, "  -n num-frame         target frame count (default=N*2)\n");
    fprintf(stderr, "  -s time-step         time step (0~1, default=0.5)\n");
    fprintf(stderr, "  -m model-path        rife model path (default=rife-v2.3)\n");
    fprintf(stderr, "  -g gpu-id            gpu device to use (default=0) can be 0,1,2 for multi-gpu\n");
    fprintf(stderr, "  -j load:proc:save    thread count for load/proc/save (default=1:2:2) can be 1:2,2,2:2 for multi-gpu\n");
    fprintf(stderr, "  -x                   enable spatial tta mode\n");
    fprintf(stderr, "  -z                   enable temporal tta mode\n");
    fprintf(stderr, "  -u                   enable UHD mode\n");
    fprintf(stderr, "  -d divisor           estimate flow at 1/divisor resolution (1 or 2; rife-v4.6; for UHD material)\n");
    fprintf(stderr, "  -p precision         full (default) or fast: one f16 product per weight tap of the residual trunks (rife-v4.6; not with -x/-z)\n");
    fprintf(stderr, "  -f pattern-format    output image filename pattern format (%%08d.jpg/png/webp/ppm, default=ext/%%08d.png)\n");
    fprintf(stderr, "  -b bit-depth         bits per sample, 8, 10 or 16 (default=8); 10: rife-v4.6 only, 16-bit png / maxval-1023 ppm output;\n");
    fprintf(stderr, "                       16: rife-v4.6 only, not with -x/-z/-u; 16-bit png / maxval-65535 ppm in and out with their full samples, with -a png only\n");
    fprintf(stderr, "  -c matrix[:range]    video mode (-i in.y4m): colour description, 709 / 601 / 2020 and limited / full (default=709:limited, or the file's XCOLORRANGE);\n");
    fprintf(stderr, "                       4:2:0 YUV4MPEG2 at 8 or 10 bits, rife-v4.6 only, not with -x/-z/-u/-a/-b 10; -o - writes to stdout; -i - (stdin) is not served;\n");
    fprintf(stderr, "                       the header line must end within 256 bytes and every frame must start with a plain FRAME line (no frame parameters)\n");
    fprintf(stderr, "  -a                   keep the alpha channel (png/webp/32-bit bmp in, png/webp out); rife-v4.6 only, not with -x/-z/-u/-b 10;\n");
    fprintf(stderr, "                       with -b 16: 16-bit RGBA png out, the alpha channel at its full depth\n");
}

static bool is_dir(const std::string& p) { struct stat s; return stat(p.c_str(), &s) == 0 && S_ISDIR(s.st_mode); }

static bool list_directory(const std::string& d, std::vector<std::string>& names) {
    DIR* dir = opendir(d.c_str());
    if (!dir) return false;
    while (struct dirent* e = readdir(dir)) {
        const std::string full = d + "/" + e->d_name;
        struct stat s;
        if (stat(full.c_str(), &s) == 0 && S_ISREG(s.st_mode)) names.push_back(e->d_name);
    }
    closedir(dir);
    std::sort(names.begin(), names.end());
    return true;
}

static std::vector<int> parse_int_list(const std::string& s) {
    std::vector<int> v;
    size_t pos = 0;
    while (pos <= s.size()) {
        const size_t c = s.find(',', pos);
        const std::string tok = s.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
        v.push_back(atoi(tok.c_str()));
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    return v;
}

int main(int argc, char** argv) {
    // codec self-test without a GPU:  rife-hip --transcode in.(png|ppm) out.(png|ppm)
    if (argc == 4 && std::string(argv[1]) == "--transcode") {
        int w = 0, h = 0;
        std::vector<unsigned char> rgb;
        g_png_helpers = std::max(0, std::min(15, (int)std::thread::hardware_concurrency() - 1));
        if (!decode_image(argv[2], w, h, rgb)) { fprintf(stderr, "decode image %s failed\n", argv[2]); return 1; }
        const bool ok = encode_image(argv[3], w, h, rgb.data());
        if (!ok) { fprintf(stderr, "encode image %s failed\n", argv[3]); return 1; }
        return 0;
    }
    // the same with alpha:  rife-hip --transcode -a in.(png|webp|bmp|...) out.(png|webp)
    if (argc == 5 && std::string(argv[1]) == "--transcode" && std::string(argv[2]) == "-a") {
        int w = 0, h = 0;
        std::vector<unsigned char> rgba;
        g_png_helpers = std::max(0, std::min(15, (int)std::thread::hardware_concurrency() - 1));
        if (!decode_image_rgba(argv[3], w, h, rgba)) { fprintf(stderr, "decode image %s failed\n", argv[3]); return 1; }
        const std::string e = ext_of(argv[4]);
        if (e != "png" && e != "webp") { fprintf(stderr, "RGBA frames are written as png or webp only\n"); return 1; }
        if (!encode_image_rgba(argv[4], w, h, rgba.data())) { fprintf(stderr, "encode image %s failed\n", argv[4]); return 1; }
        return 0;
    }
    // the same for the 10-bit codecs:  rife-hip --transcode10 in.(png|ppm|...) out.(png|ppm)
    if (argc == 4 && std::string(argv[1]) == "--transcode10") {
        int w = 0, h = 0;
        std::vector<uint16_t> codes;
        g_png_helpers = std::max(0, std::min(15, (int)std::thread::hardware_concurrency() - 1));
        if (!decode_image10(argv[2], w, h, codes)) { fprintf(stderr, "decode image %s failed\n", argv[2]); return 1; }
        const std::string e = ext_of(argv[3]);
        if (e != "png" && e != "ppm") { fprintf(stderr, "10-bit frames are written as png (16-bit) or ppm (maxval 1023) only\n"); return 1; }
        if (!encode_image10(argv[3], w, h, codes.data())) { fprintf(stderr, "encode image %s failed\n", argv[3]); return 1; }
        return 0;
    }
    // the same for the 16-bit codecs:  rife-hip --transcode16 in.(png|ppm|...) out.(png|ppm), and with alpha  --transcode16a in out.png
    if (argc == 4 && (std::string(argv[1]) == "--transcode16" || std::string(argv[1]) == "--transcode16a")) {
        const int ch = std::string(argv[1]) == "--transcode16a" ? 4 : 3;
        int w = 0, h = 0;
        std::vector<uint16_t> px;
        g_png_helpers = std::max(0, std::min(15, (int)std::thread::hardware_concurrency() - 1));
        if (!decode_image16(argv[2], w, h, ch, px)) { fprintf(stderr, "decode image %s failed\n", argv[2]); return 1; }
        const std::string e = ext_of(argv[3]);
        if (e != "png" && !(e == "ppm" && ch == 3)) { fprintf(stderr, "16-bit frames are written as png or (without alpha) ppm with maxval 65535 only\n"); return 1; }
        if (!encode_image16(argv[3], w, h, ch, px.data())) { fprintf(stderr, "encode image %s failed\n", argv[3]); return 1; }
        return 0;
    }
    std::string input0, input1, inputpath, outputpath, model = "rife-v2.3", pattern_format = "%08d.png", colour, precision_arg = "full";
    int numframe = 0;
    float timestep = 0.5f;
    std::vector<int> gpuid, jobs_proc;
    int jobs_load = 1, jobs_save = 2, bits = 8, flow_divisor = 1;
    bool verbose = false, tta = false, tta_temporal = false, uhd = false, keep_alpha = false;

    int opt;
    while ((opt = getopt(argc, argv, "0:1:i:o:n:s:m:g:j:f:b:c:d:p:avxzuh")) != -1) {
        switch (opt) {
            case '0': input0 = optarg; break;
            case '1': input1 = optarg; break;
            case 'i': inputpath = optarg; break;
            case 'o': outputpath = optarg; break;
            case 'n': numframe = atoi(optarg); break;
            case 's': timestep = (float)atof(optarg); break;
            case 'm': model = optarg; break;
            case 'g': gpuid = parse_int_list(optarg); break;
            case 'j': {
                const std::string a = optarg;
                const size_t c1 = a.find(':'), c2 = a.rfind(':');
                if (c1 == std::string::npos || c1 == c2) { fprintf(stderr, "invalid thread count argument\n"); return -1; }
                jobs_load = atoi(a.substr(0, c1).c_str());
                jobs_proc = parse_int_list(a.substr(c1 + 1, c2 - c1 - 1));
                jobs_save = atoi(a.substr(c2 + 1).c_str());
                break;
            }
            case 'f': pattern_format = optarg; break;
            case 'b': bits = atoi(optarg); break;
            case 'c': colour = optarg; break;
            case 'd': flow_divisor = atoi(optarg); break;
            case 'p': precision_arg = optarg; break;
            case 'a': keep_alpha = true; break;
            case 'v': verbose = true; break;
            case 'x': tta = true; break;
            case 'z': tta_temporal = true; break;
            case 'u': uhd = true; break;
            case 'h':
            default: print_usage(); return -1;
        }
    }

    // ---- validation, in the reference's order (src/main.cpp:575-689) ----
    if (((input0.empty() || input1.empty()) && inputpath.empty()) || outputpath.empty()) { print_usage(); return -1; }
    if (inputpath.empty() && (timestep <= 0.f || timestep >= 1.f)) { fprintf(stderr, "invalid timestep argument, must be 0~1\n"); return -1; }
    if (!inputpath.empty() && numframe < 0) { fprintf(stderr, "invalid numframe argument, must not be negative\n"); return -1; }
    if (jobs_load < 1 || jobs_save < 1) { fprintf(stderr, "invalid thread count argument\n"); return -1; }
    if (!jobs_proc.empty() && jobs_proc.size() != (gpuid.empty() ? 1 : gpuid.size())) { fprintf(stderr, "invalid jobs_proc thread count argument\n"); return -1; }
    for (int j : jobs_proc) if (j < 1) { fprintf(stderr, "invalid jobs_proc thread count argument\n"); return -1; }
    if (bits != 8 && bits != 10 && bits != 16) { fprintf(stderr, "invalid bit depth argument, must be 8, 10 or 16\n"); return -1; }
    const bool deep = bits == 10, wide16 = bits == 16;
    if (flow_divisor != 1 && flow_divisor != 2) { fprintf(stderr, "invalid flow scale divisor argument (-d), must be 1 or 2\n"); return -1; }
    if (flow_divisor == 2 && (tta || tta_temporal)) {
        fprintf(stderr, "flow scale 2 (-d 2) is served in plain mode only, not with %s\n", tta ? "-x (TTA mode)" : "-z (temporal TTA mode)");
        return -1;
    }
    if (precision_arg != "full" && precision_arg != "fast") { fprintf(stderr, "invalid precision argument (-p), must be full or fast\n"); return -1; }
    const int precision = precision_arg == "fast" ? RIFE_HIP_PRECISION_FAST : RIFE_HIP_PRECISION_FULL;
    if (precision == RIFE_HIP_PRECISION_FAST && (tta || tta_temporal)) {
        fprintf(stderr, "fast precision (-p fast) is served in plain mode only, not with %s\n", tta ? "-x (TTA mode)" : "-z (temporal TTA mode)");
        return -1;
    }
    if (keep_alpha && deep) { fprintf(stderr, "alpha (-a) is served at depth 8 only, not with -b 10 (A2B10G10R10 has two alpha bits)\n"); return -1; }
    if (wide16 && (tta || tta_temporal || uhd)) {
        fprintf(stderr, "16-bit frames (-b 16) are served in plain mode only, not with %s\n", tta ? "-x (TTA mode)" : tta_temporal ? "-z (temporal TTA mode)" : "-u (UHD mode)");
        return -1;
    }
    if (keep_alpha && (tta || tta_temporal || uhd)) {
        fprintf(stderr, "alpha (-a) is served in plain mode only, not with %s\n", tta ? "-x (TTA mode)" : tta_temporal ? "-z (temporal TTA mode)" : "-u (UHD mode)");
        return -1;
    }

    // ---- video mode: -i names a regular .y4m file.  Everything that is wrong with the file or the flags ends here with a message and exit status 1 ----
    const bool video = !inputpath.empty() && !is_dir(inputpath) && ext_of(inputpath) == "y4m";
    Y4m y4m;
    Y4mWriter y4m_out;
    int yuv_pixfmt = 0;
    if (inputpath == "-") { fprintf(stderr, "reading a video from stdin (-i -) is not served: the frame count must be known\n"); return 1; }
    if (!colour.empty() && !video) { fprintf(stderr, "-c goes with video mode (-i in.y4m) only\n"); return 1; }
    if (video) {
        const char* mode = tta ? "TTA mode (-x)" : tta_temporal ? "temporal TTA mode (-z)" : uhd ? "UHD mode (-u)" : nullptr;
        if (mode) { fprintf(stderr, "4:2:0 YUV frames are served for model family rife-v4.6 in plain mode only, not for %s\n", mode); return 1; }
        if (keep_alpha || deep || wide16) {
            fprintf(stderr, "%s goes with image files, not with a .y4m video (its depth comes from the file, and it has no alpha)\n", wide16 ? "-b 16" : keep_alpha ? "-a" : "-b 10");
            return 1;
        }
        if (outputpath != "-" && (is_dir(outputpath) || ext_of(outputpath) != "y4m")) { fprintf(stderr, "a .y4m input goes to a .y4m file or to - (stdout)\n"); return 1; }
        std::string err;
        if (!y4m_open(inputpath, y4m, err)) { fprintf(stderr, "%s: %s\n", inputpath.c_str(), err.c_str()); return 1; }
        int matrix = RIFE_HIP_CSP_BT709, full = y4m.range == 1;
        if (!colour.empty()) {
            const size_t c = colour.find(':');
            const std::string m = colour.substr(0, c), r = c == std::string::npos ? "" : colour.substr(c + 1);
            if (m == "709") matrix = RIFE_HIP_CSP_BT709; else if (m == "601") matrix = RIFE_HIP_CSP_BT601; else if (m == "2020") matrix = RIFE_HIP_CSP_BT2020NCL;
            else { fprintf(stderr, "invalid colour matrix '%s', must be 709, 601 or 2020\n", m.c_str()); return 1; }
            if (r == "full") full = 1; else if (r == "limited") full = 0;
            else if (!r.empty()) { fprintf(stderr, "invalid colour range '%s', must be limited or full\n", r.c_str()); return 1; }
        }
        yuv_pixfmt = (y4m.p10 ? RIFE_HIP_PIX_I420P10 : RIFE_HIP_PIX_I420) | matrix | (full ? RIFE_HIP_CSP_FULL : 0);
        if (numframe == 0) numframe = (int)std::min<long long>(y4m.count * 2, 1 << 30);
    }

    std::string pattern = pattern_format, format;
    if (!video) {
        const size_t dot = pattern_format.rfind('.');
        if (dot != std::string::npos) { pattern = pattern_format.substr(0, dot); format = pattern_format.substr(dot + 1); }
        else { pattern = "%08d"; format = pattern_format; }
        if (pattern.empty()) pattern = "%08d";
    }
    if (!video && !is_dir(outputpath)) {
        const std::string e = ext_of(outputpath);
        if (e == "png") format = "png";
        else if (e == "ppm") format = "ppm";
        else if (e == "webp") format = "webp";
        else if (e == "jpg" || e == "jpeg") format = "jpg";
        else { fprintf(stderr, "invalid outputpath extension type\n"); return -1; }
    }
    if (!video && format != "png" && format != "ppm" && format != "webp" && format != "jpg") { fprintf(stderr, "invalid format argument\n"); return -1; }
    if (deep && format != "png" && format != "ppm") { fprintf(stderr, "10-bit frames (-b 10) are written as png (16-bit) or ppm (maxval 1023) only, not %s\n", format.c_str()); return -1; }
    if (wide16 && format != "png" && !(format == "ppm" && !keep_alpha)) {
        fprintf(stderr, "16-bit frames (-b 16) are written as png%s only, not %s%s\n", keep_alpha ? "" : " or ppm (maxval 65535)", format.c_str(), keep_alpha ? " (-a: it has no 16-bit alpha)" : "");
        return -1;
    }
    if (keep_alpha && format != "png" && format != "webp") { fprintf(stderr, "RGBA frames (-a) are written as png or webp only, %s has no alpha\n", format.c_str()); return -1; }
#ifndef RIFE_HIP_WITH_WEBP
    if (format == "webp") { fprintf(stderr, "this rife-hip was built without libwebp\n"); return -1; }
#endif

    bool rife_v2 = false, rife_v4 = false;      // family from the directory name (src/main.cpp:658-683)
    if (model.find("rife-v2") != std::string::npos || model.find("rife-v3") != std::string::npos) rife_v2 = true;
    else if (model.find("rife-v4") != std::string::npos) rife_v4 = true;
    else if (model.find("rife") == std::string::npos) { fprintf(stderr, "unknown model dir type\n"); return -1; }
    if (wide16 && !rife_v4) { fprintf(stderr, "16-bit frames (-b 16) are served for model family rife-v4.6 only, not for %s\n", model.c_str()); return -1; }
    if (keep_alpha && !rife_v4) { fprintf(stderr, "alpha (-a) is served for model family rife-v4.6 only, not for %s\n", model.c_str()); return -1; }
    if (video && !rife_v4) { fprintf(stderr, "4:2:0 YUV frames are served for model family rife-v4.6 in plain mode only, not for %s\n", model.c_str()); return 1; }
    if (flow_divisor == 2 && !rife_v4) { fprintf(stderr, "flow scale 2 (-d 2) is served for model family rife-v4.6 only, not for %s\n", model.c_str()); return -1; }
    if (precision == RIFE_HIP_PRECISION_FAST && !rife_v4) { fprintf(stderr, "fast precision (-p fast) is served for model family rife-v4.6 only, not for %s\n", model.c_str()); return -1; }
    if (!rife_v4 && (numframe != 0 || timestep != 0.5f)) { fprintf(stderr, "only rife-v4 model support custom numframe and timestep\n"); return -1; }

    // ---- task list (src/main.cpp:692-766) ----
    std::vector<Task> tasks;
    if (video) {
        for (int i = 0; i < numframe; i++) {
            int sx; float fx;
            schedule_step(i, (int)y4m.count, numframe, sx, fx);
            Task t;
            t.id = i; t.timestep = fx; t.w = y4m.w; t.h = y4m.h;
            t.in0path = "frame " + std::to_string(sx); t.in1path = "frame " + std::to_string(sx + 1);      // the cache's keys
            t.outpath = "output frame " + std::to_string(i);
            tasks.push_back(std::move(t));
        }
    } else if (!inputpath.empty() && is_dir(inputpath) && is_dir(outputpath)) {
        std::vector<std::string> names;
        if (!list_directory(inputpath, names) || names.size() < 2) return -1;
        const int count = (int)names.size();
        if (numframe == 0) numframe = count * 2;
        for (int i = 0; i < numframe; i++) {
            int sx; float fx;
            schedule_step(i, count, numframe, sx, fx);
            char name[512];
            snprintf(name, sizeof name, pattern.c_str(), i + 1);               // ffmpeg numbering starts at 1
            Task t;
            t.id = i; t.timestep = fx;
            t.in0path = inputpath + "/" + names[sx]; t.in1path = inputpath + "/" + names[sx + 1];
            t.outpath = outputpath + "/" + name + "." + format;
            tasks.push_back(std::move(t));
        }
    } else if (inputpath.empty() && !is_dir(input0) && !is_dir(input1) && !is_dir(outputpath)) {
        Task t;
        t.timestep = timestep; t.in0path = input0; t.in1path = input1; t.outpath = outputpath;
        tasks.push_back(std::move(t));
    } else {
        fprintf(stderr, "input0path, input1path and outputpath must be file at the same time\n");
        fprintf(stderr, "inputpath and outputpath must be directory at the same time\n");
        return -1;
    }

    // RIFE_HIP_CLI_TIMING=1: one summary line on stderr that separates start-up (HIP init + model load) from the pipeline
    const bool timing = getenv("RIFE_HIP_CLI_TIMING") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    // ---- devices (src/main.cpp:774-828) ----
    if (gpuid.empty()) gpuid.push_back(0);
    if (jobs_proc.empty()) jobs_proc.assign(gpuid.size(), 2);
    {   // cores the load / proc threads do not need are lent to the PNG encoders (band-parallel deflate), at most 15 helpers per save thread
        int busy = jobs_load;
        for (int j : jobs_proc) busy += j;
        const int spare = (int)std::thread::hardware_concurrency() - busy;
        g_png_helpers = std::max(0, std::min(15, spare / jobs_save - 1));
    }
    const int ndev = rife_hip_device_count();
    for (int g : gpuid) if (g < 0 || g >= ndev) { fprintf(stderr, "invalid gpu device\n"); return video ? 1 : -1; }
    std::vector<RIFE*> rife;
    for (int g : gpuid) {
        RIFE* r = new RIFE(g, tta, tta_temporal, uhd, 1, rife_v2, rife_v4);
        if (r->load(model) != 0) { fprintf(stderr, "loading %s failed: %s\n", model.c_str(), rife_hip_last_error()); return video ? 1 : -1; }
        // rife-v4 (4.0) shares the directory prefix: the engine knows the family, and refuses before the first pair
        if (flow_divisor != 1 && r->set_flow_scale(flow_divisor) != 0) { fprintf(stderr, "flow scale %d (-d) is not available: %s\n", flow_divisor, rife_hip_last_error()); return video ? 1 : -1; }
        if (precision != RIFE_HIP_PRECISION_FULL && r->set_precision(precision) != 0) { fprintf(stderr, "fast precision (-p fast) is not available: %s\n", rife_hip_last_error()); return video ? 1 : -1; }
        if (video) {      // rife-v4 (4.0) shares the directory prefix, and the engine knows which colour descriptions it serves: ask it now, with one pixel
            const uint16_t one[3] = {0, 0, 0};
            rife_hip_frame* f = r->upload_yuv(one, 1, 1, yuv_pixfmt);
            if (!f) { fprintf(stderr, "video mode is not available: %s\n", rife_hip_last_error()); return 1; }
            RIFE::release(f);
        }
        if (deep) {      // the engine refuses 10-bit frames for every family but rife-v4.6 and for -x / -z / -u: ask it now, with one pixel, not at the first pair
            uint16_t one[3] = {0, 0, 0};
            rife_hip_frame* f = r->upload(ncnn::Mat(1, 1, (void*)one, (size_t)6, 3));
            if (!f) { fprintf(stderr, "-b 10 is not available: %s\n", rife_hip_last_error()); return -1; }
            RIFE::release(f);
        }
        if (wide16) {      // likewise, through the call the proc threads make: one pixel at timestep 0 reaches the engine's scope check and copies one sample
            uint16_t one[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
            rife_hip_packed_t d[3];
            for (int i = 0; i < 3; i++) { d[i].w = d[i].h = 1; d[i].channels = keep_alpha ? 4 : 3; d[i].depth = 16; d[i].data = one[i]; d[i].pitch = 8; }
            if (r->process_hbd_packed(d[0], d[1], 0.f, d[2]) != 0) { fprintf(stderr, "-b 16 is not available: %s\n", rife_hip_last_error()); return -1; }
        } else if (keep_alpha) {      // likewise: rife-v4 (4.0) shares the directory prefix and is told apart by the engine
            unsigned char one[4] = {0, 0, 0, 0};
            rife_hip_frame* f = r->upload(ncnn::Mat(1, 1, (void*)one, (size_t)4, 4));
            if (!f) { fprintf(stderr, "-a is not available: %s\n", rife_hip_last_error()); return -1; }
            RIFE::release(f);
        }
        rife.push_back(r);
    }

    if (video) {      // the output header: the input's, with the frame rate times numframe / count as a reduced fraction
        y4m_out.f = outputpath == "-" ? stdout : fopen(outputpath.c_str(), "wb");
        if (!y4m_out.f) { fprintf(stderr, "cannot write %s\n", outputpath.c_str()); return 1; }
        long long num = y4m.fnum * numframe, den = y4m.fden * y4m.count, a = num, b = den;
        while (b) { const long long t = a % b; a = b; b = t; }
        std::string hdr = "YUV4MPEG2 W" + std::to_string(y4m.w) + " H" + std::to_string(y4m.h) + " F" + std::to_string(num / a) + ":" + std::to_string(den / a);
        for (const std::string& tok : y4m.other) hdr += " " + tok;
        hdr += "\n";
        if (fwrite(hdr.data(), 1, hdr.size(), y4m_out.f) != hdr.size()) { fprintf(stderr, "cannot write %s\n", outputpath.c_str()); return 1; }
    }
    const auto tp1 = std::chrono::steady_clock::now();
    // ---- load -> proc -> save (src/main.cpp:309-436, 830-904) ----
    TaskQueue toproc, tosave;
    FrameCache cache;
    std::mutex next_mu;
    size_t next_task = 0;
    auto load = [&]() {
        for (;;) {
            size_t k;
            { std::lock_guard<std::mutex> g(next_mu); if (next_task >= tasks.size()) return; k = next_task++; }
            Task t = std::move(tasks[k]);
            FrameCache::Frame f0, f1;
            if (video && !y4m_out.wait_turn(t.id, 32)) return;                  // at most 32 outputs past the next one to be written: bounds the writer's reorder buffer
            auto decode = [&](const std::string& p, SharedFrame& fr) {
                if (video) {
                    fr.w = y4m.w; fr.h = y4m.h; fr.yuv = yuv_pixfmt;
                    return y4m.read_frame(atoll(p.c_str() + 6), fr.px);         // "frame <k>"
                }
                if (wide16) return decode_image16(p, fr.w, fr.h, keep_alpha ? 4 : 3, fr.px16);
                fr.rgba = keep_alpha;
                return deep ? decode_image10(p, fr.w, fr.h, fr.px10) : keep_alpha ? decode_image_rgba(p, fr.w, fr.h, fr.px) : decode_image(p, fr.w, fr.h, fr.px);
            };
            if (!cache.get(t.in0path, f0, decode) || !cache.get(t.in1path, f1, decode)) {
                fprintf(stderr, "decode image %s or %s failed\n", t.in0path.c_str(), t.in1path.c_str());
                if (video) { y4m_out.fail(); return; }                          // a video with a hole is no output
                continue;
            }
            if (f1->w != f0->w || f1->h != f0->h) { fprintf(stderr, "%s and %s differ in size\n", t.in0path.c_str(), t.in1path.c_str()); continue; }
            t.w = f0->w; t.h = f0->h; t.fr0 = f0; t.fr1 = f1;
            toproc.put(std::move(t));
        }
    };
    std::vector<std::atomic<int>> replica_tasks(rife.size());               // tasks every replica took off the shared queue (timing line; tests/test_cli.py)
    for (auto& n : replica_tasks) n = 0;
    auto proc = [&](RIFE* r) {
        size_t me = 0;
        while (me < rife.size() && rife[me] != r) me++;
        for (;;) {
            Task t = toproc.get();
            if (t.id == -233) return;                                          // end marker, like the reference
            replica_tasks[me]++;
            if (video) {                                                       // timestep 0 / 1 too: the engine returns the frame's samples as codes, the rule lives there
                const rife_hip_frame* d0 = t.fr0->on(r);
                const rife_hip_frame* d1 = t.fr1->on(r);
                t.out.resize(y4m.frame_bytes);
                ncnn::Mat out(t.w, t.h, (void*)t.out.data(), (size_t)1, 1);    // process() writes one frame of the resident frames' format behind .data
                if (!d0 || !d1 || r->process(d0, d1, t.timestep, out) != 0) { fprintf(stderr, "process %s failed: %s\n", t.outpath.c_str(), rife_hip_last_error()); y4m_out.fail(); continue; }
            }
            else if (wide16 && (t.timestep == 0.f || t.timestep == 1.f)) t.out16 = (t.timestep == 0.f ? t.fr0 : t.fr1)->px16;      // the input's samples
            else if (wide16) {      // host frames, never resident: the engine stages them and blends the samples themselves
                const int nch = keep_alpha ? 4 : 3;
                t.out16.resize((size_t)t.w * t.h * nch);
                rife_hip_packed_t d[3];
                void* const data[3] = {(void*)t.fr0->px16.data(), (void*)t.fr1->px16.data(), (void*)t.out16.data()};
                for (int i = 0; i < 3; i++) { d[i].w = t.w; d[i].h = t.h; d[i].channels = nch; d[i].depth = 16; d[i].data = data[i]; d[i].pitch = (ptrdiff_t)t.w * nch * 2; }
                if (r->process_hbd_packed(d[0], d[1], t.timestep, d[2]) != 0) { fprintf(stderr, "process %s failed: %s\n", t.outpath.c_str(), rife_hip_last_error()); continue; }
            }
            else if (deep && (t.timestep == 0.f || t.timestep == 1.f)) t.out10 = (t.timestep == 0.f ? t.fr0 : t.fr1)->px10;
            else if (t.timestep == 0.f || t.timestep == 1.f) t.out = (t.timestep == 0.f ? t.fr0 : t.fr1)->px;      // rife.cpp:2470-2480: an input frame, unchanged
            else if (deep) {
                const rife_hip_frame* d0 = t.fr0->on(r);
                const rife_hip_frame* d1 = t.fr1->on(r);
                t.out10.resize((size_t)t.w * t.h * 3);
                ncnn::Mat out(t.w, t.h, (void*)t.out10.data(), (size_t)6, 3);
                if (!d0 || !d1 || r->process(d0, d1, t.timestep, out) != 0) { fprintf(stderr, "process %s failed: %s\n", t.outpath.c_str(), rife_hip_last_error()); continue; }
            } else {
                const rife_hip_frame* d0 = t.fr0->on(r);
                const rife_hip_frame* d1 = t.fr1->on(r);
                const int nch = keep_alpha ? 4 : 3;
                t.out.resize((size_t)t.w * t.h * nch);
                ncnn::Mat out(t.w, t.h, (void*)t.out.data(), (size_t)nch, nch);
                if (!d0 || !d1 || r->process(d0, d1, t.timestep, out) != 0) { fprintf(stderr, "process %s failed: %s\n", t.outpath.c_str(), rife_hip_last_error()); continue; }
            }
            t.fr0.reset(); t.fr1.reset();                                      // the save stage needs only the output
            tosave.put(std::move(t));
        }
    };
    auto save = [&]() {
        for (;;) {
            Task t = tosave.get();
            if (t.id == -233) return;
            if (video) {
                y4m_out.submit(t.id, std::move(t.out));
                if (verbose) fprintf(stderr, "%s %s %f -> %s done\n", t.in0path.c_str(), t.in1path.c_str(), t.timestep, t.outpath.c_str());
                continue;
            }
            const bool ok = wide16 ? encode_image16(t.outpath, t.w, t.h, keep_alpha ? 4 : 3, t.out16.data()) : deep ? encode_image10(t.outpath, t.w, t.h, t.out10.data()) : keep_alpha ? encode_image_rgba(t.outpath, t.w, t.h, t.out.data())
                                                                                              : encode_image(t.outpath, t.w, t.h, t.out.data());
            if (!ok) fprintf(stderr, "encode image %s failed\n", t.outpath.c_str());
            else if (verbose) fprintf(stderr, "%s %s %f -> %s done\n", t.in0path.c_str(), t.in1path.c_str(), t.timestep, t.outpath.c_str());
        }
    };
    std::vector<std::thread> loaders, procs, savers;
    for (int i = 0; i < jobs_load; i++) loaders.emplace_back(load);
    for (size_t d = 0; d < gpuid.size(); d++) for (int i = 0; i < jobs_proc[d]; i++) procs.emplace_back(proc, rife[d]);
    for (int i = 0; i < jobs_save; i++) savers.emplace_back(save);
    for (auto& t : loaders) t.join();
    for (size_t i = 0; i < procs.size(); i++) { Task e; e.id = -233; toproc.put(std::move(e)); }
    for (auto& t : procs) t.join();
    for (size_t i = 0; i < savers.size(); i++) { Task e; e.id = -233; tosave.put(std::move(e)); }
    for (auto& t : savers) t.join();
    if (timing) {
        const auto tp2 = std::chrono::steady_clock::now();
        const double a = std::chrono::duration<double>(tp1 - tp0).count(), b = std::chrono::duration<double>(tp2 - tp1).count();
        fprintf(stderr, "timing: devices + model load %.3f s, pipeline %.3f s for %zu frames = %.1f frames/s\n", a, b, tasks.size(), tasks.size() / b);
        for (size_t d = 0; d < rife.size(); d++) fprintf(stderr, "timing: replica %zu (gpu %d) took %d task(s)\n", d, gpuid[d], replica_tasks[d].load());
    }
    cache.clear();                                                             // resident frames go before their engines
    for (RIFE* r : rife) delete r;
    if (video) {
        const bool flushed = fflush(y4m_out.f) == 0;
        if (y4m_out.f != stdout) fclose(y4m_out.f);
        if (y4m_out.failed || !flushed || y4m_out.next != numframe) { fprintf(stderr, "%s is incomplete: %d of %d frames written\n", outputpath.c_str(), y4m_out.next, numframe); return 1; }
    }
    return 0;
}
