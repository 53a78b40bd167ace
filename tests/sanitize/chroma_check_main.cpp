// TEST INFRASTRUCTURE ONLY.  A program of its own, built with ASan + UBSan (csrc/Makefile, target ../chroma-check-asan): csrc/image_check.h over the 4:2:2 / 4:4:4
// formats (RIFE_HIP_PIX_I422 / I422P10 / I444 / I444P10) - check, row_bytes, the plane rows by format and is_tight, on descriptors whose every row is touched
// inside buffers of exactly the size the rules promise, so that a wrong row count or row size is a heap overflow the sanitizer sees.
// Exit status 0 and a last line "chroma_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/image_check.h"

static int g_cases = 0, g_wrong = 0;
static void want(bool cond, const char* what, int f, int w, int h) {
    g_cases++;
    if (!cond) { g_wrong++; std::printf("WRONG %s (format %d, %dx%d)\n", what, f, w, h); }
}
static void expect(const rife_hip_image_t& im, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_img::check(&im, err);
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}

int main() {
    static const int FMT[4] = {RIFE_HIP_PIX_I422, RIFE_HIP_PIX_I422P10, RIFE_HIP_PIX_I444, RIFE_HIP_PIX_I444P10};
    static const int SZ[5][2] = {{1, 1}, {2, 1}, {3, 5}, {33, 47}, {64, 34}};
    for (int f : FMT) for (auto& sz : SZ) {
        const int w = sz[0], h = sz[1];
        const bool p10 = (f & 2) != 0, c444 = (f >> 4) == 3;
        const size_t es = p10 ? 2 : 1, cw = c444 ? (size_t)w : ((size_t)w + 1) / 2;
        want(rife_img::is_yuv(f) && rife_img::known(f | RIFE_HIP_CSP_BT2020NCL) && rife_img::planes(f) == 3 && rife_img::elem_size(f) == (int)es, "format properties", f, w, h);
        for (int p = 0; p < 4; p++) want(rife_img::row_bytes(w, f, p) == (p == 0 ? w * es : p < 3 ? cw * es : 0), "row_bytes", f, w, h);
        for (int p = 0; p < 3; p++) want(rife_img::plane_rows(h, f, p) == h, "plane rows", f, w, h);
        want(rife_img::plane_rows(h, RIFE_HIP_PIX_I420, 1) == (h + 1) / 2 && rife_img::plane_rows(h, 1) == (h + 1) / 2 && rife_img::plane_rows(h, RIFE_HIP_PIX_RGB8, 0) == h, "plane rows of the other formats", f, w, h);
        // a tight frame in ONE buffer of exactly (w * h + 2 * cw * h) samples: is_tight accepts it, and every row the rules name lies inside it
        const size_t nbytes = ((size_t)w * h + 2 * cw * h) * es;
        std::vector<unsigned char> tight(nbytes, 0x5a);
        rife_hip_image_t im;
        std::memset(&im, 0, sizeof im);
        im.w = w; im.h = h; im.pixfmt = f | RIFE_HIP_CSP_BT601;
        size_t at = 0;
        for (int p = 0; p < 3; p++) {
            im.plane[p] = tight.data() + at; im.pitch[p] = (ptrdiff_t)rife_img::row_bytes(w, f, p);
            for (int y = 0; y < rife_img::plane_rows(h, f, p); y++) std::memset(static_cast<unsigned char*>(im.plane[p]) + (size_t)y * im.pitch[p], y, rife_img::row_bytes(w, f, p));
            at += (size_t)im.pitch[p] * rife_img::plane_rows(h, f, p);
        }
        want(at == nbytes, "the planes add up to the frame", f, w, h);
        expect(im, true, "", "accept tight");
        want(rife_img::is_tight(&im), "is_tight on a tight frame", f, w, h);
        if (h > 1) {      // the 4:2:0 offsets are NOT tight for these formats
            rife_hip_image_t b = im; b.plane[2] = static_cast<unsigned char*>(im.plane[1]) + (size_t)im.pitch[1] * ((h + 1) / 2);
            want(!rife_img::is_tight(&b), "is_tight on 4:2:0 plane offsets", f, w, h);
        }
        // pitched planes in buffers of their own, exactly rows * pitch bytes each
        std::vector<std::vector<unsigned char>> mem(3);
        rife_hip_image_t q = im;
        for (int p = 0; p < 3; p++) {
            const size_t rb = rife_img::row_bytes(w, f, p);
            q.pitch[p] = (ptrdiff_t)((rb + 63) / 64 * 64);
            mem[p].assign((size_t)q.pitch[p] * rife_img::plane_rows(h, f, p), 0x5a);
            q.plane[p] = mem[p].data();
            for (int y = 0; y < rife_img::plane_rows(h, f, p); y++) std::memset(mem[p].data() + (size_t)y * q.pitch[p], y, rb);
        }
        expect(q, true, "", "accept pitched");
        want(!rife_img::is_tight(&q), "is_tight on pitched planes", f, w, h);
        rife_hip_image_t b = q; b.plane[2] = nullptr; expect(b, false, "plane 2 is NULL", "NULL third plane");
        b = q; b.pitch[1] = (ptrdiff_t)rife_img::row_bytes(w, f, 1) - (ptrdiff_t)es; expect(b, false, b.pitch[1] > 0 ? "smaller than the row bytes" : "zero", "short chroma pitch");
        b = q; b.pitch[0] = (ptrdiff_t)rife_img::row_bytes(w, f, 0) - (ptrdiff_t)es; expect(b, false, b.pitch[0] > 0 ? "smaller than the row bytes" : "zero", "short luma pitch");
        b = q; b.pitch[2] = -q.pitch[2]; expect(b, false, "negative", "negative pitch");
        if (p10) {
            b = q; b.pitch[1] = q.pitch[1] + 65; expect(b, false, "multiple of the element size (2)", "odd pitch at 10 bits");
            b = q; b.plane[2] = mem[2].data() + 1; expect(b, false, "not aligned to the element size (2)", "odd pointer at 10 bits");
            b = q; b.pixfmt = f | RIFE_HIP_CSP_FULL; expect(b, false, "full-range", "CSP_FULL at 10 bits");
        } else {
            b = q; b.pixfmt = f | RIFE_HIP_CSP_FULL | RIFE_HIP_CSP_BT2020NCL; expect(b, true, "", "CSP_FULL at 8 bits");
        }
        b = q; b.pixfmt = f | (3 << 8); expect(b, false, "unknown colour matrix", "colour matrix 3");
        b = q; b.pixfmt = f | (1 << 13); expect(b, false, "unknown pixel format", "a bit above the colour description");
        std::string e;
        b = q; b.pixfmt = f; want(rife_img::check_same(&q, &b, e) == 1 && e.find("differ") != std::string::npos, "check_same on two colour descriptions", f, w, h);
    }
    rife_hip_image_t im;
    std::memset(&im, 0, sizeof im);
    unsigned char px[64] = {0};
    im.w = im.h = 1; im.plane[0] = im.plane[1] = im.plane[2] = px; im.pitch[0] = im.pitch[1] = im.pitch[2] = 16;
    for (int f : {20, 21, 31, 32, 34, 36, 48, 50, 52, 53, 64, 65, 255}) {
        im.pixfmt = f; expect(im, false, "unknown pixel format", "unknown format");
        want(rife_img::planes(f) == 0 && rife_img::row_bytes(33, f, 0) == 0 && !rife_img::is_yuv(f), "an unknown format has no planes", f, 1, 1);
    }
    std::printf("chroma_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
