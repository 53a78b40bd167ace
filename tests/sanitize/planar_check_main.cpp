// TEST INFRASTRUCTURE ONLY.  A program of its own, built with ASan + UBSan (csrc/Makefile, target ../planar-check-asan; tests/test_planar_host.py builds and runs
// it too): csrc/image_check.h over the planar RGB formats (RIFE_HIP_PIX_RGBP8 / RGBP10 / RGBPH / RGBPF) - check, row_bytes, element size, plane rows and
// is_tight, on descriptors whose every row is touched inside buffers of exactly the size the rules promise, so that a wrong row count or row size is a heap
// overflow the sanitizer sees.
// Exit status 0 and a last line "planar_check: N cases, 0 wrong" when every answer is the expected one.
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
    static const int FMT[4] = {RIFE_HIP_PIX_RGBP8, RIFE_HIP_PIX_RGBP10, RIFE_HIP_PIX_RGBPH, RIFE_HIP_PIX_RGBPF};
    static const size_t ES[4] = {1, 2, 2, 4};
    static const int SZ[5][2] = {{1, 1}, {2, 1}, {3, 5}, {33, 47}, {64, 34}};
    for (int k = 0; k < 4; k++) for (auto& sz : SZ) {
        const int f = FMT[k], w = sz[0], h = sz[1];
        const size_t es = ES[k];
        want(f == 16 * 4 + 2 * k + 1, "the format number", f, w, h);
        want(rife_img::is_rgbp(f) && !rife_img::is_yuv(f) && rife_img::known(f) && rife_img::planes(f) == 3 && rife_img::elem_size(f) == (int)es, "format properties", f, w, h);
        for (int p = 0; p < 4; p++) want(rife_img::row_bytes(w, f, p) == (p < 3 ? w * es : 0), "row_bytes", f, w, h);
        for (int p = 0; p < 3; p++) want(rife_img::plane_rows(h, f, p) == h, "plane rows", f, w, h);
        // a tight frame in ONE buffer of exactly 3 * w * h samples: is_tight accepts it, and every row the rules name lies inside it
        const size_t nbytes = (size_t)3 * w * h * es;
        unsigned char* tight = new unsigned char[nbytes];      // operator new: aligned for every element size
        rife_hip_image_t im;
        std::memset(&im, 0, sizeof im);
        im.w = w; im.h = h; im.pixfmt = f;
        size_t at = 0;
        for (int p = 0; p < 3; p++) {
            im.plane[p] = tight + at; im.pitch[p] = (ptrdiff_t)rife_img::row_bytes(w, f, p);
            for (int y = 0; y < rife_img::plane_rows(h, f, p); y++) std::memset(static_cast<unsigned char*>(im.plane[p]) + (size_t)y * im.pitch[p], y, rife_img::row_bytes(w, f, p));
            at += (size_t)im.pitch[p] * rife_img::plane_rows(h, f, p);
        }
        want(at == nbytes, "the planes add up to the frame", f, w, h);
        expect(im, true, "", "accept tight");
        want(rife_img::is_tight(&im), "is_tight on a tight frame", f, w, h);
        {      // planes permuted G, B, R (ffmpeg's gbrp): accepted, and not the tight frame
            rife_hip_image_t b = im; b.plane[0] = im.plane[1]; b.plane[1] = im.plane[2]; b.plane[2] = im.plane[0];
            expect(b, true, "", "accept permuted planes");
            want(!rife_img::is_tight(&b), "is_tight on permuted planes", f, w, h);
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
        for (int p = 0; p < 3; p++) {
            const std::string pl = "plane " + std::to_string(p);
            rife_hip_image_t b = q; b.plane[p] = nullptr; expect(b, false, (pl + " is NULL").c_str(), "NULL plane");
            b = q; b.pitch[p] = (ptrdiff_t)rife_img::row_bytes(w, f, p) - (ptrdiff_t)es; expect(b, false, b.pitch[p] > 0 ? "smaller than the row bytes" : "zero", "short pitch");
            b = q; b.pitch[p] = -q.pitch[p]; expect(b, false, "negative", "negative pitch");
            const std::string esz = "element size (" + std::to_string(es) + ")";
            if (es > 1) {
                b = q; b.pitch[p] = q.pitch[p] + 64 + 1; expect(b, false, ("multiple of the " + esz).c_str(), "odd pitch");
                b = q; b.plane[p] = mem[p].data() + 1; expect(b, false, ("not aligned to the " + esz).c_str(), "odd pointer");
            } else {
                b = q; b.pitch[p] = q.pitch[p] + 1; expect(b, true, "", "any pitch at u8");
            }
            if (es == 4) {
                b = q; b.pitch[p] = q.pitch[p] + 64 + 2; expect(b, false, ("multiple of the " + esz).c_str(), "pitch of half a float");
                b = q; b.plane[p] = mem[p].data() + 2; expect(b, false, ("not aligned to the " + esz).c_str(), "pointer half a float in");
            }
        }
        rife_hip_image_t b = q; b.pixfmt = f | RIFE_HIP_CSP_BT601; expect(b, false, "colour description", "a colour matrix on planar RGB");
        b = q; b.pixfmt = f | RIFE_HIP_CSP_FULL; expect(b, false, "colour description", "CSP_FULL on planar RGB");
        b = q; b.pixfmt = f | (1 << 13); expect(b, false, "unknown pixel format", "a bit above the colour description");
        std::string e;
        b = q; b.pixfmt = FMT[(k + 1) & 3]; want(rife_img::check_same(&q, &b, e) == 1 && e.find("differ") != std::string::npos, "check_same on two planar formats", f, w, h);
        delete[] tight;
    }
    rife_hip_image_t im;
    std::memset(&im, 0, sizeof im);
    alignas(16) unsigned char px[64] = {0};
    im.w = im.h = 1; im.plane[0] = im.plane[1] = im.plane[2] = px; im.pitch[0] = im.pitch[1] = im.pitch[2] = 16;
    for (int f : {64, 66, 68, 70, 72, 73, 80, 81, 255}) {
        im.pixfmt = f; expect(im, false, "unknown pixel format", "unknown format");
        want(rife_img::planes(f) == 0 && rife_img::row_bytes(33, f, 0) == 0 && !rife_img::is_rgbp(f) && !rife_img::known(f), "an unknown format has no planes", f, 1, 1);
    }
    std::printf("planar_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
