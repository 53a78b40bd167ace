// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (tools/sanitize_run.sh, built with ASan + UBSan): csrc/image_check.h - the host-only rules
// behind rife_hip_image_check / rife_hip_image_row_bytes - walked over one refusing descriptor per rule and one accepting descriptor per format and size.
// Exit status 0 and a last line "image_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/image_check.h"

static int g_cases = 0, g_wrong = 0;
static void expect(const rife_hip_image_t& im, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_img::check(&im, err);
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}

int main() {
    static const int FMT[8] = {RIFE_HIP_PIX_RGB8, RIFE_HIP_PIX_RGB10_U16, RIFE_HIP_PIX_A2B10G10R10, RIFE_HIP_PIX_RGBA8, RIFE_HIP_PIX_NV12, RIFE_HIP_PIX_I420, RIFE_HIP_PIX_P010, RIFE_HIP_PIX_I420P10};
    static const int SZ[2][2] = {{1, 1}, {33, 47}};
    for (int f : FMT) for (auto& sz : SZ) {
        const int w = sz[0], h = sz[1];
        std::vector<std::vector<unsigned char>> mem(3);
        rife_hip_image_t im;
        std::memset(&im, 0, sizeof im);
        im.w = w; im.h = h; im.pixfmt = f | (f >= RIFE_HIP_PIX_NV12 ? RIFE_HIP_CSP_BT601 : 0);
        for (int p = 0; p < rife_img::planes(f); p++) {
            const size_t rb = rife_img::row_bytes(w, f, p);
            im.pitch[p] = (ptrdiff_t)((rb + 63) / 64 * 64);
            mem[p].assign((size_t)im.pitch[p] * rife_img::plane_rows(h, p) + 8, 0x5a);
            im.plane[p] = mem[p].data() + ((8 - reinterpret_cast<uintptr_t>(mem[p].data()) % 8) % 8);      // element-aligned whatever the allocator returned
            for (int y = 0; y < rife_img::plane_rows(h, p); y++) std::memset(static_cast<unsigned char*>(im.plane[p]) + (size_t)y * im.pitch[p], y, rb);      // every row is inside its buffer
        }
        expect(im, true, "", "accept");
        expect(im, rife_img::planes(f) > 0, "", "accept again");
        const int es = rife_img::elem_size(f), last = rife_img::planes(f) - 1;
        rife_hip_image_t b = im; b.plane[last] = nullptr; expect(b, false, "NULL", "NULL plane");
        b = im; b.pitch[last] = (ptrdiff_t)rife_img::row_bytes(w, f, last) - 1; expect(b, false, b.pitch[last] > 0 ? "smaller than the row bytes" : "zero", "pitch under the row bytes");
        b = im; b.pitch[0] = -im.pitch[0]; expect(b, false, "negative", "negative pitch");
        b = im; b.pitch[0] = (ptrdiff_t)INT32_MAX + 1; expect(b, false, "INT32_MAX", "pitch above INT32_MAX");
        if (es > 1) {
            b = im; b.pitch[0] = im.pitch[0] + es - 1 + 64; expect(b, false, "multiple of the element size", "pitch off the element size");
            b = im; b.plane[0] = static_cast<unsigned char*>(im.plane[0]) + 1; expect(b, false, "not aligned", "pointer off the element size");
        }
        b = im; b.w = 0; expect(b, false, "bad frame size", "w = 0");
        b = im; b.h = -3; expect(b, false, "bad frame size", "h < 0");
    }
    rife_hip_image_t im;
    std::memset(&im, 0, sizeof im);
    unsigned char px[64] = {0};
    im.w = im.h = 1; im.plane[0] = im.plane[1] = im.plane[2] = px; im.pitch[0] = im.pitch[1] = im.pitch[2] = 16;
    for (int f : {3, 5, 7, 20, -1, 0x2000}) { im.pixfmt = f; expect(im, false, "unknown pixel format", "unknown format"); }
    im.pixfmt = RIFE_HIP_PIX_RGB8 | RIFE_HIP_CSP_BT601; expect(im, false, "colour description", "colour bits on an RGB format");
    im.pixfmt = RIFE_HIP_PIX_P010 | RIFE_HIP_CSP_FULL; expect(im, false, "full-range", "CSP_FULL at 10 bits");
    im.pixfmt = RIFE_HIP_PIX_NV12 | (3 << 8); expect(im, false, "unknown colour matrix", "unknown matrix");
    { std::string e; g_cases++; if (!rife_img::check(nullptr, e)) { g_wrong++; std::printf("WRONG: a null descriptor passed\n"); } }
    for (int f : FMT) for (int w : {1, 2, 3, 33}) for (int p = 0; p < 4; p++) {
        g_cases++;
        const size_t cw = (size_t)(w + 1) / 2, es = (size_t)rife_img::elem_size(f);
        const size_t want = f == RIFE_HIP_PIX_RGB8 ? (p ? 0 : 3 * w) : f == RIFE_HIP_PIX_RGB10_U16 ? (p ? 0 : 6 * w) : f < RIFE_HIP_PIX_NV12 ? (p ? 0 : 4 * w)
                            : p == 0 ? w * es : (f == RIFE_HIP_PIX_NV12 || f == RIFE_HIP_PIX_P010) ? (p == 1 ? 2 * cw * es : 0) : (p < 3 ? cw * es : 0);
        if (rife_img::row_bytes(w, f, p) != want) { g_wrong++; std::printf("WRONG row_bytes(%d, %d, %d) = %zu, wanted %zu\n", w, f, p, rife_img::row_bytes(w, f, p), want); }
    }
    std::printf("image_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
