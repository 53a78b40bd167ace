// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (built with ASan + UBSan, nothing preloaded): csrc/hbd_check.h - the host-only rules behind
// rife_hip_hbd_check and the argument checks of the two hbd calls - walked over accepting images per layout, depth, size and row padding and one refusing image per
// rule; the sets every accepted call stands for are built (make_sets), passed through the rules of the sets calls, and every output plane is then written row by row
// the way a call fills it, so a rule that let a short plane through would show as an out-of-bounds write.  The proxy reduction is walked over every sample value.
// Exit status 0 and a last line "hbd_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/hbd_check.h"

static int g_cases = 0, g_wrong = 0;
static void tally(int rc, const std::string& err, bool ok, const char* needle, const char* what) {
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}
static void expect(const rife_hip_image_t* im, int depth, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_hbd::check(im, depth, err);
    tally(rc, err, ok, needle, what);
}
static void expect_call(const rife_hip_image_t* a, const rife_hip_image_t* b, const rife_hip_image_t* o, int depth, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_hbd::check_call(a, b, o, depth, err);
    tally(rc, err, ok, needle, what);
}
static void truth(bool ok, const char* what) {
    g_cases++;
    if (!ok) { g_wrong++; std::printf("WRONG %s\n", what); }
}

struct Image {
    std::vector<unsigned char> mem[3];
    rife_hip_image_t d;
    Image(int w, int h, int pixfmt, size_t pad) {
        std::memset(&d, 0, sizeof d);
        d.w = w; d.h = h; d.pixfmt = pixfmt;
        for (int p = 0; p < 3; p++) {
            const size_t pitch = rife_img::row_bytes(w, pixfmt, p) + pad;
            mem[p].assign(pitch * (size_t)rife_img::plane_rows(h, pixfmt, p) + 2, 0x5a);
            d.plane[p] = mem[p].data() + (reinterpret_cast<uintptr_t>(mem[p].data()) & 1);
            d.pitch[p] = (ptrdiff_t)pitch;
        }
    }
};

int main() {
    static const int FMT[4] = {RIFE_HIP_PIX_I420P10, RIFE_HIP_PIX_I422P10, RIFE_HIP_PIX_I444P10, RIFE_HIP_PIX_RGBP10};
    static const int SZ[7][2] = {{1, 1}, {2, 2}, {3, 5}, {17, 9}, {64, 32}, {100, 60}, {258, 130}};
    for (int fi = 0; fi < 4; fi++) for (auto& sz : SZ) for (int depth = 10; depth <= 16; depth++) {
        const int fmt = FMT[fi], w = sz[0], h = sz[1];
        const int px = fmt == RIFE_HIP_PIX_RGBP10 ? fmt : fmt | ((depth & 1) ? RIFE_HIP_CSP_BT2020NCL : RIFE_HIP_CSP_BT709);
        Image a(w, h, px, 0), b(w, h, px, 48), o(w, h, px, 16);
        expect(&a.d, depth, true, "", "accept tight");
        expect(&b.d, depth, true, "", "accept padded");
        expect_call(&a.d, &b.d, &o.d, depth, true, "", "accept call");
        // the sets of the definition pass the rules of the sets calls, and the output planes hold what a call writes
        rife_hbd::Sets S;
        rife_hbd::make_sets(S, a.d, b.d, o.d, depth);
        std::string err;
        const int src = rife_apply::check_sets(S.n, S.sets, w, h, err);
        tally(src, err, true, "", "the sets of an accepted call");
        const int cls = rife_img::yuv_class(px);
        truth(S.n == ((cls == 1 || cls == 2) ? 2 : 1), "set count");
        truth(S.sets[0].shift_x == 0 && S.sets[0].shift_y == 0 && S.sets[0].wp == 0 && S.sets[0].hp == 0, "set 0 shift and extent");
        if (S.n == 2) truth(S.sets[1].shift_x == -1 && S.sets[1].shift_y == (cls == 1 ? -1 : 0) && S.sets[1].out->n == 2 && S.sets[0].out->n == 1, "set 1 shift");
        int planes = 0;
        for (int k = 0; k < S.n; k++) {
            const rife_hip_planes_t& d = *S.sets[k].out;
            truth(d.maxval == (1 << depth) - 1 && d.sample == RIFE_HIP_SAMPLE_U16, "maxval and sample");
            for (int q = 0; q < d.n; q++, planes++)
                for (int y = 0; y < d.h; y++) std::memset(static_cast<unsigned char*>(d.plane[q]) + (size_t)y * d.pitch[q], y, rife_apply::row_bytes(d.w, d.sample));
        }
        truth(planes == 3, "three planes in the sets");
        // depth
        expect(&a.d, 9, false, "the depth (9) is not in 10..16", "depth 9");
        expect(&a.d, 17, false, "the depth (17) is not in 10..16", "depth 17");
        expect(&a.d, 0, false, "the depth (0)", "depth 0");
        // the layout
        static const int BAD[9] = {RIFE_HIP_PIX_RGB8, RIFE_HIP_PIX_RGB10_U16, RIFE_HIP_PIX_A2B10G10R10, RIFE_HIP_PIX_I420, RIFE_HIP_PIX_P010, RIFE_HIP_PIX_I422, RIFE_HIP_PIX_I444,
                                   RIFE_HIP_PIX_RGBP8, RIFE_HIP_PIX_RGBPF};
        for (int bf : BAD) {
            Image x(w, h, bf, 0);
            const std::string want = "pixel format " + std::to_string(bf) + " is not a high-bit-depth layout";
            expect(&x.d, depth, false, want.c_str(), "another format");
        }
        rife_hip_image_t c = a.d;
        c.pixfmt = 52; expect(&c, depth, false, "unknown pixel format", "unknown format");
        if (fmt != RIFE_HIP_PIX_RGBP10) { c = a.d; c.pixfmt = fmt | RIFE_HIP_CSP_FULL; expect(&c, depth, false, "full-range YUV is served at 8 bits only", "full range"); }
        else { c = a.d; c.pixfmt = fmt | RIFE_HIP_CSP_BT601; expect(&c, depth, false, "a colour description", "colour bits on RGB"); }
        // the rules of the image
        c = a.d; c.plane[2] = nullptr; expect(&c, depth, false, "plane 2 is NULL", "null plane");
        c = a.d; c.pitch[1] = 0; expect(&c, depth, false, "plane 1: the pitch is zero", "zero pitch");
        c = a.d; c.pitch[0] = -c.pitch[0]; expect(&c, depth, false, "plane 0: the pitch is negative", "negative pitch");
        c = b.d; c.pitch[0] = 2 * w - 2; if (w > 1) expect(&c, depth, false, "plane 0: the pitch (", "short pitch");
        c = b.d; c.pitch[1] += 1; expect(&c, depth, false, "plane 1: the pitch is not a multiple of the element size (2)", "odd pitch");
        c = b.d; c.plane[0] = static_cast<unsigned char*>(c.plane[0]) + 1; expect(&c, depth, false, "plane 0: the pointer is not aligned", "odd pointer");
        c = a.d; c.w = 0; expect(&c, depth, false, "bad frame size", "w = 0");
        expect(nullptr, depth, false, "null image descriptor", "null image");
        // the three images of a call
        expect_call(nullptr, &b.d, &o.d, depth, false, "image 0: null image descriptor", "null image 0");
        expect_call(&a.d, &b.d, nullptr, depth, false, "image out: null image descriptor", "null image out");
        c = b.d; c.pitch[2] = 0; expect_call(&a.d, &c, &o.d, depth, false, "image 1: plane 2: the pitch is zero", "bad image 1");
        Image other(w + 1, h, px, 0);
        expect_call(&a.d, &b.d, &other.d, depth, false, "the images of one call differ in size", "size differs");
        Image fo(w, h, FMT[(fi + 1) % 4], 0);
        expect_call(&a.d, &fo.d, &o.d, depth, false, "the images of one call differ in pixel format", "format differs");
        expect_call(&a.d, &b.d, &o.d, 20, false, "image 0: the depth (20)", "depth of a call");
    }
    // sizes the sets calls would refuse
    {
        Image a(4, 4, RIFE_HIP_PIX_I444P10, 0);
        rife_hip_image_t c = a.d; c.h = 1 << 20; c.pitch[0] = c.pitch[1] = c.pitch[2] = 4096;
        expect(&c, 12, false, "rows * pitch reaches 2^32 bytes", "2^32 bytes");      // only the descriptor is read
        c = a.d; c.w = 1 << 14; c.h = (1 << 13) + 1; c.pitch[0] = c.pitch[1] = c.pitch[2] = 1 << 15;
        expect(&c, 12, false, "image too large", "2^27 pixels");
    }
    // the proxy reduction: the identity on c << (depth - 10), monotone, saturating, and the definition spelled out
    for (int depth = 10; depth <= 16; depth++) {
        bool ident = true, mono = true, def = true;
        for (unsigned c10 = 0; c10 < 1024; c10++) ident = ident && rife_hbd::reduce10(c10 << (depth - 10), depth) == c10;
        unsigned prev = 0;
        for (unsigned v = 0; v < 65536; v++) {
            const unsigned c10 = rife_hbd::reduce10(v, depth);
            mono = mono && c10 >= prev && c10 <= 1023;
            prev = c10;
            const unsigned long long want = depth > 10 ? ((unsigned long long)v + (1ull << (depth - 11))) >> (depth - 10) : v;
            def = def && c10 == (want < 1023 ? (unsigned)want : 1023u);
        }
        truth(ident, "reduce10 is the identity on shifted codes");
        truth(mono, "reduce10 is monotone and at most 1023");
        truth(def, "reduce10 is the definition");
        truth(rife_hbd::reduce10(65535, depth) == 1023 && rife_hbd::reduce10((1u << depth) - 1, depth) == 1023, "reduce10 saturates");
    }
    std::printf("hbd_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
