// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (built with ASan + UBSan, nothing preloaded): csrc/semiplanar_check.h - the host-only rules behind
// rife_hip_semiplanar_check and the argument checks of the two semi-planar calls - walked over accepting images per chroma mode, depth, size and row padding and one
// refusing image per rule; every accepted output image is then written row by row the way the timestep 0 / 1 copy fills it, and every accepted input read the way the
// kernels read it (h rows of w luma samples, ch rows of 2 * cw chroma samples), so a rule that let a short image through would show as an out-of-bounds access.
// Exit status 0 and a last line "semiplanar_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/semiplanar_check.h"

static int g_cases = 0, g_wrong = 0;
static void tally(int rc, const std::string& err, bool ok, const char* needle, const char* what) {
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}
static void expect(const rife_hip_semiplanar_t* im, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_sp::check(im, err);
    tally(rc, err, ok, needle, what);
}
static void expect_call(const rife_hip_semiplanar_t* a, const rife_hip_semiplanar_t* b, const rife_hip_semiplanar_t* o, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_sp::check_call(a, b, o, err);
    tally(rc, err, ok, needle, what);
}
static void truth(bool ok, const char* what) {
    g_cases++;
    if (!ok) { g_wrong++; std::printf("WRONG %s\n", what); }
}

struct Image {
    std::vector<unsigned char> my, mc;
    rife_hip_semiplanar_t d;
    Image(int w, int h, int chroma, int depth, size_t pad, int csp = RIFE_HIP_CSP_BT709) {
        std::memset(&d, 0, sizeof d);
        d.w = w; d.h = h; d.chroma = chroma; d.depth = depth; d.csp = csp;
        const int cw = (w + 1) / 2, ch = chroma == 1 ? (h + 1) / 2 : h;
        const size_t py = (size_t)w * 2 + pad, pc = (size_t)cw * 4 + pad;
        my.assign(py * (size_t)(h - 1) + (size_t)w * 2 + 2, 0x5a);            // the last row ends with its last sample: no padding behind it
        mc.assign(pc * (size_t)(ch - 1) + (size_t)cw * 4 + 2, 0x5a);
        d.y = my.data() + (reinterpret_cast<uintptr_t>(my.data()) & 1);
        d.cbcr = mc.data() + (reinterpret_cast<uintptr_t>(mc.data()) & 1);
        d.pitch_y = (ptrdiff_t)py; d.pitch_c = (ptrdiff_t)pc;
    }
};

int main() {
    static const int SZ[8][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 5}, {17, 9}, {64, 32}, {100, 60}, {258, 130}};
    static const int CSP[3] = {RIFE_HIP_CSP_BT709, RIFE_HIP_CSP_BT601, RIFE_HIP_CSP_BT2020NCL};
    for (int chroma = 1; chroma <= 2; chroma++) for (auto& sz : SZ) for (int depth = 10; depth <= 16; depth++) {
        const int w = sz[0], h = sz[1], cw = (w + 1) / 2, ch = chroma == 1 ? (h + 1) / 2 : h, csp = CSP[depth % 3];
        Image a(w, h, chroma, depth, 0, csp), b(w, h, chroma, depth, 48, csp), o(w, h, chroma, depth, 6, csp);
        expect(&a.d, true, "", "accept tight");
        expect(&b.d, true, "", "accept padded");
        expect(&o.d, true, "", "accept odd padding");
        expect_call(&a.d, &b.d, &o.d, true, "", "accept call");
        truth(rife_sp::chroma_w(w) == cw && rife_sp::chroma_h(h, chroma) == ch, "the chroma size");
        truth(rife_sp::planar_pixfmt(chroma, csp) == ((chroma == 1 ? RIFE_HIP_PIX_I420P10 : RIFE_HIP_PIX_I422P10) | csp), "the planar layout of the definition");
        // what a call does with accepted images: every sample of both inputs read, every sample of the output written, nothing else
        const int sh = 16 - depth;
        unsigned long long sum = 0;
        for (int p = 0; p < 2; p++) {
            const int n = p ? 2 * cw : w, rows = p ? ch : h;
            for (int y = 0; y < rows; y++) {
                const uint16_t* r0 = reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(p ? a.d.cbcr : a.d.y) + (size_t)y * (p ? a.d.pitch_c : a.d.pitch_y));
                const uint16_t* r1 = reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(p ? b.d.cbcr : b.d.y) + (size_t)y * (p ? b.d.pitch_c : b.d.pitch_y));
                uint16_t* ro = reinterpret_cast<uint16_t*>(static_cast<unsigned char*>(p ? o.d.cbcr : o.d.y) + (size_t)y * (p ? o.d.pitch_c : o.d.pitch_y));
                for (int x = 0; x < n; x++) { sum += r0[x] + r1[x]; ro[x] = (uint16_t)((r0[x] >> sh) << sh); }
            }
        }
        truth(sum == 2ull * 0x5a5a * ((unsigned long long)w * h + 2ull * cw * ch), "the samples read are the image's");
        // one refusing image per rule
        { rife_hip_semiplanar_t r = a.d; r.w = 0; expect(&r, false, "bad image size", "w 0"); }
        { rife_hip_semiplanar_t r = a.d; r.h = -1; expect(&r, false, "bad image size", "h -1"); }
        { rife_hip_semiplanar_t r = a.d; r.chroma = 3; expect(&r, false, "4:4:4 semi-planar (P410 / P416) is not served", "chroma 3"); }
        for (int c : {0, 4, -1, 16}) { rife_hip_semiplanar_t r = a.d; r.chroma = c; expect(&r, false, "is not 1 (4:2:0) or 2 (4:2:2)", "chroma"); }
        { rife_hip_semiplanar_t r = a.d; r.csp |= RIFE_HIP_CSP_FULL; expect(&r, false, "RIFE_HIP_CSP_FULL", "full range"); }
        for (int c : {3 << 8, 1, 1 << 13, 4 << 8, 16}) { rife_hip_semiplanar_t r = a.d; r.csp = c; expect(&r, false, "is not RIFE_HIP_CSP_BT709, _BT601 or _BT2020NCL", "csp"); }
        for (int dp : {9, 17, 0, 8, -1}) { rife_hip_semiplanar_t r = a.d; r.depth = dp; expect(&r, false, "is not in 10..16", "depth"); }
        { rife_hip_semiplanar_t r = a.d; r.y = nullptr; expect(&r, false, "null y pointer", "null y"); }
        { rife_hip_semiplanar_t r = a.d; r.cbcr = nullptr; expect(&r, false, "null cbcr pointer", "null cbcr"); }
        { rife_hip_semiplanar_t r = a.d; r.y = static_cast<unsigned char*>(r.y) + 1; expect(&r, false, "the y pointer is not aligned to 2 bytes", "odd y"); }
        { rife_hip_semiplanar_t r = a.d; r.cbcr = static_cast<unsigned char*>(r.cbcr) + 1; expect(&r, false, "the cbcr pointer is not aligned to 2 bytes", "odd cbcr"); }
        { rife_hip_semiplanar_t r = a.d; r.pitch_y = 0; expect(&r, false, "the y pitch is not positive", "pitch_y 0"); }
        { rife_hip_semiplanar_t r = a.d; r.pitch_c = -r.pitch_c; expect(&r, false, "the cbcr pitch is not positive", "negative pitch_c"); }
        { rife_hip_semiplanar_t r = a.d; r.pitch_y -= 2; expect(&r, false, r.pitch_y > 0 ? "the y pitch is smaller than a row of w * 2 bytes" : "the y pitch is not positive", "short pitch_y"); }
        { rife_hip_semiplanar_t r = a.d; r.pitch_c -= 2; expect(&r, false, "the cbcr pitch is smaller than a row of ((w + 1) / 2) * 4 bytes", "short pitch_c"); }
        { rife_hip_semiplanar_t r = b.d; r.pitch_y += 1; expect(&r, false, "the y pitch is not a multiple of 2 bytes", "odd pitch_y"); }
        { rife_hip_semiplanar_t r = b.d; r.pitch_c += 1; expect(&r, false, "the cbcr pitch is not a multiple of 2 bytes", "odd pitch_c"); }
        { rife_hip_semiplanar_t r = a.d; r.pitch_y = (ptrdiff_t)INT32_MAX + 1; expect(&r, false, "the y pitch exceeds INT32_MAX", "huge pitch_y"); }      // only the descriptor is read
        { rife_hip_semiplanar_t r = a.d; r.pitch_c = (ptrdiff_t)INT32_MAX + 1; expect(&r, false, "the cbcr pitch exceeds INT32_MAX", "huge pitch_c"); }
        { rife_hip_semiplanar_t r = a.d; r.w = 1 << 14; r.h = (1 << 13) + 1; r.pitch_y = r.pitch_c = (ptrdiff_t)r.w * 2; expect(&r, false, "more than 2^27 pixels", "too many pixels"); }
        { rife_hip_semiplanar_t r = a.d; r.w = 1; r.h = 1 << 20; r.pitch_y = 4096; r.pitch_c = 4; expect(&r, false, "the y plane: rows * pitch reaches 2^32 bytes", "rows * pitch_y"); }
        { rife_hip_semiplanar_t r = a.d; r.w = 1; r.h = 1 << 21; r.pitch_y = 2; r.pitch_c = 4096; expect(&r, false, "the cbcr plane: rows * pitch reaches 2^32 bytes", "rows * pitch_c"); }
        expect(nullptr, false, "null descriptor", "null descriptor");
        // the three images of a call
        expect_call(nullptr, &b.d, &o.d, false, "image 0: null descriptor", "call null 0");
        expect_call(&a.d, nullptr, &o.d, false, "image 1: null descriptor", "call null 1");
        expect_call(&a.d, &b.d, nullptr, false, "image out: null descriptor", "call null out");
        { rife_hip_semiplanar_t r = b.d; r.depth = 9; expect_call(&a.d, &r, &o.d, false, "image 1: the depth (9)", "call depth"); }
        { rife_hip_semiplanar_t r = o.d; r.cbcr = nullptr; expect_call(&a.d, &b.d, &r, false, "image out: null cbcr pointer", "call null cbcr"); }
        { Image c2(w + 1, h, chroma, depth, 0, csp); expect_call(&a.d, &c2.d, &o.d, false, "image 0 and image 1 differ in size", "call size 1"); }
        { Image c2(w, h + 1, chroma, depth, 0, csp); expect_call(&a.d, &b.d, &c2.d, false, "image 0 and image out differ in size", "call size out"); }
        { Image c2(w, h, 3 - chroma, depth, 0, csp); expect_call(&a.d, &c2.d, &o.d, false, "image 0 and image 1 differ in chroma", "call chroma"); }
        { Image c2(w, h, chroma, depth, 0, CSP[(depth + 1) % 3]); expect_call(&a.d, &b.d, &c2.d, false, "image 0 and image out differ in csp", "call csp"); }
        { Image c2(w, h, chroma, depth == 16 ? 10 : depth + 1, 0, csp); expect_call(&a.d, &b.d, &c2.d, false, "image 0 and image out differ in depth", "call depth out"); }
    }
    // the limits themselves: 2^27 pixels and rows * pitch one short of 2^32 pass (only the descriptor is read)
    {
        static uint16_t one[4];
        rife_hip_semiplanar_t r;
        std::memset(&r, 0, sizeof r);
        r.chroma = 2; r.depth = 16; r.y = one; r.cbcr = one;
        r.w = 1 << 14; r.h = 1 << 13; r.pitch_y = r.pitch_c = (ptrdiff_t)r.w * 2; expect(&r, true, "", "2^27 pixels");
        r.w = 1; r.h = 1 << 20; r.pitch_y = 4094; r.pitch_c = 4092; expect(&r, true, "", "rows * pitch below 2^32");
        r.pitch_c = 4096; expect(&r, false, "the cbcr plane: rows * pitch reaches 2^32 bytes", "rows * pitch_c at 2^32");
        r.chroma = 1; expect(&r, true, "", "half the chroma rows at 4:2:0");
        r.h = 1; r.pitch_y = INT32_MAX - 1; r.pitch_c = INT32_MAX - 1; expect(&r, true, "", "pitch INT32_MAX - 1");
    }
    std::printf("semiplanar_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
