// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (built with ASan + UBSan, nothing preloaded): csrc/packed_check.h - the host-only rules behind
// rife_hip_packed_check and the argument checks of the two packed calls - walked over accepting images per channel count, depth, size and row padding and one refusing
// image per rule; every accepted output image is then written row by row the way a call fills it, and every accepted input read the way the blend reads it, so a rule
// that let a short image through would show as an out-of-bounds access.  The one-plane view of the timestep 0 / 1 copy (as_plane) is checked against the image.
// Exit status 0 and a last line "packed_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/packed_check.h"

static int g_cases = 0, g_wrong = 0;
static void tally(int rc, const std::string& err, bool ok, const char* needle, const char* what) {
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}
static void expect(const rife_hip_packed_t* im, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_packed::check(im, err);
    tally(rc, err, ok, needle, what);
}
static void expect_call(const rife_hip_packed_t* a, const rife_hip_packed_t* b, const rife_hip_packed_t* o, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_packed::check_call(a, b, o, err);
    tally(rc, err, ok, needle, what);
}
static void truth(bool ok, const char* what) {
    g_cases++;
    if (!ok) { g_wrong++; std::printf("WRONG %s\n", what); }
}

struct Image {
    std::vector<unsigned char> mem;
    rife_hip_packed_t d;
    Image(int w, int h, int ch, int depth, size_t pad) {
        std::memset(&d, 0, sizeof d);
        d.w = w; d.h = h; d.channels = ch; d.depth = depth;
        const size_t pitch = (size_t)w * ch * 2 + pad;
        mem.assign(pitch * (size_t)(h - 1) + (size_t)w * ch * 2 + 2, 0x5a);      // the last row ends with its last sample: no padding behind it
        d.data = mem.data() + (reinterpret_cast<uintptr_t>(mem.data()) & 1);
        d.pitch = (ptrdiff_t)pitch;
    }
};

int main() {
    static const int SZ[8][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 5}, {17, 9}, {64, 32}, {100, 60}, {258, 130}};
    for (int ch = 3; ch <= 4; ch++) for (auto& sz : SZ) for (int depth = 10; depth <= 16; depth++) {
        const int w = sz[0], h = sz[1];
        Image a(w, h, ch, depth, 0), b(w, h, ch, depth, 48), o(w, h, ch, depth, 6);
        expect(&a.d, true, "", "accept tight");
        expect(&b.d, true, "", "accept padded");
        expect(&o.d, true, "", "accept odd padding");
        expect_call(&a.d, &b.d, &o.d, true, "", "accept call");
        // what a call does with accepted images: every sample of both inputs read, every sample of the output written, nothing else
        const unsigned maxval = (1u << depth) - 1u;
        unsigned long long sum = 0;
        for (int y = 0; y < h; y++) {
            const uint16_t* r0 = reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(a.d.data) + (size_t)y * a.d.pitch);
            const uint16_t* r1 = reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(b.d.data) + (size_t)y * b.d.pitch);
            uint16_t* ro = reinterpret_cast<uint16_t*>(static_cast<unsigned char*>(o.d.data) + (size_t)y * o.d.pitch);
            for (int x = 0; x < w * ch; x++) { sum += r0[x] + r1[x]; ro[x] = (uint16_t)(r0[x] < maxval ? r0[x] : maxval); }
        }
        truth(sum == 2ull * 0x5a5a * (unsigned long long)w * h * ch, "the samples read are the image's");
        const rife_hip_planes_t pl = rife_packed::as_plane(o.d);
        truth(pl.w == w * ch && pl.h == h && pl.n == 1 && pl.sample == RIFE_HIP_SAMPLE_U16 && pl.maxval == (int)maxval && pl.plane[0] == o.d.data && pl.pitch[0] == o.d.pitch,
              "as_plane is the image as one plane of w * channels samples");
        // one refusing image per rule
        { rife_hip_packed_t r = a.d; r.w = 0; expect(&r, false, "bad image size", "w 0"); }
        { rife_hip_packed_t r = a.d; r.h = -1; expect(&r, false, "bad image size", "h -1"); }
        for (int c : {0, 1, 2, 5, -3}) { rife_hip_packed_t r = a.d; r.channels = c; expect(&r, false, "is not 3 (R G B) or 4 (R G B A)", "channels"); }
        for (int dp : {9, 17, 0, 8, -1}) { rife_hip_packed_t r = a.d; r.depth = dp; expect(&r, false, "is not in 10..16", "depth"); }
        { rife_hip_packed_t r = a.d; r.data = nullptr; expect(&r, false, "null data pointer", "null data"); }
        { rife_hip_packed_t r = a.d; r.data = static_cast<unsigned char*>(r.data) + 1; expect(&r, false, "the data pointer is not aligned to 2 bytes", "odd pointer"); }
        { rife_hip_packed_t r = a.d; r.pitch = 0; expect(&r, false, "the pitch is not positive", "pitch 0"); }
        { rife_hip_packed_t r = a.d; r.pitch = -r.pitch; expect(&r, false, "the pitch is not positive", "negative pitch"); }
        { rife_hip_packed_t r = a.d; r.pitch -= 2; expect(&r, false, r.pitch > 0 ? "the pitch is smaller than a row" : "the pitch is not positive", "short pitch"); }
        { rife_hip_packed_t r = b.d; r.pitch += 1; expect(&r, false, "the pitch is not a multiple of 2 bytes", "odd pitch"); }
        { rife_hip_packed_t r = a.d; r.pitch = (ptrdiff_t)INT32_MAX + 1; expect(&r, false, "the pitch exceeds INT32_MAX", "huge pitch"); }      // only the descriptor is read
        { rife_hip_packed_t r = a.d; r.w = 1 << 14; r.h = (1 << 13) + 1; r.pitch = (ptrdiff_t)r.w * ch * 2; expect(&r, false, "more than 2^27 pixels", "too many pixels"); }
        { rife_hip_packed_t r = a.d; r.w = 1; r.h = 1 << 20; r.pitch = 4096; expect(&r, false, "rows * pitch reaches 2^32 bytes", "rows * pitch"); }
        expect(nullptr, false, "null descriptor", "null descriptor");
        // the three images of a call
        expect_call(nullptr, &b.d, &o.d, false, "image 0: null descriptor", "call null 0");
        expect_call(&a.d, nullptr, &o.d, false, "image 1: null descriptor", "call null 1");
        expect_call(&a.d, &b.d, nullptr, false, "image out: null descriptor", "call null out");
        { rife_hip_packed_t r = b.d; r.depth = 9; expect_call(&a.d, &r, &o.d, false, "image 1: the depth (9)", "call depth"); }
        { rife_hip_packed_t r = o.d; r.data = nullptr; expect_call(&a.d, &b.d, &r, false, "image out: null data pointer", "call null data"); }
        { Image c2(w + 1, h, ch, depth, 0); expect_call(&a.d, &c2.d, &o.d, false, "image 0 and image 1 differ in size", "call size 1"); }
        { Image c2(w, h + 1, ch, depth, 0); expect_call(&a.d, &b.d, &c2.d, false, "image 0 and image out differ in size", "call size out"); }
        { Image c2(w, h, 7 - ch, depth, 0); expect_call(&a.d, &c2.d, &o.d, false, "image 0 and image 1 differ in channels", "call channels"); }
        { Image c2(w, h, ch, depth == 16 ? 10 : depth + 1, 0); expect_call(&a.d, &b.d, &c2.d, false, "image 0 and image out differ in depth", "call depth out"); }
    }
    // the limits themselves: 2^27 pixels and rows * pitch one short of 2^32 pass (only the descriptor is read)
    {
        static uint16_t one[4];
        rife_hip_packed_t r;
        std::memset(&r, 0, sizeof r);
        r.channels = 3; r.depth = 16; r.data = one;
        r.w = 1 << 14; r.h = 1 << 13; r.pitch = (ptrdiff_t)r.w * 6; expect(&r, true, "", "2^27 pixels");
        r.w = 1; r.h = 1 << 20; r.pitch = 4094; expect(&r, true, "", "rows * pitch below 2^32");
        r.pitch = 4096; expect(&r, false, "rows * pitch reaches 2^32 bytes", "rows * pitch at 2^32");
        r.h = 1; r.pitch = INT32_MAX - 1; expect(&r, true, "", "pitch INT32_MAX - 1");
    }
    std::printf("packed_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
