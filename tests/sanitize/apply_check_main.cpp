// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (built with ASan + UBSan, nothing preloaded): csrc/apply_check.h - the host-only rules behind
// rife_hip_planes_check and the argument checks of the apply calls - walked over one refusing descriptor per rule and accepting descriptors per sample type, plane
// count, size and padding; every accepted output set is then written row by row the way an apply call fills it, so a rule that let a short plane through would show
// as an out-of-bounds write.  Exit status 0 and a last line "apply_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/apply_check.h"

static int g_cases = 0, g_wrong = 0;
static void tally(int rc, const std::string& err, bool ok, const char* needle, const char* what) {
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}
static void expect(const rife_hip_planes_t* p, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_apply::check(p, err);
    tally(rc, err, ok, needle, what);
}
static void expect_call(const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_planes_t* out, const rife_hip_motion_t* m, bool with_motion, int wp, int hp,
                        bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_apply::check_call(p0, p1, out, m, with_motion, wp, hp, err);
    tally(rc, err, ok, needle, what);
}
static unsigned char* align16(std::vector<unsigned char>& v) { return v.data() + ((16 - reinterpret_cast<uintptr_t>(v.data()) % 16) % 16); }

struct Set {
    std::vector<unsigned char> mem[4];
    rife_hip_planes_t d;
    Set(int w, int h, int n, int sample, size_t pad) {
        std::memset(&d, 0, sizeof d);
        d.w = w; d.h = h; d.n = n; d.sample = sample; d.maxval = rife_apply::integer(sample) ? rife_apply::maxval_limit(sample) : 0;
        const size_t pitch = rife_apply::row_bytes(w, sample) + pad;
        for (int k = 0; k < n; k++) { mem[k].assign(pitch * h + 16, 0x5a); d.plane[k] = align16(mem[k]); d.pitch[k] = (ptrdiff_t)pitch; }
    }
};

int main() {
    static const int SMP[4] = {RIFE_HIP_SAMPLE_U8, RIFE_HIP_SAMPLE_U16, RIFE_HIP_SAMPLE_F16, RIFE_HIP_SAMPLE_F32};
    static const int SZ[3][2] = {{1, 1}, {33, 47}, {100, 60}};
    static const size_t PAD[2] = {0, 48};
    for (int s : SMP) for (auto& sz : SZ) for (size_t pad : PAD) for (int n = 1; n <= 4; n++) {
        const int w = sz[0], h = sz[1];
        const size_t es = rife_apply::sample_bytes(s), row = rife_apply::row_bytes(w, s);
        Set a(w, h, n, s, pad), b2(w, h, n, s, pad), o(w, h, n, s, pad);
        const rife_hip_planes_t& g = a.d;
        expect(&g, true, "", "accept");
        for (int k = 0; k < n; k++) for (int y = 0; y < h; y++) std::memset(static_cast<unsigned char*>(o.d.plane[k]) + (size_t)y * o.d.pitch[k], y, row);      // what a call writes
        rife_hip_planes_t b = g; b.w = 0; expect(&b, false, "bad plane size", "w = 0");
        b = g; b.h = -2; expect(&b, false, "bad plane size", "h < 0");
        b = g; b.n = 0; expect(&b, false, "is not in 1..4", "n = 0");
        b = g; b.n = 5; expect(&b, false, "is not in 1..4", "n = 5");
        b = g; b.sample = 4; expect(&b, false, "unknown sample type", "sample 4");
        b = g; b.sample = -1; expect(&b, false, "unknown sample type", "sample -1");
        if (rife_apply::integer(s)) {
            b = g; b.maxval = 0; expect(&b, false, "maxval (0) is not in 1..", "maxval 0");
            b = g; b.maxval = rife_apply::maxval_limit(s) + 1; expect(&b, false, "is not in 1..", "maxval over the type");
            b = g; b.maxval = 1; expect(&b, true, "", "maxval 1");
        } else {
            b = g; b.maxval = 255; expect(&b, false, "maxval must be 0 for float samples", "maxval on floats");
        }
        b = g; b.plane[n - 1] = nullptr; expect(&b, false, "null pointer", "null plane");
        b = g; b.pitch[n - 1] = 0; expect(&b, false, "the pitch is not positive", "pitch 0");
        b = g; b.pitch[0] = -(ptrdiff_t)(row + pad); expect(&b, false, "the pitch is not positive", "negative pitch");
        if (w > 1) { b = g; b.pitch[0] = (ptrdiff_t)(row - es); expect(&b, false, "is smaller than the row bytes", "pitch under the row bytes"); }
        if (es > 1) {
            b = g; b.pitch[n - 1] = (ptrdiff_t)(row + pad + 1); expect(&b, false, "the pitch is not a multiple of the element size", "pitch off the element");
            b = g; b.plane[0] = static_cast<unsigned char*>(g.plane[0]) + 1; expect(&b, false, "the pointer is not aligned to the element size", "pointer off the element");
        }
        b = g; b.pitch[0] = (ptrdiff_t)(((1ull << 32) / (size_t)h + es) / es * es); expect(&b, false, "h * pitch reaches 2^32", "a plane of 4 GB");
        b = g; b.pitch[0] = (ptrdiff_t)(((1ull << 32) - 1) / (size_t)h / es * es);
        if ((size_t)b.pitch[0] >= row) expect(&b, true, "", "a plane just under 4 GB");
        // the whole call
        const size_t frow = rife_motion::flow_row_bytes(w, RIFE_HIP_MOTION_F32), mrow = rife_motion::mask_row_bytes(w, RIFE_HIP_MOTION_F32);
        std::vector<unsigned char> fmem(frow * h + 16), mmem(mrow * h + 16);
        rife_hip_motion_t m;
        m.flow = align16(fmem); m.flow_pitch = frow; m.mask = align16(mmem); m.mask_pitch = mrow; m.format = RIFE_HIP_MOTION_F32;
        expect_call(&a.d, &b2.d, &o.d, &m, true, 0, 0, true, "", "call accept");
        expect_call(&a.d, &b2.d, &o.d, &m, true, w, h, true, "", "extent w, h");
        expect_call(&a.d, &b2.d, &o.d, &m, true, (w + 63) / 64 * 64, (h + 63) / 64 * 64, true, "", "extent padded");
        expect_call(&a.d, &b2.d, &o.d, nullptr, false, 0, 0, true, "", "call without motion");
        expect_call(&a.d, &b2.d, &o.d, &m, true, w - 1, h, false, "the extent", "extent under w");
        expect_call(&a.d, &b2.d, &o.d, &m, true, w, 0, false, "the extent", "extent w, 0");
        expect_call(&a.d, &b2.d, &o.d, &m, true, 1 << 14, (1 << 13) + 1, false, "the extent is too large", "extent over 2^27");
        expect_call(nullptr, &b2.d, &o.d, &m, true, 0, 0, false, "planes 0: null planes descriptor", "null planes 0");
        expect_call(&a.d, nullptr, &o.d, &m, true, 0, 0, false, "planes 1: null planes descriptor", "null planes 1");
        expect_call(&a.d, &b2.d, nullptr, &m, true, 0, 0, false, "planes out: null planes descriptor", "null planes out");
        expect_call(&a.d, &b2.d, &o.d, nullptr, true, 0, 0, false, "motion: null motion descriptor", "null motion");
        rife_hip_motion_t mb = m; mb.mask = nullptr; expect_call(&a.d, &b2.d, &o.d, &mb, true, 0, 0, false, "needs both flow and mask", "mask missing");
        mb = m; mb.flow = nullptr; expect_call(&a.d, &b2.d, &o.d, &mb, true, 0, 0, false, "needs both flow and mask", "flow missing");
        mb = m; mb.flow_pitch = 8; if (w > 0) expect_call(&a.d, &b2.d, &o.d, &mb, true, 0, 0, false, "motion: flow: the pitch", "motion pitch");
        rife_hip_planes_t c = b2.d; c.n = n == 4 ? 3 : n + 1;
        if (c.n <= n) expect_call(&a.d, &c, &o.d, &m, true, 0, 0, false, "the three plane sets differ", "n differs");
        if (rife_apply::integer(s)) { c = o.d; c.maxval = 1; expect_call(&a.d, &b2.d, &c, &m, true, 0, 0, false, "the three plane sets differ", "maxval differs"); }
        c = b2.d; c.sample = (s + 1) % 4; c.maxval = rife_apply::integer(c.sample) ? 1 : 0;
        if (rife_apply::sample_bytes(c.sample) <= es) expect_call(&a.d, &c, &o.d, &m, true, 0, 0, false, "the three plane sets differ", "sample differs");
        if (h > 1) { c = o.d; c.h = h - 1; expect_call(&a.d, &b2.d, &c, &m, true, 0, 0, false, "the three plane sets differ", "h differs"); }
    }
    expect(nullptr, false, "null planes descriptor", "null descriptor");
    std::printf("apply_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
