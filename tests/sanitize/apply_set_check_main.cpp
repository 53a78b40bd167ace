// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (built with ASan + UBSan, nothing preloaded): csrc/apply_set_check.h - the host-only rules behind
// rife_hip_apply_set_check and the per-set argument checks of the sets calls - walked over accepting sets per sample type, shift pair and motion size (both plane
// sizes of the up shift) and one refusing set per rule; every accepted output set is then written row by row the way a call fills it, so a rule that let a short
// plane through would show as an out-of-bounds write.  Exit status 0 and a last line "apply_set_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/apply_set_check.h"

static int g_cases = 0, g_wrong = 0;
static void tally(int rc, const std::string& err, bool ok, const char* needle, const char* what) {
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}
static void expect(const rife_hip_apply_set_t* s, int mw, int mh, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_apply::check_set(s, mw, mh, err);
    tally(rc, err, ok, needle, what);
}
static void expect_sets(int n, const rife_hip_apply_set_t* s, int mw, int mh, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_apply::check_sets(n, s, mw, mh, err);
    tally(rc, err, ok, needle, what);
}
static unsigned char* align16(std::vector<unsigned char>& v) { return v.data() + ((16 - reinterpret_cast<uintptr_t>(v.data()) % 16) % 16); }

struct Planes {
    std::vector<unsigned char> mem[4];
    rife_hip_planes_t d;
    Planes(int w, int h, int n, int sample, size_t pad) {
        std::memset(&d, 0, sizeof d);
        d.w = w; d.h = h; d.n = n; d.sample = sample; d.maxval = rife_apply::integer(sample) ? rife_apply::maxval_limit(sample) : 0;
        const size_t pitch = rife_apply::row_bytes(w, sample) + pad;
        for (int k = 0; k < n; k++) { mem[k].assign(pitch * h + 16, 0x5a); d.plane[k] = align16(mem[k]); d.pitch[k] = (ptrdiff_t)pitch; }
    }
};
static rife_hip_apply_set_t make(const Planes& a, const Planes& b, const Planes& o, int sx, int sy, int wp, int hp) {
    rife_hip_apply_set_t s;
    s.p0 = &a.d; s.p1 = &b.d; s.out = &o.d; s.shift_x = sx; s.shift_y = sy; s.wp = wp; s.hp = hp;
    return s;
}

int main() {
    static const int SMP[4] = {RIFE_HIP_SAMPLE_U8, RIFE_HIP_SAMPLE_U16, RIFE_HIP_SAMPLE_F16, RIFE_HIP_SAMPLE_F32};
    static const int MSZ[6][2] = {{1, 1}, {2, 2}, {3, 3}, {33, 47}, {100, 60}, {257, 130}};
    static const int SH[4][2] = {{0, 0}, {-1, -1}, {-1, 0}, {1, 1}};
    for (int smp : SMP) for (auto& ms : MSZ) for (auto& sh : SH) for (int alt = 0; alt < 2; alt++) {
        const int mw = ms[0], mh = ms[1], sx = sh[0], sy = sh[1];
        if (alt && sx != 1) continue;      // the up shift takes 2 m and 2 m - 1
        const int w = sx == 0 ? mw : sx < 0 ? (mw + 1) / 2 : 2 * mw - alt, h = sy == 0 ? mh : sy < 0 ? (mh + 1) / 2 : 2 * mh - alt;
        const int n = 1 + (mw + smp) % 4;
        const size_t row = rife_apply::row_bytes(w, smp);
        Planes a(w, h, n, smp, 0), b(w, h, n, smp, 48), o(w, h, n, smp, 16);
        rife_hip_apply_set_t g = make(a, b, o, sx, sy, 0, 0);
        expect(&g, mw, mh, true, "", "accept");
        for (int k = 0; k < n; k++) for (int y = 0; y < h; y++) std::memset(static_cast<unsigned char*>(o.d.plane[k]) + (size_t)y * o.d.pitch[k], y, row);      // what a call writes
        rife_hip_apply_set_t s = g; s.wp = w; s.hp = h; expect(&s, mw, mh, true, "", "extent w, h");
        s = g; s.wp = (w + 63) / 64 * 64; s.hp = (h + 63) / 64 * 64; expect(&s, mw, mh, true, "", "extent padded");
        s = g; s.wp = w - 1; s.hp = h; expect(&s, mw, mh, false, "the extent", "extent under w");
        s = g; s.wp = w; s.hp = 0; expect(&s, mw, mh, false, "the extent", "extent w, 0");
        s = g; s.wp = 1 << 14; s.hp = (1 << 13) + 1; expect(&s, mw, mh, false, "the extent is too large", "extent over 2^27");
        // the shift pair
        static const int BAD[6][2] = {{0, -1}, {0, 1}, {1, 0}, {-1, 1}, {2, 2}, {-2, -2}};
        for (auto& bs : BAD) { s = g; s.shift_x = bs[0]; s.shift_y = bs[1]; expect(&s, mw, mh, false, "the shift pair", "shift not admitted"); }
        // the size against the motion
        expect(&g, mw + 2, mh, false, "does not fit a motion of", "motion wider");
        expect(&g, mw, mh + 2, false, "does not fit a motion of", "motion higher");
        if (sx == 1) { expect(&g, mw + 1, mh, false, "does not fit a motion of", "up: motion one wider"); }
        if (sx == -1 && mw > 1) { s = g; s.shift_x = 0; s.shift_y = 0; expect(&s, mw, mh, false, "does not fit a motion of", "half planes at shift 0"); }
        expect(&g, 0, mh, false, "bad motion size", "mw = 0");
        expect(&g, mw, -1, false, "bad motion size", "mh < 0");
        // the descriptors
        s = g; s.p0 = nullptr; expect(&s, mw, mh, false, "planes 0: null planes descriptor", "null planes 0");
        s = g; s.p1 = nullptr; expect(&s, mw, mh, false, "planes 1: null planes descriptor", "null planes 1");
        s = g; s.out = nullptr; expect(&s, mw, mh, false, "planes out: null planes descriptor", "null planes out");
        rife_hip_planes_t c = b.d; c.pitch[0] = 0; s = g; s.p1 = &c; expect(&s, mw, mh, false, "planes 1: plane 0: the pitch is not positive", "bad pitch");
        c = b.d; c.n = n == 4 ? 3 : n + 1;
        if (c.n <= n) { s = g; s.p1 = &c; expect(&s, mw, mh, false, "the three plane sets differ", "n differs"); }
        if (rife_apply::integer(smp)) { c = o.d; c.maxval = 1; s = g; s.out = &c; expect(&s, mw, mh, false, "the three plane sets differ", "maxval differs"); }
        if (h > 1) { c = o.d; c.h = h - 1; s = g; s.out = &c; expect(&s, mw, mh, false, "the three plane sets differ", "h differs"); }
        // the sets of a call
        rife_hip_apply_set_t four[5] = {g, g, g, g, g};
        expect_sets(1, four, mw, mh, true, "", "one set");
        expect_sets(4, four, mw, mh, true, "", "four sets");
        expect_sets(0, four, mw, mh, false, "the set count (0) is not in 1..4", "no set");
        expect_sets(5, four, mw, mh, false, "the set count (5) is not in 1..4", "five sets");
        expect_sets(2, nullptr, mw, mh, false, "null sets", "null sets");
        four[2].shift_x = 3; expect_sets(4, four, mw, mh, false, "set 2: the shift pair (3, ", "the third set is bad");
        expect_sets(2, four, mw, mh, true, "", "the bad set is not among the first two");
    }
    expect(nullptr, 4, 4, false, "null set", "null set");
    std::printf("apply_set_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
