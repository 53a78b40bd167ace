// TEST INFRASTRUCTURE ONLY.  A program of its own for the sanitizer job (built with ASan + UBSan, nothing preloaded): csrc/motion_check.h - the host-only rules behind
// rife_hip_motion_check - walked over one refusing descriptor per rule and accepting descriptors per format, size and padding; every accepted descriptor is then
// written row by row the way a motion call fills it, so a rule that let a short buffer through would show as an out-of-bounds write.
// Exit status 0 and a last line "motion_check: N cases, 0 wrong" when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/motion_check.h"

static int g_cases = 0, g_wrong = 0;
static void expect(const rife_hip_motion_t* m, int w, int h, bool ok, const char* needle, const char* what) {
    std::string err;
    const int rc = rife_motion::check(m, w, h, err);
    g_cases++;
    if ((rc == 0) != ok || (!ok && err.find(needle) == std::string::npos)) { g_wrong++; std::printf("WRONG %s: rc %d, message '%s' (wanted '%s')\n", what, rc, err.c_str(), needle); }
}
static unsigned char* align16(std::vector<unsigned char>& v) { return v.data() + ((16 - reinterpret_cast<uintptr_t>(v.data()) % 16) % 16); }

int main() {
    static const int FMT[2] = {RIFE_HIP_MOTION_F32, RIFE_HIP_MOTION_F16};
    static const int SZ[3][2] = {{1, 1}, {33, 47}, {100, 60}};
    static const size_t PAD[2] = {0, 48};      // tight rows, and rows padded by a multiple of every alignment
    for (int f : FMT) for (auto& sz : SZ) for (size_t pad : PAD) {
        const int w = sz[0], h = sz[1];
        const size_t frow = rife_motion::flow_row_bytes(w, f), mrow = rife_motion::mask_row_bytes(w, f), fpx = rife_motion::flow_pixel_bytes(f), es = rife_motion::sample_bytes(f);
        std::vector<unsigned char> fmem((frow + pad) * h + 16, 0x5a), mmem((mrow + pad) * h + 16, 0x5a);
        rife_hip_motion_t m;
        m.flow = align16(fmem); m.flow_pitch = frow + pad; m.mask = align16(mmem); m.mask_pitch = mrow + pad; m.format = f;
        expect(&m, w, h, true, "", "accept");
        for (int y = 0; y < h; y++) {      // what a call writes: the row bytes of every row, nothing else
            std::memset(static_cast<unsigned char*>(m.flow) + (size_t)y * m.flow_pitch, y, frow);
            std::memset(static_cast<unsigned char*>(m.mask) + (size_t)y * m.mask_pitch, y, mrow);
        }
        rife_hip_motion_t b = m; b.flow = nullptr; b.flow_pitch = 0; expect(&b, w, h, true, "", "flow not wanted");
        b = m; b.mask = nullptr; b.mask_pitch = 0; expect(&b, w, h, true, "", "mask not wanted");
        b = m; b.flow = nullptr; b.mask = nullptr; expect(&b, w, h, false, "both NULL", "nothing wanted");
        b = m; b.format = 2; expect(&b, w, h, false, "unknown motion format", "format 2");
        b = m; b.format = -1; expect(&b, w, h, false, "unknown motion format", "format -1");
        b = m; b.flow_pitch = frow - fpx; expect(&b, w, h, false, "flow: the pitch", "flow pitch under the row bytes");
        b = m; b.mask_pitch = mrow - es; expect(&b, w, h, false, "mask: the pitch", "mask pitch under the row bytes");
        b = m; b.flow_pitch = frow + pad + es; expect(&b, w, h, false, "flow: the pitch is not a multiple", "flow pitch off the pixel");
        b = m; b.mask_pitch = mrow + pad + 1; expect(&b, w, h, false, "mask: the pitch is not a multiple", "mask pitch off the element");
        b = m; b.flow = static_cast<unsigned char*>(m.flow) + es; expect(&b, w, h, false, "flow: the pointer is not aligned", "flow pointer off the pixel");
        b = m; b.mask = static_cast<unsigned char*>(m.mask) + 1; expect(&b, w, h, false, "mask: the pointer is not aligned", "mask pointer off the element");
        b = m; b.flow_pitch = ((1ull << 32) / (size_t)h + fpx) / fpx * fpx; expect(&b, w, h, false, "flow: h * pitch reaches 2^32", "flow of 4 GB");
        b = m; b.mask_pitch = ((1ull << 32) / (size_t)h + es) / es * es; expect(&b, w, h, false, "mask: h * pitch reaches 2^32", "mask of 4 GB");
        b = m; b.flow_pitch = ((1ull << 32) - 1) / (size_t)h / fpx * fpx;
        if (b.flow_pitch >= frow) expect(&b, w, h, true, "", "flow just under 4 GB");
        expect(&m, 0, h, false, "bad frame size", "w = 0");
        expect(&m, w, -3, false, "bad frame size", "h < 0");
    }
    expect(nullptr, 4, 4, false, "null motion descriptor", "null descriptor");
    std::printf("motion_check: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
