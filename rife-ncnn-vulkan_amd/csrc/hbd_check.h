// hbd_check.h: the host-only rules of a high-bit-depth image (include/rife_hip.h "high bit depth": a rife_hip_image_t plus a depth) - what rife_hip_hbd_check answers
// and what the two hbd calls repeat before they touch anything - and the sets such an image stands for in the sets calls it is defined by.  Plain C++, no HIP include:
// the engine (engine_hbd.h) and the stand-alone sanitizer program (tests/sanitize/hbd_check_main.cpp) compile this one statement.  The rules of the image are
// image_check.h's, those of the sets apply_set_check.h's.
#pragma once
#include "apply_set_check.h"
#include "image_check.h"

namespace rife_hbd {

// the four layouts: planar u16, the ten-bit format the proxy is made in
static inline bool base_ok(int pixfmt) {
    const int b = rife_img::base(pixfmt);
    return b == RIFE_HIP_PIX_I420P10 || b == RIFE_HIP_PIX_I422P10 || b == RIFE_HIP_PIX_I444P10 || b == RIFE_HIP_PIX_RGBP10;
}
// the proxy sample of a stored sample (tests/hbd_ref.py reduce10; csrc/hbd.h runs this statement on the device)
static inline unsigned reduce10(unsigned v, int depth) {
    const unsigned c = depth > 10 ? (v + (1u << (depth - 11))) >> (depth - 10) : v;
    return c < 1023u ? c : 1023u;
}

// 0, or 1 with the fault in `err`
static inline int check(const rife_hip_image_t* im, int depth, std::string& err) {
    if (rife_img::check(im, err)) return 1;
    if (!base_ok(im->pixfmt)) {
        err = "pixel format " + std::to_string(rife_img::base(im->pixfmt)) + " is not a high-bit-depth layout (RIFE_HIP_PIX_I420P10, _I422P10, _I444P10 or _RGBP10)";
        return 1;
    }
    if (depth < 10 || depth > 16) { err = "the depth (" + std::to_string(depth) + ") is not in 10..16"; return 1; }
    // what the sets calls ask of the same planes (apply_check.h): byte offsets inside a plane are 32-bit, and no more pixels than the frame path takes
    if ((long long)im->w * im->h > (1ll << 27)) { err = "image too large (more than 2^27 pixels)"; return 1; }
    for (int p = 0; p < 3; p++)
        if ((unsigned long long)rife_img::plane_rows(im->h, im->pixfmt, p) * (unsigned long long)im->pitch[p] >= (1ull << 32)) {
            err = "plane " + std::to_string(p) + ": rows * pitch reaches 2^32 bytes";
            return 1;
        }
    return 0;
}
// the three images of one call: each by its name, and that they agree
static inline int check_call(const rife_hip_image_t* in0, const rife_hip_image_t* in1, const rife_hip_image_t* out, int depth, std::string& err) {
    const rife_hip_image_t* im[3] = {in0, in1, out};
    static const char* const nm[3] = {"image 0: ", "image 1: ", "image out: "};
    for (int i = 0; i < 3; i++) if (check(im[i], depth, err)) { err = nm[i] + err; return 1; }
    if (rife_img::check_same(in0, in1, err) || rife_img::check_same(in0, out, err)) return 1;
    return 0;
}

// The sets of the definition: I444P10 / RGBP10 one set of three planes at shift (0, 0); I420P10 / I422P10 the luma plane at (0, 0) and Cb, Cr at (-1, -1) / (-1, 0).
// Every set: u16 samples, maxval (1 << depth) - 1, extent 0, 0 (edge semantics).  The descriptors live in the struct; `sets` points into it.
struct Sets {
    int n = 0;
    rife_hip_planes_t d[2][3];      // [set][p0, p1, out]
    rife_hip_apply_set_t sets[2];
};
static inline void planes_of(rife_hip_planes_t& d, const rife_hip_image_t& im, int first, int n, int w, int h, int depth) {
    d = rife_hip_planes_t();
    d.w = w; d.h = h; d.n = n; d.sample = RIFE_HIP_SAMPLE_U16; d.maxval = (1 << depth) - 1;
    for (int k = 0; k < n; k++) { d.plane[k] = im.plane[first + k]; d.pitch[k] = im.pitch[first + k]; }
}
static inline void make_sets(Sets& s, const rife_hip_image_t& in0, const rife_hip_image_t& in1, const rife_hip_image_t& out, int depth) {
    const rife_hip_image_t* im[3] = {&in0, &in1, &out};
    const int cls = rife_img::yuv_class(in0.pixfmt), w = in0.w, h = in0.h;      // 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4, 4 = planar RGB
    const bool sub = cls == 1 || cls == 2;
    s.n = sub ? 2 : 1;
    for (int i = 0; i < 3; i++) {
        planes_of(s.d[0][i], *im[i], 0, sub ? 1 : 3, w, h, depth);
        if (sub) planes_of(s.d[1][i], *im[i], 1, 2, (w + 1) / 2, cls == 1 ? (h + 1) / 2 : h, depth);
    }
    for (int k = 0; k < s.n; k++) {
        s.sets[k] = rife_hip_apply_set_t();
        s.sets[k].p0 = &s.d[k][0]; s.sets[k].p1 = &s.d[k][1]; s.sets[k].out = &s.d[k][2];
        s.sets[k].shift_x = k ? -1 : 0; s.sets[k].shift_y = (k && cls == 1) ? -1 : 0;
    }
}

}  // namespace rife_hbd
