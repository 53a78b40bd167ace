// semiplanar_check.h: the host-only rules of a semi-planar, MSB-aligned high-bit-depth image (include/rife_hip.h "semi-planar high bit depth": rife_hip_semiplanar_t) -
// what rife_hip_semiplanar_check answers and what the two semi-planar calls repeat before they touch anything - and the planar layout such an image stands for in the
// hbd call it is defined by.  Plain C++, no HIP include: the engine (engine_hbd_semiplanar.h) and the stand-alone sanitizer program
// (tests/sanitize/semiplanar_check_main.cpp) compile this one statement.
#pragma once
#include <climits>
#include <cstdint>
#include <string>

#include "../../include/rife_hip.h"

namespace rife_sp {

static inline int chroma_w(int w) { return (w + 1) / 2; }                          // Cb, Cr PAIRS per chroma row
static inline int chroma_h(int h, int chroma) { return chroma == 1 ? (h + 1) / 2 : h; }
// the layout of the planar hbd call that defines the result
static inline int planar_pixfmt(int chroma, int csp) { return (chroma == 1 ? RIFE_HIP_PIX_I420P10 : RIFE_HIP_PIX_I422P10) | csp; }

static inline int check_plane(const char* name, const void* p, ptrdiff_t pitch, long long row_bytes, const char* row_words, int rows, std::string& err) {
    const std::string n = name;
    if (!p) { err = "null " + n + " pointer"; return 1; }
    if (reinterpret_cast<uintptr_t>(p) & 1) { err = "the " + n + " pointer is not aligned to 2 bytes"; return 1; }
    if (pitch <= 0) { err = "the " + n + " pitch is not positive"; return 1; }
    if ((long long)pitch < row_bytes) { err = "the " + n + " pitch is smaller than a row of " + row_words + " bytes"; return 1; }
    if (pitch & 1) { err = "the " + n + " pitch is not a multiple of 2 bytes"; return 1; }
    if ((long long)pitch > (long long)INT32_MAX) { err = "the " + n + " pitch exceeds INT32_MAX"; return 1; }
    if ((unsigned long long)rows * (unsigned long long)pitch >= (1ull << 32)) { err = "the " + n + " plane: rows * pitch reaches 2^32 bytes"; return 1; }
    return 0;
}
// 0, or 1 with the fault in `err`
static inline int check(const rife_hip_semiplanar_t* im, std::string& err) {
    if (!im) { err = "null descriptor"; return 1; }
    if (im->w <= 0 || im->h <= 0) { err = "bad image size"; return 1; }
    if (im->chroma == 3) { err = "chroma 3: 4:4:4 semi-planar (P410 / P416) is not served"; return 1; }
    if (im->chroma != 1 && im->chroma != 2) { err = "the chroma mode (" + std::to_string(im->chroma) + ") is not 1 (4:2:0) or 2 (4:2:2)"; return 1; }
    if (im->csp & RIFE_HIP_CSP_FULL) { err = "RIFE_HIP_CSP_FULL: full-range YUV is served at 8 bits only"; return 1; }
    if ((im->csp & ~(3 << 8)) || (im->csp >> 8) > 2) { err = "the colour description (" + std::to_string(im->csp) + ") is not RIFE_HIP_CSP_BT709, _BT601 or _BT2020NCL"; return 1; }
    if (im->depth < 10 || im->depth > 16) { err = "the depth (" + std::to_string(im->depth) + ") is not in 10..16"; return 1; }
    if ((long long)im->w * im->h > (1ll << 27)) { err = "image too large (more than 2^27 pixels)"; return 1; }
    if (check_plane("y", im->y, im->pitch_y, 2ll * im->w, "w * 2", im->h, err)) return 1;
    if (check_plane("cbcr", im->cbcr, im->pitch_c, 4ll * chroma_w(im->w), "((w + 1) / 2) * 4", chroma_h(im->h, im->chroma), err)) return 1;
    return 0;
}
// the three images of one call: each by its name, and that they agree
static inline int check_call(const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, const rife_hip_semiplanar_t* out, std::string& err) {
    const rife_hip_semiplanar_t* im[3] = {in0, in1, out};
    static const char* const nm[3] = {"image 0: ", "image 1: ", "image out: "};
    for (int i = 0; i < 3; i++) if (check(im[i], err)) { err = nm[i] + err; return 1; }
    for (int i = 1; i < 3; i++) {
        const char* const other = i == 1 ? "image 1" : "image out";
        if (im[i]->w != in0->w || im[i]->h != in0->h) { err = std::string("image 0 and ") + other + " differ in size"; return 1; }
        if (im[i]->chroma != in0->chroma) { err = std::string("image 0 and ") + other + " differ in chroma"; return 1; }
        if (im[i]->csp != in0->csp) { err = std::string("image 0 and ") + other + " differ in csp"; return 1; }
        if (im[i]->depth != in0->depth) { err = std::string("image 0 and ") + other + " differ in depth"; return 1; }
    }
    return 0;
}

}  // namespace rife_sp
