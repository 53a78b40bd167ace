// image_check.h: the host-only rules of a rife_hip_image_t (include/rife_hip.h "strides and planes") - what rife_hip_image_check / rife_hip_image_row_bytes
// answer and what every image call repeats before it touches anything.  Plain C++, no HIP include: the engine (engine_image.h) and the stand-alone
// sanitizer program (tests/sanitize/image_check_main.cpp) compile this one statement.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/rife_hip.h"

namespace rife_img {

static inline int base(int pixfmt) { return pixfmt & 0xff; }
// YUV formats are 16 * class + 2 * (10 bits) + planar; class 1 = 4:2:0 (all four), 2 = 4:2:2 and 3 = 4:4:4 (planar only)
static inline int yuv_class(int pixfmt) { return base(pixfmt) >> 4; }
static inline bool is_yuv(int pixfmt) {
    const int b = base(pixfmt);
    return (b >= RIFE_HIP_PIX_NV12 && b <= RIFE_HIP_PIX_I420P10) || b == RIFE_HIP_PIX_I422 || b == RIFE_HIP_PIX_I422P10 || b == RIFE_HIP_PIX_I444 || b == RIFE_HIP_PIX_I444P10;
}
// planar RGB is class 4 of that numbering: planes R, G, B of w x h samples each; k = 0 u8, 1 u16, 2 half, 3 float (the even, packed slots are unknown formats)
static inline bool is_rgbp(int pixfmt) {
    const int b = base(pixfmt);
    return b == RIFE_HIP_PIX_RGBP8 || b == RIFE_HIP_PIX_RGBP10 || b == RIFE_HIP_PIX_RGBPH || b == RIFE_HIP_PIX_RGBPF;
}
static inline bool known(int pixfmt) {
    const int b = base(pixfmt);
    return pixfmt >= 0 && (b == RIFE_HIP_PIX_RGB8 || b == RIFE_HIP_PIX_RGB10_U16 || b == RIFE_HIP_PIX_A2B10G10R10 || b == RIFE_HIP_PIX_RGBA8 || is_yuv(pixfmt) || is_rgbp(pixfmt));
}
// the rules of the _px calls for a pixfmt argument (format | colour description); nullptr = fine
static inline const char* pixfmt_fault(int pixfmt) {
    const int csp = pixfmt & ~0xff;
    if (!known(pixfmt) || (csp & ~0x1f00)) return "unknown pixel format";
    if (!is_yuv(pixfmt)) return csp ? "a colour description (RIFE_HIP_CSP_*) goes with a YUV format, not with an RGB format" : nullptr;
    if (((csp >> 8) & 15) > 2) return "unknown colour matrix";
    if ((csp & RIFE_HIP_CSP_FULL) && is_yuv(pixfmt) && (base(pixfmt) & 2))
        return "full-range YUV is served at 8 bits only (the 10-bit full-range round trip through 10-bit RGB is not exact)";
    return nullptr;
}
// bytes of one sample group the kernels address as a unit: 1 for the u8 formats, 2 for the u16 and half formats, 4 for A2B10G10R10 and float planes
static inline int elem_size(int pixfmt) {
    const int b = base(pixfmt);
    if (is_rgbp(pixfmt)) return b == RIFE_HIP_PIX_RGBP8 ? 1 : b == RIFE_HIP_PIX_RGBPF ? 4 : 2;
    return b == RIFE_HIP_PIX_A2B10G10R10 ? 4 : (b == RIFE_HIP_PIX_RGB10_U16 || (is_yuv(pixfmt) && (b & 2))) ? 2 : 1;
}
static inline int planes(int pixfmt) {
    const int b = base(pixfmt);
    return !known(pixfmt) ? 0 : is_rgbp(pixfmt) ? 3 : !is_yuv(pixfmt) ? 1 : (b == RIFE_HIP_PIX_NV12 || b == RIFE_HIP_PIX_P010) ? 2 : 3;
}
// rows of plane p of a 4:2:0 frame h rows high: h for the first plane, ch = (h + 1) / 2 for chroma
static inline int plane_rows(int h, int p) { return p == 0 ? h : (h + 1) / 2; }
// the same for any format: the chroma planes of 4:2:2 and 4:4:4 and the planes of planar RGB (class 4) have h rows
static inline int plane_rows(int h, int pixfmt, int p) { return yuv_class(pixfmt) >= 2 ? h : plane_rows(h, p); }
// bytes of one row of plane p, 0 for a plane the format does not have (or w <= 0, an unknown format)
static inline size_t row_bytes(int w, int pixfmt, int p) {
    if (w <= 0 || p < 0 || p >= planes(pixfmt)) return 0;
    const int b = base(pixfmt);
    if (is_rgbp(pixfmt)) return (size_t)w * (size_t)elem_size(pixfmt);
    if (!is_yuv(pixfmt)) return (size_t)w * (b == RIFE_HIP_PIX_RGB8 ? 3 : b == RIFE_HIP_PIX_RGB10_U16 ? 6 : 4);
    const size_t cw = yuv_class(pixfmt) == 3 ? (size_t)w : ((size_t)w + 1) / 2, es = (size_t)elem_size(pixfmt);
    return p == 0 ? (size_t)w * es : planes(pixfmt) == 2 ? 2 * cw * es : cw * es;
}

// 0, or 1 with the fault in `err`
static inline int check(const rife_hip_image_t* im, std::string& err) {
    if (!im) { err = "null image descriptor"; return 1; }
    if (im->w <= 0 || im->h <= 0) { err = "bad frame size"; return 1; }
    if (const char* f = pixfmt_fault(im->pixfmt)) { err = f; return 1; }
    const int es = elem_size(im->pixfmt), np = planes(im->pixfmt);
    for (int p = 0; p < np; p++) {
        const std::string pl = "plane " + std::to_string(p);
        if (!im->plane[p]) { err = pl + " is NULL"; return 1; }
        const ptrdiff_t pitch = im->pitch[p];
        const size_t rb = row_bytes(im->w, im->pixfmt, p);
        if (pitch <= 0) { err = pl + ": the pitch is " + (pitch < 0 ? "negative (bottom-up rows are not served)" : "zero"); return 1; }
        if ((unsigned long long)pitch < (unsigned long long)rb) { err = pl + ": the pitch (" + std::to_string((long long)pitch) + ") is smaller than the row bytes (" + std::to_string(rb) + ")"; return 1; }
        if ((long long)pitch > (long long)INT32_MAX) { err = pl + ": the pitch is larger than INT32_MAX"; return 1; }
        if (pitch % es) { err = pl + ": the pitch is not a multiple of the element size (" + std::to_string(es) + ")"; return 1; }
        if (reinterpret_cast<uintptr_t>(im->plane[p]) % (uintptr_t)es) { err = pl + ": the pointer is not aligned to the element size (" + std::to_string(es) + ")"; return 1; }
    }
    return 0;
}
// the three images of one call agree in size and format
static inline int check_same(const rife_hip_image_t* a, const rife_hip_image_t* b, std::string& err) {
    if (a->w != b->w || a->h != b->h) { err = "the images of one call differ in size"; return 1; }
    if (a->pixfmt != b->pixfmt) { err = "the images of one call differ in pixel format or colour description"; return 1; }
    return 0;
}
// every row of every plane sits where the tight frame of the _px calls has it (planes glued one after the other)
static inline bool is_tight(const rife_hip_image_t* im) {
    const uint8_t* at = static_cast<const uint8_t*>(im->plane[0]);
    for (int p = 0; p < planes(im->pixfmt); p++) {
        const size_t rb = row_bytes(im->w, im->pixfmt, p);
        if (static_cast<const uint8_t*>(im->plane[p]) != at || (size_t)im->pitch[p] != rb) return false;
        at += rb * (size_t)plane_rows(im->h, im->pixfmt, p);
    }
    return true;
}

}  // namespace rife_img
