// packed_check.h: the host-only rules of a packed 16-bit image (include/rife_hip.h "16-bit packed RGB and RGBA": rife_hip_packed_t) - what rife_hip_packed_check
// answers and what the two packed calls repeat before they touch anything - and the plane set such an image stands for in the sets call it is defined by.  Plain C++,
// no HIP include: the engine (engine_hbd_packed.h) and the stand-alone sanitizer program (tests/sanitize/packed_check_main.cpp) compile this one statement.
#pragma once
#include <climits>
#include <cstdint>
#include <string>

#include "../../include/rife_hip.h"

namespace rife_packed {

// 0, or 1 with the fault in `err`
static inline int check(const rife_hip_packed_t* im, std::string& err) {
    if (!im) { err = "null descriptor"; return 1; }
    if (im->w <= 0 || im->h <= 0) { err = "bad image size"; return 1; }
    if (im->channels != 3 && im->channels != 4) { err = "the channel count (" + std::to_string(im->channels) + ") is not 3 (R G B) or 4 (R G B A)"; return 1; }
    if (im->depth < 10 || im->depth > 16) { err = "the depth (" + std::to_string(im->depth) + ") is not in 10..16"; return 1; }
    if (!im->data) { err = "null data pointer"; return 1; }
    if (reinterpret_cast<uintptr_t>(im->data) & 1) { err = "the data pointer is not aligned to 2 bytes"; return 1; }
    if (im->pitch <= 0) { err = "the pitch is not positive"; return 1; }
    if ((long long)im->pitch < (long long)im->w * im->channels * 2) { err = "the pitch is smaller than a row of w * channels * 2 bytes"; return 1; }
    if (im->pitch & 1) { err = "the pitch is not a multiple of 2 bytes"; return 1; }
    if ((long long)im->pitch > (long long)INT32_MAX) { err = "the pitch exceeds INT32_MAX"; return 1; }
    if ((long long)im->w * im->h > (1ll << 27)) { err = "image too large (more than 2^27 pixels)"; return 1; }
    if ((unsigned long long)im->h * (unsigned long long)im->pitch >= (1ull << 32)) { err = "rows * pitch reaches 2^32 bytes"; return 1; }
    return 0;
}
// the three images of one call: each by its name, and that they agree
static inline int check_call(const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, const rife_hip_packed_t* out, std::string& err) {
    const rife_hip_packed_t* im[3] = {in0, in1, out};
    static const char* const nm[3] = {"image 0: ", "image 1: ", "image out: "};
    for (int i = 0; i < 3; i++) if (check(im[i], err)) { err = nm[i] + err; return 1; }
    for (int i = 1; i < 3; i++) {
        const char* const other = i == 1 ? "image 1" : "image out";
        if (im[i]->w != in0->w || im[i]->h != in0->h) { err = std::string("image 0 and ") + other + " differ in size"; return 1; }
        if (im[i]->channels != in0->channels) { err = std::string("image 0 and ") + other + " differ in channels"; return 1; }
        if (im[i]->depth != in0->depth) { err = std::string("image 0 and ") + other + " differ in depth"; return 1; }
    }
    return 0;
}
// one plane of w * channels samples: what the timestep 0 / 1 copy (k_apply_copy, apply_copy_host) takes
static inline rife_hip_planes_t as_plane(const rife_hip_packed_t& im) {
    rife_hip_planes_t d = rife_hip_planes_t();
    d.w = im.w * im.channels; d.h = im.h; d.n = 1; d.sample = RIFE_HIP_SAMPLE_U16; d.maxval = (1 << im.depth) - 1;
    d.plane[0] = im.data; d.pitch[0] = im.pitch;
    return d;
}

}  // namespace rife_packed
