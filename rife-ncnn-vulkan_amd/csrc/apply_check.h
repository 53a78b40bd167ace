// apply_check.h: the host-only rules of a rife_hip_planes_t and of an apply call (include/rife_hip.h "apply motion") - what rife_hip_planes_check answers and what
// every apply call repeats before it touches anything.  Plain C++, no HIP include: the engine (engine_abi.h) and the stand-alone sanitizer program
// (tests/sanitize/apply_check_main.cpp) compile this one statement.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/rife_hip.h"
#include "motion_check.h"

namespace rife_apply {

static inline bool known(int sample) { return sample >= RIFE_HIP_SAMPLE_U8 && sample <= RIFE_HIP_SAMPLE_F32; }
static inline size_t sample_bytes(int sample) { return sample == RIFE_HIP_SAMPLE_U8 ? 1 : sample == RIFE_HIP_SAMPLE_F32 ? 4 : 2; }
static inline bool integer(int sample) { return sample == RIFE_HIP_SAMPLE_U8 || sample == RIFE_HIP_SAMPLE_U16; }
static inline int maxval_limit(int sample) { return sample == RIFE_HIP_SAMPLE_U8 ? 255 : 65535; }
static inline size_t row_bytes(int w, int sample) { return w > 0 ? (size_t)w * sample_bytes(sample) : 0; }

// 0, or 1 with the fault in `err`
static inline int check(const rife_hip_planes_t* p, std::string& err) {
    if (!p) { err = "null planes descriptor"; return 1; }
    if (p->w <= 0 || p->h <= 0) { err = "bad plane size"; return 1; }
    if (p->n < 1 || p->n > 4) { err = "the plane count (" + std::to_string(p->n) + ") is not in 1..4"; return 1; }
    if (!known(p->sample)) { err = "unknown sample type"; return 1; }
    if (integer(p->sample)) {
        if (p->maxval < 1 || p->maxval > maxval_limit(p->sample)) { err = "maxval (" + std::to_string(p->maxval) + ") is not in 1.." + std::to_string(maxval_limit(p->sample)); return 1; }
    } else if (p->maxval != 0) { err = "maxval must be 0 for float samples"; return 1; }
    const size_t es = sample_bytes(p->sample), row = row_bytes(p->w, p->sample);
    for (int k = 0; k < p->n; k++) {
        const std::string nm = "plane " + std::to_string(k);
        if (!p->plane[k]) { err = nm + ": null pointer"; return 1; }
        if (p->pitch[k] <= 0) { err = nm + ": the pitch is not positive"; return 1; }
        const size_t pitch = (size_t)p->pitch[k];
        if (pitch < row) { err = nm + ": the pitch (" + std::to_string(pitch) + ") is smaller than the row bytes (" + std::to_string(row) + ")"; return 1; }
        if (pitch % es) { err = nm + ": the pitch is not a multiple of the element size (" + std::to_string(es) + ")"; return 1; }
        if (reinterpret_cast<uintptr_t>(p->plane[k]) % (uintptr_t)es) { err = nm + ": the pointer is not aligned to the element size (" + std::to_string(es) + ")"; return 1; }
        if (pitch >= (1ull << 32) || (unsigned long long)p->h * (unsigned long long)pitch >= (1ull << 32)) { err = nm + ": h * pitch reaches 2^32 bytes"; return 1; }
    }
    return 0;
}

static inline bool agree(const rife_hip_planes_t& a, const rife_hip_planes_t& b) {
    return a.w == b.w && a.h == b.h && a.n == b.n && a.sample == b.sample && a.maxval == b.maxval;
}

// the extent of an apply call: 0, 0 (= w, h) or at least w, h, and no more pixels than the frame path accepts (2^27: process_common)
static inline int check_extent(int w, int h, int wp, int hp, std::string& err) {
    if (wp == 0 && hp == 0) return 0;
    if (wp < w || hp < h) { err = "the extent (" + std::to_string(wp) + " x " + std::to_string(hp) + ") is neither 0, 0 nor at least the plane size"; return 1; }
    if ((long long)wp * hp > (1ll << 27)) { err = "the extent is too large (more than 2^27 pixels)"; return 1; }
    return 0;
}

// a whole apply call: the three plane sets, that they agree, the motion (both buffers) and the extent.  m == nullptr: a process_apply call, whose motion is the engine's.
static inline int check_call(const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_planes_t* out, const rife_hip_motion_t* m, bool with_motion,
                             int wp, int hp, std::string& err) {
    const rife_hip_planes_t* s[3] = {p0, p1, out};
    static const char* const nm[3] = {"planes 0: ", "planes 1: ", "planes out: "};
    for (int i = 0; i < 3; i++) if (check(s[i], err)) { err = nm[i] + err; return 1; }
    if (!agree(*p0, *p1) || !agree(*p0, *out)) { err = "the three plane sets differ in w, h, n, sample or maxval"; return 1; }
    if ((long long)p0->w * p0->h > (1ll << 27)) { err = "planes too large (more than 2^27 pixels)"; return 1; }
    if (with_motion) {
        if (rife_motion::check(m, p0->w, p0->h, err)) { err = "motion: " + err; return 1; }
        if (!m->flow || !m->mask) { err = "motion: an apply call needs both flow and mask"; return 1; }
    }
    return check_extent(p0->w, p0->h, wp, hp, err);
}

}  // namespace rife_apply
