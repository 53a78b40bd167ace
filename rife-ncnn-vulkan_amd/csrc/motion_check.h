// motion_check.h: the host-only rules of a rife_hip_motion_t (include/rife_hip.h "motion export") - what rife_hip_motion_check answers and what every motion call
// repeats before it touches anything.  Plain C++, no HIP include: the engine (engine_abi.h) and the stand-alone sanitizer program
// (tests/sanitize/motion_check_main.cpp) compile this one statement.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/rife_hip.h"

namespace rife_motion {

static inline bool known(int format) { return format == RIFE_HIP_MOTION_F32 || format == RIFE_HIP_MOTION_F16; }
// bytes of one sample, of one flow pixel (dx0, dy0, dx1, dy1: what a lane stores as one vector) and of one mask element
static inline size_t sample_bytes(int format) { return format == RIFE_HIP_MOTION_F16 ? 2 : 4; }
static inline size_t flow_pixel_bytes(int format) { return 4 * sample_bytes(format); }
static inline size_t flow_row_bytes(int w, int format) { return w > 0 ? (size_t)w * flow_pixel_bytes(format) : 0; }
static inline size_t mask_row_bytes(int w, int format) { return w > 0 ? (size_t)w * sample_bytes(format) : 0; }

// one buffer: pitch >= row bytes, pointer and pitch aligned to `unit`, h * pitch < 2^32 (the kernels address it with 32-bit byte offsets, like the frame)
static inline int check_buffer(const char* name, const void* p, size_t pitch, size_t row, size_t unit, int h, std::string& err) {
    const std::string nm(name);
    if (pitch < row) { err = nm + ": the pitch (" + std::to_string(pitch) + ") is smaller than the row bytes (" + std::to_string(row) + ")"; return 1; }
    if (pitch % unit) { err = nm + ": the pitch is not a multiple of " + std::to_string(unit) + " bytes"; return 1; }
    if (reinterpret_cast<uintptr_t>(p) % (uintptr_t)unit) { err = nm + ": the pointer is not aligned to " + std::to_string(unit) + " bytes"; return 1; }
    if (pitch >= (1ull << 32) || (unsigned long long)h * (unsigned long long)pitch >= (1ull << 32)) { err = nm + ": h * pitch reaches 2^32 bytes"; return 1; }
    return 0;
}

// 0, or 1 with the fault in `err`
static inline int check(const rife_hip_motion_t* m, int w, int h, std::string& err) {
    if (!m) { err = "null motion descriptor"; return 1; }
    if (w <= 0 || h <= 0) { err = "bad frame size"; return 1; }
    if (!known(m->format)) { err = "unknown motion format"; return 1; }
    if (!m->flow && !m->mask) { err = "flow and mask are both NULL: nothing to export"; return 1; }
    if (m->flow && check_buffer("flow", m->flow, m->flow_pitch, flow_row_bytes(w, m->format), flow_pixel_bytes(m->format), h, err)) return 1;
    if (m->mask && check_buffer("mask", m->mask, m->mask_pitch, mask_row_bytes(w, m->format), sample_bytes(m->format), h, err)) return 1;
    return 0;
}

}  // namespace rife_motion
