// TEST INFRASTRUCTURE ONLY - never linked into a product library.
// The motion entry points of include/rife_hip.h for the sanitizer builds of the host side: what csrc/rife.cpp calls from RIFE::process_motion and
// RIFE::process_frames_motion.  The stub engine blends its inputs without estimating any flow, so its motion is the one a copy has - flow 0 and mask 1 - timestep -
// written row by row into the caller's pitched buffers under the rules of csrc/motion_check.h (the real call's), after the frame call of the other stub files.
#include <cstring>
#include <string>
#include <vector>

#include "../../rife-ncnn-vulkan_amd/csrc/motion_check.h"

struct rife_hip_frame { std::vector<uint8_t> px; int w = 0, h = 0; };      // the definition of stub_engine.cpp, token for token

static void stub_motion_fill(const rife_hip_motion_t& m, int w, int h, float mask) {
    for (int y = 0; y < h; y++) {
        if (m.flow) std::memset(static_cast<uint8_t*>(m.flow) + (size_t)y * m.flow_pitch, 0, rife_motion::flow_row_bytes(w, m.format));
        if (!m.mask) continue;
        uint8_t* row = static_cast<uint8_t*>(m.mask) + (size_t)y * m.mask_pitch;
        for (int x = 0; x < w; x++) {
            if (m.format == RIFE_HIP_MOTION_F32) std::memcpy(row + 4 * (size_t)x, &mask, 4);
            else { const uint16_t hbits = mask >= 1.f ? 0x3c00 : mask <= 0.f ? 0 : 0x3800; std::memcpy(row + 2 * (size_t)x, &hbits, 2); }      // 1, 0, else one half
        }
    }
}

extern "C" {

int rife_hip_motion_check(const rife_hip_motion_t* m, int w, int h) {
    std::string err;
    return rife_motion::check(m, w, h, err) ? -RIFE_HIP_EINVAL : 0;
}

int rife_hip_process_motion(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, const rife_hip_motion_t* host_motion) {
    if (int rc = rife_hip_motion_check(host_motion, w, h)) return rc;
    if (int rc = rife_hip_process_px(r, in0, in1, w, h, timestep, out, pixfmt)) return rc;
    stub_motion_fill(*host_motion, w, h, 1.f - timestep);
    return 0;
}

int rife_hip_process_frames_motion(const rife_hip_t* r, const rife_hip_frame_t* frame0, const rife_hip_frame_t* frame1, float timestep, void* out,
                                   const rife_hip_motion_t* host_motion) {
    if (!frame0 || !frame1) return -RIFE_HIP_EINVAL;
    if (int rc = rife_hip_motion_check(host_motion, frame0->w, frame0->h)) return rc;
    if (int rc = rife_hip_process_frames(r, frame0, frame1, timestep, static_cast<uint8_t*>(out))) return rc;
    stub_motion_fill(*host_motion, frame0->w, frame0->h, 1.f - timestep);
    return 0;
}

}
