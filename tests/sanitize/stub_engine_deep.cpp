// TEST INFRASTRUCTURE ONLY - never linked into a product library.
// The deep-colour entry points of include/rife_hip.h for the sanitizer builds of the host side, next to stub_engine.cpp (which answers the 8-bit ones): what
// csrc/rife.cpp calls for an `elemsize 6, elempack 3` Mat, i.e. what `rife-hip -b 10` sends.  A 10-bit frame is "resident" as the heap copy of its 6 bytes per
// pixel in the same rife_hip_frame stub_engine.cpp defines, so rife_hip_process_frames there blends it byte by byte into the caller's 6 bytes per pixel: the
// memory traffic of the real call (which is what the sanitizers watch), not its values.  rife_hip_process_px blends the u16 codes themselves.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rife_hip.h"

struct rife_hip { bool loaded = false; int gpuid = 0; };                        // the definitions of stub_engine.cpp, token for token
struct rife_hip_frame { std::vector<uint8_t> px; int w = 0, h = 0; };

extern "C" {

size_t rife_hip_frame_bytes(int w, int h, int pixfmt) {
    const int bpp = pixfmt == RIFE_HIP_PIX_RGB8 ? 3 : pixfmt == RIFE_HIP_PIX_RGB10_U16 ? 6 : pixfmt == RIFE_HIP_PIX_A2B10G10R10 ? 4 : 0;
    return (w > 0 && h > 0) ? (size_t)w * h * bpp : 0;
}

int rife_hip_process_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt) {
    if (pixfmt == RIFE_HIP_PIX_RGB8) return rife_hip_process(r, (const uint8_t*)in0, (const uint8_t*)in1, w, h, timestep, (uint8_t*)out);
    if (pixfmt != RIFE_HIP_PIX_RGB10_U16 || !r || !r->loaded || !in0 || !in1 || !out || w <= 0 || h <= 0) return -RIFE_HIP_EINVAL;
    const uint16_t* a = (const uint16_t*)in0; const uint16_t* b = (const uint16_t*)in1; uint16_t* o = (uint16_t*)out;
    for (size_t i = 0; i < (size_t)w * h * 3; i++) o[i] = (uint16_t)((1.f - timestep) * a[i] + timestep * b[i] + 0.5f);
    return 0;
}

int rife_hip_frame_upload_px(const rife_hip_t* r, const void* pixels, int w, int h, int pixfmt, rife_hip_frame_t** frame) {
    if (pixfmt == RIFE_HIP_PIX_RGB8) return rife_hip_frame_upload(r, (const uint8_t*)pixels, w, h, frame);
    if (pixfmt != RIFE_HIP_PIX_RGB10_U16 || !r || !pixels || !frame || w <= 0 || h <= 0) return -RIFE_HIP_EINVAL;
    rife_hip_frame* f = new rife_hip_frame; f->w = w; f->h = h;
    f->px.assign((const uint8_t*)pixels, (const uint8_t*)pixels + (size_t)w * h * 6);
    *frame = f;
    return 0;
}

}  // extern "C"
