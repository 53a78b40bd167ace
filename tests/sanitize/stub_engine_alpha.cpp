// TEST INFRASTRUCTURE ONLY - never linked into a product library.
// The RGBA entry points of include/rife_hip.h for the sanitizer builds of the host side: what csrc/rife.cpp calls for an `elemsize 4, elempack 4` Mat, i.e. what
// `rife-hip -a` sends.  The three _px symbols exist once per program, so this file takes stub_engine_deep.cpp in (renamed, unchanged) and answers
// RIFE_HIP_PIX_RGBA8 in front of it; the sanitizer binaries link this file INSTEAD of stub_engine_deep.cpp.  An RGBA frame is "resident" as the heap copy of
// its 4 bytes per pixel in the rife_hip_frame stub_engine.cpp defines, so rife_hip_process_frames there blends it byte by byte into the caller's 4 bytes per
// pixel: the memory traffic of the real call (which is what the sanitizers watch), not its values.
#include "../../include/rife_hip.h"

#define rife_hip_frame_bytes stub_deep_frame_bytes
#define rife_hip_process_px stub_deep_process_px
#define rife_hip_frame_upload_px stub_deep_frame_upload_px
#include "stub_engine_deep.cpp"
#undef rife_hip_frame_bytes
#undef rife_hip_process_px
#undef rife_hip_frame_upload_px

extern "C" {

size_t rife_hip_frame_bytes(int w, int h, int pixfmt) {
    if (pixfmt == RIFE_HIP_PIX_RGBA8) return (w > 0 && h > 0) ? (size_t)w * h * 4 : 0;
    return stub_deep_frame_bytes(w, h, pixfmt);
}

int rife_hip_process_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt) {
    if (pixfmt != RIFE_HIP_PIX_RGBA8) return stub_deep_process_px(r, in0, in1, w, h, timestep, out, pixfmt);
    if (!r || !r->loaded || !in0 || !in1 || !out || w <= 0 || h <= 0) return -RIFE_HIP_EINVAL;
    const uint8_t* a = (const uint8_t*)in0; const uint8_t* b = (const uint8_t*)in1; uint8_t* o = (uint8_t*)out;
    for (size_t i = 0; i < (size_t)w * h * 4; i++) o[i] = (uint8_t)((1.f - timestep) * a[i] + timestep * b[i] + 0.5f);
    return 0;
}

int rife_hip_frame_upload_px(const rife_hip_t* r, const void* pixels, int w, int h, int pixfmt, rife_hip_frame_t** frame) {
    if (pixfmt != RIFE_HIP_PIX_RGBA8) return stub_deep_frame_upload_px(r, pixels, w, h, pixfmt, frame);
    if (!r || !pixels || !frame || w <= 0 || h <= 0) return -RIFE_HIP_EINVAL;
    rife_hip_frame* f = new rife_hip_frame; f->w = w; f->h = h;
    f->px.assign((const uint8_t*)pixels, (const uint8_t*)pixels + (size_t)w * h * 4);
    *frame = f;
    return 0;
}

}  // extern "C"
