// TEST INFRASTRUCTURE ONLY - never linked into a product library.
// The 4:2:0 entry points of include/rife_hip.h for the sanitizer builds of the host side: what csrc/rife.cpp calls from process_yuv / upload_yuv, i.e. what
// `rife-hip -i in.y4m` sends.  The three _px symbols exist once per program and stub_engine_alpha.cpp cannot be wrapped a second time (it undefines the names it
// renames), so this file takes stub_engine_deep.cpp in the way that file does and answers RGBA8 (its words) AND the four YUV formats in front of it; the
// sanitizer binaries link this file INSTEAD of stub_engine_alpha.cpp.  A YUV frame is "resident" as the heap copy of its rife_hip_frame_bytes() bytes in the
// rife_hip_frame stub_engine.cpp defines, so rife_hip_process_frames there blends it byte by byte into the caller's frame: the memory traffic of the real call
// (which is what the sanitizers watch) and, for the 8-bit formats, values a test can predict.
#include "../../include/rife_hip.h"

#define rife_hip_frame_bytes stub_deep_frame_bytes
#define rife_hip_process_px stub_deep_process_px
#define rife_hip_frame_upload_px stub_deep_frame_upload_px
#include "stub_engine_deep.cpp"
#undef rife_hip_frame_bytes
#undef rife_hip_process_px
#undef rife_hip_frame_upload_px

static bool stub_is_yuv(int pixfmt) {      // a served format with a served colour description (the real engine's -EINVAL cases are refused here too)
    const int fmt = pixfmt & 0xff, m = (pixfmt >> 8) & 15;
    if (pixfmt < 0 || fmt < RIFE_HIP_PIX_NV12 || fmt > RIFE_HIP_PIX_I420P10 || (pixfmt & ~0x1fff) || m > 2) return false;
    return !((pixfmt & RIFE_HIP_CSP_FULL) && fmt >= RIFE_HIP_PIX_P010);
}
static size_t stub_own_bytes(int w, int h, int pixfmt) {      // RGBA8 or YUV; 0 otherwise
    if (w <= 0 || h <= 0) return 0;
    if (pixfmt == RIFE_HIP_PIX_RGBA8) return (size_t)w * h * 4;
    if (!stub_is_yuv(pixfmt)) return 0;
    return ((size_t)w * h + 2 * (size_t)((w + 1) / 2) * ((h + 1) / 2)) * ((pixfmt & 0xff) >= RIFE_HIP_PIX_P010 ? 2 : 1);
}

extern "C" {

size_t rife_hip_frame_bytes(int w, int h, int pixfmt) {
    const size_t n = pixfmt >= 0 ? stub_own_bytes(w, h, pixfmt & 0xff) : 0;
    return n ? n : stub_deep_frame_bytes(w, h, pixfmt);
}

int rife_hip_process_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt) {
    const size_t n = stub_own_bytes(w, h, pixfmt);
    if (!n) return stub_deep_process_px(r, in0, in1, w, h, timestep, out, pixfmt);
    if (!r || !r->loaded || !in0 || !in1 || !out) return -RIFE_HIP_EINVAL;
    const uint8_t* a = (const uint8_t*)in0; const uint8_t* b = (const uint8_t*)in1; uint8_t* o = (uint8_t*)out;
    for (size_t i = 0; i < n; i++) o[i] = (uint8_t)((1.f - timestep) * a[i] + timestep * b[i] + 0.5f);
    return 0;
}

int rife_hip_frame_upload_px(const rife_hip_t* r, const void* pixels, int w, int h, int pixfmt, rife_hip_frame_t** frame) {
    const size_t n = stub_own_bytes(w, h, pixfmt);
    if (!n) return stub_deep_frame_upload_px(r, pixels, w, h, pixfmt, frame);
    if (!r || !pixels || !frame) return -RIFE_HIP_EINVAL;
    rife_hip_frame* f = new rife_hip_frame; f->w = w; f->h = h;
    f->px.assign((const uint8_t*)pixels, (const uint8_t*)pixels + n);
    *frame = f;
    return 0;
}

}  // extern "C"
