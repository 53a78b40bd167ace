// High-bit-depth planes at the frame boundary (include/rife_hip.h "high bit depth"): the caller's pitched u16 planes at 10..16 bits -> the resident 10:10:10 dwords the
// network estimates motion on.  The proxy of the definition is never stored: a lane reduces each sample to its ten-bit code,
//     c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023)        depth 10: c = min(v, 1023)
// with a run-time shift (hbd_code; tests/hbd_ref.py reduce10 states it in numpy), and converts the codes with the device functions the ten-bit formats use (yuv.h
// yuv_to_pk10; planar RGB packs them as planar_rgb.h does), so the dwords are those of the ten-bit pre-processing kernels on the reduced planes.
//   k_preproc_hbd<SUBX, SUBY> / _x8     Y, Cb, Cr planes: SUBX, SUBY = 1, 1 4:2:0; 1, 0 4:2:2; 0, 0 4:4:4
//   k_preproc_hbd_rgb / _x8             R, G, B planes
// They sit where k_preproc_yuv_pitch, k_preproc_yuvc and k_preproc_rgbp sit (run_v4's pre-processing step).  Scalar form: any size, element-aligned planes.  x8 form:
// w % 8 == 0 and every plane pointer and pitch aligned to its load - 16 bytes for eight samples, 8 bytes for the four chroma samples of a subsampled row; the host
// picks (hbd_x8_ok), as launch_preproc_planes does.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yuv.h"
#include "planar_rgb.h"

namespace rife {

// the reduction as the kernels take it: sh = depth - 10, rnd = half of the divisor (depth 10: 0, 0)
struct HbdShift { uint32_t sh, rnd; };
static inline HbdShift hbd_shift(int depth) { return HbdShift{(uint32_t)(depth - 10), depth > 10 ? 1u << (depth - 11) : 0u}; }
__host__ __device__ __forceinline__ int hbd_code(uint32_t v, HbdShift r) {
    const uint32_t c = (v + r.rnd) >> r.sh;                                   // v < 2^16, rnd <= 32: no overflow
    return (int)(c < 1023u ? c : 1023u);
}
// N = 8 / 4 consecutive u16 samples from an address aligned to 16 / 8 bytes, as codes
__device__ __forceinline__ void hbd_load8(const uint8_t* row, int x, HbdShift r, int* c) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + (size_t)x * 2);
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; i++) { c[2 * i] = hbd_code(d[i] & 0xffffu, r); c[2 * i + 1] = hbd_code(d[i] >> 16, r); }
}
__device__ __forceinline__ void hbd_load4(const uint8_t* row, int x, HbdShift r, int* c) {
    const uint2 q = *reinterpret_cast<const uint2*>(row + (size_t)x * 2);
    c[0] = hbd_code(q.x & 0xffffu, r); c[1] = hbd_code(q.x >> 16, r); c[2] = hbd_code(q.y & 0xffffu, r); c[3] = hbd_code(q.y >> 16, r);
}

// ---- Y'CbCr, scalar: two columns x (1 + SUBY) rows of the PADDED frame per lane; grid ((wp / 2 + 255) / 256, hp / (1 + SUBY)) ----
template <int SUBX, int SUBY>
__global__ void k_preproc_hbd(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k, HbdShift r) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2, y = blockIdx.y * (1 + SUBY);
    if (x >= wp) return;
    uint2 o[1 + SUBY];
#pragma unroll
    for (int i = 0; i <= SUBY; i++) o[i] = make_uint2(0u, 0u);
    if (x < w && y < h) {
        const int cy = SUBY ? y / 2 : y, cx = SUBX ? x / 2 : x;
        const uint16_t* c0 = reinterpret_cast<const uint16_t*>(s.p[1] + (size_t)cy * s.pitch[1]) + cx;
        const uint16_t* c1 = reinterpret_cast<const uint16_t*>(s.p[2] + (size_t)cy * s.pitch[2]) + cx;
        const int cb0 = hbd_code(c0[0], r), cr0 = hbd_code(c1[0], r);
        int cb1 = cb0, cr1 = cr0;
        if (!SUBX && x + 1 < w) { cb1 = hbd_code(c0[1], r); cr1 = hbd_code(c1[1], r); }
#pragma unroll
        for (int i = 0; i <= SUBY; i++) {
            if (y + i >= h) break;
            const uint16_t* p = reinterpret_cast<const uint16_t*>(s.p[0] + (size_t)(y + i) * s.pitch[0]) + x;
            o[i].x = yuv_to_pk10(k, hbd_code(p[0], r), cb0, cr0);
            if (x + 1 < w) o[i].y = yuv_to_pk10(k, hbd_code(p[1], r), cb1, cr1);
        }
    }
#pragma unroll
    for (int i = 0; i <= SUBY; i++) *reinterpret_cast<uint2*>(out + (size_t)(y + i) * wp + x) = o[i];      // wp, hp are multiples of 32: x is even, row y + SUBY exists
}
// ---- Y'CbCr, x8: eight columns x (1 + SUBY) rows of the PADDED frame per lane (w % 8 == 0, aligned planes and pitches); grid ((wp / 8 + 255) / 256, hp / (1 + SUBY)) ----
template <int SUBX, int SUBY>
__global__ void k_preproc_hbd_x8(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k, HbdShift r) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y * (1 + SUBY);
    if (x >= wp) return;                                                      // wp is a multiple of 32: a lane's run is inside the row or past it
    uint32_t o[1 + SUBY][8];
#pragma unroll
    for (int i = 0; i <= SUBY; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) o[i][j] = 0u;
    if (x < w && y < h) {                                                     // w is a multiple of 8: the whole run is inside the frame
        int cb[8], cr[8], yv[8];
        const int cy = SUBY ? y / 2 : y;
        const uint8_t* c0 = s.p[1] + (size_t)cy * s.pitch[1];
        const uint8_t* c1 = s.p[2] + (size_t)cy * s.pitch[2];
        if (SUBX) { hbd_load4(c0, x / 2, r, cb); hbd_load4(c1, x / 2, r, cr); }
        else { hbd_load8(c0, x, r, cb); hbd_load8(c1, x, r, cr); }
#pragma unroll
        for (int i = 0; i <= SUBY; i++) {
            if (y + i >= h) break;
            hbd_load8(s.p[0] + (size_t)(y + i) * s.pitch[0], x, r, yv);
#pragma unroll
            for (int j = 0; j < 8; j++) o[i][j] = yuv_to_pk10(k, yv[j], cb[SUBX ? j / 2 : j], cr[SUBX ? j / 2 : j]);
        }
    }
#pragma unroll
    for (int i = 0; i <= SUBY; i++) {
        uint4* d = reinterpret_cast<uint4*>(out + (size_t)(y + i) * wp + x);
        d[0] = make_uint4(o[i][0], o[i][1], o[i][2], o[i][3]);
        d[1] = make_uint4(o[i][4], o[i][5], o[i][6], o[i][7]);
    }
}
// ---- planar RGB, scalar: one pixel of the PADDED frame per lane; grid ((wp + 255) / 256, hp) ----
__global__ void k_preproc_hbd_rgb(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, HbdShift r) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= wp) return;
    uint32_t v = 0u;
    if (x < w && y < h) {
        const uint32_t cr = (uint32_t)hbd_code(reinterpret_cast<const uint16_t*>(s.p[0] + (size_t)y * s.pitch[0])[x], r);
        const uint32_t cg = (uint32_t)hbd_code(reinterpret_cast<const uint16_t*>(s.p[1] + (size_t)y * s.pitch[1])[x], r);
        const uint32_t cb = (uint32_t)hbd_code(reinterpret_cast<const uint16_t*>(s.p[2] + (size_t)y * s.pitch[2])[x], r);
        v = cr | (cg << 10) | (cb << 20);
    }
    out[(size_t)y * wp + x] = v;                                              // blockIdx.y < hp: the grid has hp rows
}
// ---- planar RGB, x8: eight columns of one row of the PADDED frame per lane (w % 8 == 0, aligned planes and pitches); grid ((wp / 8 + 255) / 256, hp) ----
__global__ void k_preproc_hbd_rgb_x8(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, HbdShift r) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y;
    if (x >= wp) return;
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = 0u;
    if (x < w && y < h) {
        int cr[8], cg[8], cb[8];
        hbd_load8(s.p[0] + (size_t)y * s.pitch[0], x, r, cr);
        hbd_load8(s.p[1] + (size_t)y * s.pitch[1], x, r, cg);
        hbd_load8(s.p[2] + (size_t)y * s.pitch[2], x, r, cb);
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = (uint32_t)cr[j] | ((uint32_t)cg[j] << 10) | ((uint32_t)cb[j] << 20);
    }
    uint4* d = reinterpret_cast<uint4*>(out + (size_t)y * wp + x);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// ---- host side ----
// the x8 forms load eight samples of a full-width plane (16 bytes) and four of a subsampled chroma row (8 bytes): every plane pointer and pitch is aligned to its load
static inline bool hbd_x8_ok(const PlaneSet& s, int w, int fmt) {
    const unsigned ac = (fmt == RIFE_HIP_PIX_I420P10 || fmt == RIFE_HIP_PIX_I422P10) ? 8u : 16u;
    return (w & 7) == 0 && planes_aligned(s, 0, 16u) && planes_aligned(s, 1, ac) && planes_aligned(s, 2, ac);
}
// pixfmt: one of the four bases (I420P10, I422P10, I444P10 with their colour bits, RGBP10); force_scalar: the single-kernel test runs both forms on one image
static inline void launch_preproc_hbd(hipStream_t st, const PlaneSet& s, int w, int h, uint32_t* out, int wp, int hp, int pixfmt, int depth, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    const HbdShift r = hbd_shift(depth);
    const bool x8 = !force_scalar && hbd_x8_ok(s, w, fmt);
    if (fmt == RIFE_HIP_PIX_RGBP10) {
        if (x8) hipLaunchKernelGGL(k_preproc_hbd_rgb_x8, dim3((wp / 8 + 255) / 256, hp), dim3(256), 0, st, s, w, h, out, wp, hp, r);
        else hipLaunchKernelGGL(k_preproc_hbd_rgb, dim3((wp + 255) / 256, hp), dim3(256), 0, st, s, w, h, out, wp, hp, r);
        return;
    }
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, 10);
    const int suby = fmt == RIFE_HIP_PIX_I420P10 ? 1 : 0;
    const dim3 g = x8 ? dim3((wp / 8 + 255) / 256, hp / (1 + suby)) : dim3((wp / 2 + 255) / 256, hp / (1 + suby));
#define RIFE_HBD_IN(SX, SY) do { if (x8) hipLaunchKernelGGL((k_preproc_hbd_x8<SX, SY>), g, dim3(256), 0, st, s, w, h, out, wp, hp, k, r); \
                                 else hipLaunchKernelGGL((k_preproc_hbd<SX, SY>), g, dim3(256), 0, st, s, w, h, out, wp, hp, k, r); } while (0)
    if (fmt == RIFE_HIP_PIX_I420P10) RIFE_HBD_IN(1, 1); else if (fmt == RIFE_HIP_PIX_I422P10) RIFE_HBD_IN(1, 0); else RIFE_HBD_IN(0, 0);
#undef RIFE_HBD_IN
}
// the two input images of an hbd call, as run_v4 takes them
struct HbdIO {
    PlaneSet in0, in1;
    int depth;
    int packed = 0;      // 3 / 4: in0.p[0], in1.p[0] are packed frames of that many interleaved samples per pixel (hbd_packed.h); 0: planes
    int semiplanar = 0;  // 1: p[0] is the Y plane and p[1] the plane of interleaved Cb, Cr pairs, codes in the HIGH bits (hbd_semiplanar.h); 0: planar, codes in the low bits
};

}  // namespace rife
