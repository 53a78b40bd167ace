// Planar RGB at the frame boundary (include/rife_hip.h RIFE_HIP_PIX_RGBP8 / RGBP10 / RGBPH / RGBPF): three planes R, G, B of u8, u16, half or float samples, and the
// two streaming kernels that stand between them and the depth-10 schedule.  tests/planar_ref.py states the same conversions in numpy; the two agree bit for bit.
//   k_preproc_rgbp<T> / _wide    R, G, B planes -> resident 10:10:10 dwords (img0 / img1), zero-padded
//   k_postproc_rgbp<T> / _wide   the pass's A2B10G10R10 frame (tight, pitch w) -> R, G, B planes: each row's own bytes and nothing else
// T = uint8_t, uint16_t, _Float16, float.  Like the 4:2:2 / 4:4:4 kernels of yuv.h they take their planes as a PlaneSet (pointer and pitch per plane), so one set
// serves tight frames (rgbp_tight_planes) and the caller's pitched planes.  The scalar form moves one pixel per lane (any size, any element-aligned pointer); the
// wide form 16 bytes per lane and plane (u8: 8 bytes), i.e. eight pixels per lane (float: four), when w % 8 == 0 and every pointer and pitch is aligned to that
// access.  The host picks the form (rgbp_wide_ok).  No LDS, no scratch: a lane holds at most 3 x 16 bytes of samples and eight dwords.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yuv.h"

namespace rife {

// fmt = the format bits of a pixfmt: 16 * 4 + 2 * k + 1, k = 0 u8, 1 u16, 2 half, 3 float
static inline bool rgbp_fmt(int fmt) { return fmt == RIFE_HIP_PIX_RGBP8 || fmt == RIFE_HIP_PIX_RGBP10 || fmt == RIFE_HIP_PIX_RGBPH || fmt == RIFE_HIP_PIX_RGBPF; }
static inline size_t rgbp_elem(int fmt) { return fmt == RIFE_HIP_PIX_RGBP8 ? 1 : fmt == RIFE_HIP_PIX_RGBPF ? 4 : 2; }

// ---- the conversions (include/rife_hip.h states them; host and device run this one statement) ----
// a float sample -> its code: clamp to [0, 1] (NaN and negatives: 0), times 1023, plus one half, truncate - product and sum rounded separately.  The comparisons
// are fminf(fmaxf(x, 0.f), 1.f) spelled out, so that no NaN of either kind survives whatever the float mode of the kernel is.
__host__ __device__ __forceinline__ uint32_t rgbp_code_f32(float x) {
#pragma clang fp contract(off)
    x = x > 0.f ? x : 0.f;
    x = x < 1.f ? x : 1.f;
    const float p = x * 1023.f;
    return (uint32_t)(int)(p + 0.5f);
}
// a code -> the float sample: a correctly rounded division (c * (1 / 1023.f) differs in 24 of the 1024 codes)
__host__ __device__ __forceinline__ float rgbp_f32_code(uint32_t c) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn((float)c, 1023.f);
#else
    return (float)c / 1023.f;
#endif
}
template <typename T> __host__ __device__ __forceinline__ uint32_t rgbp_to10(T v);
template <> __host__ __device__ __forceinline__ uint32_t rgbp_to10<uint8_t>(uint8_t v) { return ((uint32_t)v << 2) | ((uint32_t)v >> 6); }
template <> __host__ __device__ __forceinline__ uint32_t rgbp_to10<uint16_t>(uint16_t v) { return v < 1023u ? (uint32_t)v : 1023u; }
template <> __host__ __device__ __forceinline__ uint32_t rgbp_to10<_Float16>(_Float16 v) { return rgbp_code_f32((float)v); }
template <> __host__ __device__ __forceinline__ uint32_t rgbp_to10<float>(float v) { return rgbp_code_f32(v); }
template <typename T> __host__ __device__ __forceinline__ T rgbp_from10(uint32_t c);
template <> __host__ __device__ __forceinline__ uint8_t rgbp_from10<uint8_t>(uint32_t c) { return (uint8_t)(c >> 2); }
template <> __host__ __device__ __forceinline__ uint16_t rgbp_from10<uint16_t>(uint32_t c) { return (uint16_t)c; }
template <> __host__ __device__ __forceinline__ _Float16 rgbp_from10<_Float16>(uint32_t c) { return (_Float16)rgbp_f32_code(c); }      // round to nearest even
template <> __host__ __device__ __forceinline__ float rgbp_from10<float>(uint32_t c) { return rgbp_f32_code(c); }
// timestep 0 / 1: the sample a pass over identical frames would write
template <typename T> __host__ __device__ __forceinline__ T rgbp_canon(T v) { return rgbp_from10<T>(rgbp_to10<T>(v)); }

// ---- in, scalar: one pixel of the PADDED frame per lane; grid ((wp + 255) / 256, hp) ----
template <typename T>
__global__ void k_preproc_rgbp(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= wp) return;
    uint32_t v = 0u;
    if (x < w && y < h) {
        const uint32_t r = rgbp_to10<T>(reinterpret_cast<const T*>(s.p[0] + (size_t)y * s.pitch[0])[x]);
        const uint32_t g = rgbp_to10<T>(reinterpret_cast<const T*>(s.p[1] + (size_t)y * s.pitch[1])[x]);
        const uint32_t b = rgbp_to10<T>(reinterpret_cast<const T*>(s.p[2] + (size_t)y * s.pitch[2])[x]);
        v = r | (g << 10) | (b << 20);
    }
    out[(size_t)y * wp + x] = v;                                              // blockIdx.y < hp: the grid has hp rows
}
// ---- out, scalar: one pixel of the frame per lane; rgb = A2B10G10R10, tight (pitch w); grid ((w + 255) / 256, h) ----
template <typename T>
__global__ void k_postproc_rgbp(const uint32_t* __restrict__ rgb, int w, int h, PlaneSet d) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t pk = rgb[(size_t)y * w + x];
    reinterpret_cast<T*>(d.p[0] + (size_t)y * d.pitch[0])[x] = rgbp_from10<T>(pk & 1023u);
    reinterpret_cast<T*>(d.p[1] + (size_t)y * d.pitch[1])[x] = rgbp_from10<T>((pk >> 10) & 1023u);
    reinterpret_cast<T*>(d.p[2] + (size_t)y * d.pitch[2])[x] = rgbp_from10<T>((pk >> 20) & 1023u);
}

// the wide access: N consecutive samples of one plane as ONE load or store of 16 bytes (u8: 8 bytes)
template <typename T> struct RgbpWide { typedef uint4 V; static constexpr int N = 16 / (int)sizeof(T); };
template <> struct RgbpWide<uint8_t> { typedef uint2 V; static constexpr int N = 8; };
template <typename T>
__device__ __forceinline__ void rgbp_load(const uint8_t* row, int x, T* v) {
    const typename RgbpWide<T>::V q = *reinterpret_cast<const typename RgbpWide<T>::V*>(row + (size_t)x * sizeof(T));
    __builtin_memcpy(v, &q, sizeof(q));
}
template <typename T>
__device__ __forceinline__ void rgbp_store(uint8_t* row, int x, const T* v) {
    typename RgbpWide<T>::V q;
    __builtin_memcpy(&q, v, sizeof(q));
    *reinterpret_cast<typename RgbpWide<T>::V*>(row + (size_t)x * sizeof(T)) = q;
}
// ---- in, wide: N columns of one row of the PADDED frame per lane (w % 8 == 0, planes and pitches aligned to the loads); grid ((wp / N + 255) / 256, hp) ----
template <typename T>
__global__ void k_preproc_rgbp_wide(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp) {
    constexpr int N = RgbpWide<T>::N;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * N, y = blockIdx.y;
    if (x >= wp) return;                                                      // wp is a multiple of 32, so of N: a lane's run is inside the row or past it
    uint32_t o[N];
#pragma unroll
    for (int i = 0; i < N; i++) o[i] = 0u;
    if (x < w && y < h) {                                                     // w is a multiple of 8, so of N: x < w means the whole run is inside the frame
        T r[N], g[N], b[N];
        rgbp_load<T>(s.p[0] + (size_t)y * s.pitch[0], x, r);
        rgbp_load<T>(s.p[1] + (size_t)y * s.pitch[1], x, g);
        rgbp_load<T>(s.p[2] + (size_t)y * s.pitch[2], x, b);
#pragma unroll
        for (int i = 0; i < N; i++) o[i] = rgbp_to10<T>(r[i]) | (rgbp_to10<T>(g[i]) << 10) | (rgbp_to10<T>(b[i]) << 20);
    }
    uint4* d = reinterpret_cast<uint4*>(out + (size_t)y * wp + x);
#pragma unroll
    for (int i = 0; i < N / 4; i++) d[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}
// ---- out, wide: N columns of one row per lane (w % 8 == 0, planes and pitches aligned to the stores); grid ((w / N + 255) / 256, h) ----
template <typename T>
__global__ void k_postproc_rgbp_wide(const uint32_t* __restrict__ rgb, int w, int h, PlaneSet d) {
    constexpr int N = RgbpWide<T>::N;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * N, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const uint4* s = reinterpret_cast<const uint4*>(rgb + (size_t)y * w + x);  // w % 8 == 0: every run starts on 16 bytes
    uint32_t px[N];
#pragma unroll
    for (int i = 0; i < N / 4; i++) { const uint4 a = s[i]; px[4 * i] = a.x; px[4 * i + 1] = a.y; px[4 * i + 2] = a.z; px[4 * i + 3] = a.w; }
    T r[N], g[N], b[N];
#pragma unroll
    for (int i = 0; i < N; i++) { r[i] = rgbp_from10<T>(px[i] & 1023u); g[i] = rgbp_from10<T>((px[i] >> 10) & 1023u); b[i] = rgbp_from10<T>((px[i] >> 20) & 1023u); }
    rgbp_store<T>(d.p[0] + (size_t)y * d.pitch[0], x, r);
    rgbp_store<T>(d.p[1] + (size_t)y * d.pitch[1], x, g);
    rgbp_store<T>(d.p[2] + (size_t)y * d.pitch[2], x, b);
}

// ---- host side ----
// the planes of a tight frame: R, G, B, each w x h samples, one after the other
static inline PlaneSet rgbp_tight_planes(const void* frame, int w, int h, int fmt) {
    const size_t es = rgbp_elem(fmt);
    PlaneSet s;
    for (int p = 0; p < 3; p++) { s.p[p] = static_cast<uint8_t*>(const_cast<void*>(frame)) + (size_t)p * w * h * es; s.pitch[p] = (size_t)w * es; }
    return s;
}
// the wide forms load / store 16 bytes per plane (u8: 8): every plane pointer and pitch is aligned to that, and w % 8 == 0 keeps every run inside a row (a tight
// frame with w % 8 == 0 at a 16-byte aligned address qualifies: rows and planes are multiples of 8 samples)
static inline bool rgbp_wide_ok(const PlaneSet& s, int w, int fmt) {
    const unsigned a = fmt == RIFE_HIP_PIX_RGBP8 ? 8u : 16u;
    return (w & 7) == 0 && planes_aligned(s, 0, a) && planes_aligned(s, 1, a) && planes_aligned(s, 2, a);
}
template <typename T>
static inline void launch_preproc_rgbp_t(hipStream_t st, const PlaneSet& s, int w, int h, uint32_t* out, int wp, int hp, bool wide) {
    if (wide) hipLaunchKernelGGL(k_preproc_rgbp_wide<T>, dim3((wp / RgbpWide<T>::N + 255) / 256, hp), dim3(256), 0, st, s, w, h, out, wp, hp);
    else hipLaunchKernelGGL(k_preproc_rgbp<T>, dim3((wp + 255) / 256, hp), dim3(256), 0, st, s, w, h, out, wp, hp);
}
template <typename T>
static inline void launch_postproc_rgbp_t(hipStream_t st, const uint32_t* rgb, int w, int h, const PlaneSet& d, bool wide) {
    if (wide) hipLaunchKernelGGL(k_postproc_rgbp_wide<T>, dim3((w / RgbpWide<T>::N + 255) / 256, h), dim3(256), 0, st, rgb, w, h, d);
    else hipLaunchKernelGGL(k_postproc_rgbp<T>, dim3((w + 255) / 256, h), dim3(256), 0, st, rgb, w, h, d);
}
// force_scalar: the single-kernel tests run both forms on one frame
static inline void launch_preproc_rgbp(hipStream_t st, const PlaneSet& s, int w, int h, uint32_t* out, int wp, int hp, int pixfmt, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    const bool wide = !force_scalar && rgbp_wide_ok(s, w, fmt);
    if (fmt == RIFE_HIP_PIX_RGBP8) launch_preproc_rgbp_t<uint8_t>(st, s, w, h, out, wp, hp, wide);
    else if (fmt == RIFE_HIP_PIX_RGBP10) launch_preproc_rgbp_t<uint16_t>(st, s, w, h, out, wp, hp, wide);
    else if (fmt == RIFE_HIP_PIX_RGBPH) launch_preproc_rgbp_t<_Float16>(st, s, w, h, out, wp, hp, wide);
    else launch_preproc_rgbp_t<float>(st, s, w, h, out, wp, hp, wide);
}
static inline void launch_postproc_rgbp(hipStream_t st, const uint32_t* rgb, int w, int h, const PlaneSet& d, int pixfmt, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    const bool wide = !force_scalar && rgbp_wide_ok(d, w, fmt);
    if (fmt == RIFE_HIP_PIX_RGBP8) launch_postproc_rgbp_t<uint8_t>(st, rgb, w, h, d, wide);
    else if (fmt == RIFE_HIP_PIX_RGBP10) launch_postproc_rgbp_t<uint16_t>(st, rgb, w, h, d, wide);
    else if (fmt == RIFE_HIP_PIX_RGBPH) launch_postproc_rgbp_t<_Float16>(st, rgb, w, h, d, wide);
    else launch_postproc_rgbp_t<float>(st, rgb, w, h, d, wide);
}

}  // namespace rife
