// Strided frames and separate planes at the boundary (include/rife_hip.h rife_hip_image_t): the pitched forms of the pre- and post-processing kernels.
// They read and write the caller's planes IN PLACE - a row of plane p starts at plane[p] + (size_t)y * pitch[p] BYTES - and restate the per-pixel arithmetic of
// the tight kernels (elementwise.h k_preproc*, yuv.h k_preproc_yuv / k_postproc_yuv) through the same device functions, so an image call is byte for byte the
// _px call on the repacked samples.  The tight kernels are untouched: a tight call launches what it launched before.
//   k_preproc_pitch<PX, WIDE>            RGB8 / RGB10_U16 / A2B10G10R10 / RGBA8 plane -> resident dwords, zero (alpha: edge) padded
//   k_preproc_yuv_pitch / _x8            Y, Cb, Cr (or Y, CbCr) planes -> resident 10:10:10 dwords
//   k_postproc_yuv_pitch / _x8           the pass's tight A2B10G10R10 frame -> Y, Cb, Cr (or Y, CbCr) planes
//   (4:2:2 / 4:4:4: yuv.h k_preproc_yuvc / k_postproc_yuvc take pitched planes to begin with; the launchers below pass the caller's planes to them.  Planar RGB:
//   planar_rgb.h k_preproc_rgbp / k_postproc_rgbp, likewise)
//   k_store_rows<T>                      the pass's tight RGB-format frame (Ctx::d_out) -> the caller's strided plane, row_bytes of each row and nothing else
//   k_canon_rows<MODE>                   timestep 0 / 1 at depth 10 and for half / float planes: strided plane -> strided plane in canonical form
// Wide forms (four pixels / a run of eight samples per lane): every plane pointer AND every pitch the kernel touches is aligned to the access width, and
// w % 4 / w % 8 holds as for the tight kernels; otherwise the scalar form runs.  The host picks (planes_*_wide below), as yuv_x8_ok does for tight frames.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstring>

#include "elementwise.h"
#include "yuv.h"
#include "planar_rgb.h"

namespace rife {

// one frame's planes as the kernels take them (PlaneSet: yuv.h)
static inline PlaneSet plane_set(const rife_hip_image_t& im) {
    PlaneSet s;
    for (int i = 0; i < 3; i++) { s.p[i] = static_cast<uint8_t*>(im.plane[i]); s.pitch[i] = (size_t)im.pitch[i]; }
    return s;
}

// ---- in, RGB formats: PX = RIFE_HIP_PIX_RGB8 / RGB10_U16 / A2B10G10R10 / RGBA8.  scalar: one pixel per lane, grid2d(wp, hp); WIDE: four, grid ((wp / 4 + 255) / 256, hp) ----
template <int PX, bool WIDE>
__global__ void k_preproc_pitch(const uint8_t* __restrict__ base, size_t pitch, int w, int h, uint32_t* __restrict__ out, int wp, int hp) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * (WIDE ? 4 : 1), y = blockIdx.y;
    if (x >= wp) return;
    const bool rgba = PX == RIFE_HIP_PIX_RGBA8;
    const uint8_t* const row = base + (size_t)(rgba ? min(y, h - 1) : y) * pitch;      // RGBA: the padding replicates alpha from the nearest frame pixel
    if (!WIDE) {
        uint32_t v = 0;
        if (rgba) {
            const uint8_t* p = row + (size_t)min(x, w - 1) * 4;
            v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            if (!(x < w && y < h)) v &= 0xff000000u;
        } else if (x < w && y < h) {
            if (PX == RIFE_HIP_PIX_RGB8) {
                const uint8_t* p = row + (size_t)x * 3;
                v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            } else if (PX == RIFE_HIP_PIX_RGB10_U16) {
                const uint16_t* p = reinterpret_cast<const uint16_t*>(row) + (size_t)x * 3;
                v = pack10(p[0], p[1], p[2]);
            } else v = reinterpret_cast<const uint32_t*>(row)[x] & 0x3fffffffu;
        }
        out[(size_t)y * wp + x] = v;
        return;
    }
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (rgba) {
        if (x < w) {
            v = *reinterpret_cast<const uint4*>(row + (size_t)x * 4);
            if (y >= h) { v.x &= 0xff000000u; v.y &= 0xff000000u; v.z &= 0xff000000u; v.w &= 0xff000000u; }
        } else {
            const uint32_t e = reinterpret_cast<const uint32_t*>(row)[w - 1] & 0xff000000u;
            v = make_uint4(e, e, e, e);
        }
    } else if (x < w && y < h) {
        if (PX == RIFE_HIP_PIX_RGB8) {
            typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
            u32x3 q;
            __builtin_memcpy(&q, __builtin_assume_aligned(row + (size_t)x * 3, 4), 12);
            v.x = q.x & 0xffffffu; v.y = (q.x >> 24) | ((q.y & 0xffffu) << 8); v.z = (q.y >> 16) | ((q.z & 0xffu) << 16); v.w = q.z >> 8;
        } else if (PX == RIFE_HIP_PIX_RGB10_U16) {
            uint2 q[3];
            __builtin_memcpy(q, __builtin_assume_aligned(row + (size_t)x * 6, 8), 24);
            v.x = pack10(q[0].x & 0xffffu, q[0].x >> 16, q[0].y & 0xffffu);
            v.y = pack10(q[0].y >> 16, q[1].x & 0xffffu, q[1].x >> 16);
            v.z = pack10(q[1].y & 0xffffu, q[1].y >> 16, q[2].x & 0xffffu);
            v.w = pack10(q[2].x >> 16, q[2].y & 0xffffu, q[2].y >> 16);
        } else {
            v = *reinterpret_cast<const uint4*>(row + (size_t)x * 4);
            v.x &= 0x3fffffffu; v.y &= 0x3fffffffu; v.z &= 0x3fffffffu; v.w &= 0x3fffffffu;
        }
    }
    *reinterpret_cast<uint4*>(out + (size_t)y * wp + x) = v;
}
// the access width of the wide form: RGB8 12 bytes as dwords, RGB10_U16 24 bytes as 8-byte words, the dword formats 16 bytes (the tight kernels' rule)
static inline unsigned preproc_wide_align(int pixfmt) { return pixfmt == RIFE_HIP_PIX_RGB8 ? 4u : pixfmt == RIFE_HIP_PIX_RGB10_U16 ? 8u : 16u; }
static inline bool planes_preproc_wide(const PlaneSet& s, int w, int pixfmt) { return (w & 3) == 0 && planes_aligned(s, 0, preproc_wide_align(pixfmt)); }

// ---- in, 4:2:0, scalar: one 2x2 block of the PADDED frame per lane; grid ((wp / 2 + 255) / 256, hp / 2) ----
template <bool PLANAR, int DEPTH>
__global__ void k_preproc_yuv_pitch(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2, y = blockIdx.y * 2;
    if (x >= wp) return;
    uint2 r0 = make_uint2(0u, 0u), r1 = make_uint2(0u, 0u);
    if (x < w && y < h) {
        const T* c0 = reinterpret_cast<const T*>(s.p[1] + (size_t)(y / 2) * s.pitch[1]);
        int cb, cr;
        if (PLANAR) {
            const T* c1 = reinterpret_cast<const T*>(s.p[2] + (size_t)(y / 2) * s.pitch[2]);
            cb = yuv_code<PLANAR, DEPTH>(c0[x / 2]); cr = yuv_code<PLANAR, DEPTH>(c1[x / 2]);
        } else { cb = yuv_code<PLANAR, DEPTH>(c0[x]); cr = yuv_code<PLANAR, DEPTH>(c0[x + 1]); }      // x is even: the pair of block x / 2
        const T* p = reinterpret_cast<const T*>(s.p[0] + (size_t)y * s.pitch[0]) + x;
        r0.x = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(p[0]), cb, cr);
        if (x + 1 < w) r0.y = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(p[1]), cb, cr);
        if (y + 1 < h) {
            const T* q = reinterpret_cast<const T*>(s.p[0] + (size_t)(y + 1) * s.pitch[0]) + x;
            r1.x = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(q[0]), cb, cr);
            if (x + 1 < w) r1.y = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(q[1]), cb, cr);
        }
    }
    *reinterpret_cast<uint2*>(out + (size_t)y * wp + x) = r0;                 // wp, hp are multiples of 32: rows y and y + 1 exist, x is even
    *reinterpret_cast<uint2*>(out + (size_t)(y + 1) * wp + x) = r1;
}
// ---- in, 4:2:0, x8: eight columns x two rows of the PADDED frame per lane (w % 8 == 0, aligned planes and pitches); grid ((wp / 8 + 255) / 256, hp / 2) ----
template <bool PLANAR, int DEPTH>
__global__ void k_preproc_yuv_pitch_x8(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y * 2;
    if (x >= wp) return;
    uint32_t o[2][8];
    for (int i = 0; i < 8; i++) o[0][i] = o[1][i] = 0u;
    if (x < w && y < h) {
        int cb[4], cr[4], yv[8];
        const T* c0 = reinterpret_cast<const T*>(s.p[1] + (size_t)(y / 2) * s.pitch[1]);
        if (PLANAR) {
            const T* c1 = reinterpret_cast<const T*>(s.p[2] + (size_t)(y / 2) * s.pitch[2]);
            yuv_load4<PLANAR, DEPTH>(c0 + x / 2, cb);
            yuv_load4<PLANAR, DEPTH>(c1 + x / 2, cr);
        } else {
            int uv[8];
            yuv_load8<PLANAR, DEPTH>(c0 + x, uv);
            for (int i = 0; i < 4; i++) { cb[i] = uv[2 * i]; cr[i] = uv[2 * i + 1]; }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if (y + r >= h) break;
            yuv_load8<PLANAR, DEPTH>(reinterpret_cast<const T*>(s.p[0] + (size_t)(y + r) * s.pitch[0]) + x, yv);
            for (int i = 0; i < 8; i++) o[r][i] = yuv_to_pk10(k, yv[i], cb[i / 2], cr[i / 2]);
        }
    }
    for (int r = 0; r < 2; r++) {
        uint4* d = reinterpret_cast<uint4*>(out + (size_t)(y + r) * wp + x);
        d[0] = make_uint4(o[r][0], o[r][1], o[r][2], o[r][3]);
        d[1] = make_uint4(o[r][4], o[r][5], o[r][6], o[r][7]);
    }
}

// ---- out, 4:2:0, scalar: one 2x2 block of the frame per lane; rgb = A2B10G10R10, tight (pitch w); grid ((cw + 255) / 256, ch) ----
template <bool PLANAR, int DEPTH>
__global__ void k_postproc_yuv_pitch(const uint32_t* __restrict__ rgb, int w, int h, PlaneSet d, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= cw || by >= ch) return;
    const int x = 2 * bx, y = 2 * by;                                            // inside the frame: bx < cw, by < ch
    const bool right = x + 1 < w, below = y + 1 < h;
    const uint32_t* s = rgb + (size_t)y * w + x;
    T* p = reinterpret_cast<T*>(d.p[0] + (size_t)y * d.pitch[0]) + x;
    int sr = 0, sg = 0, sb = 0;
    p[0] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[0], sr, sg, sb));
    if (right) p[1] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[1], sr, sg, sb));
    if (below) {
        T* q = reinterpret_cast<T*>(d.p[0] + (size_t)(y + 1) * d.pitch[0]) + x;
        q[0] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[w], sr, sg, sb));
        if (right) q[1] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[w + 1], sr, sg, sb));
    }
    int cb, cr;
    yuv_chroma<DEPTH>(k, sr, sg, sb, (right ? 1 : 0) + (below ? 1 : 0), cb, cr);
    T* c0 = reinterpret_cast<T*>(d.p[1] + (size_t)by * d.pitch[1]);
    if (PLANAR) {
        T* c1 = reinterpret_cast<T*>(d.p[2] + (size_t)by * d.pitch[2]);
        c0[bx] = (T)yuv_sample<PLANAR, DEPTH>(cb); c1[bx] = (T)yuv_sample<PLANAR, DEPTH>(cr);
    } else { c0[2 * bx] = (T)yuv_sample<PLANAR, DEPTH>(cb); c0[2 * bx + 1] = (T)yuv_sample<PLANAR, DEPTH>(cr); }
}
// ---- out, 4:2:0, x8: eight columns x two rows per lane (w % 8 == 0, aligned planes and pitches); grid ((w / 8 + 255) / 256, ch) ----
template <bool PLANAR, int DEPTH>
__global__ void k_postproc_yuv_pitch_x8(const uint32_t* __restrict__ rgb, int w, int h, PlaneSet d, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int ch = (h + 1) / 2;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, by = blockIdx.y, y = 2 * by;
    if (x >= w || by >= ch) return;
    const int rows = y + 1 < h ? 2 : 1;
    int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r >= rows) break;
        const uint4* s = reinterpret_cast<const uint4*>(rgb + (size_t)(y + r) * w + x);
        const uint4 a = s[0], b = s[1];
        const uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        int yv[8];
        for (int i = 0; i < 8; i++) yv[i] = yuv_luma<DEPTH>(k, px[i], sr[i / 2], sg[i / 2], sb[i / 2]);
        yuv_store8<PLANAR, DEPTH>(reinterpret_cast<T*>(d.p[0] + (size_t)(y + r) * d.pitch[0]) + x, yv);
    }
    int cb[4], cr[4];
    for (int i = 0; i < 4; i++) yuv_chroma<DEPTH>(k, sr[i], sg[i], sb[i], rows, cb[i], cr[i]);      // lg = 1 + (rows - 1): every block is two columns wide
    T* c0 = reinterpret_cast<T*>(d.p[1] + (size_t)by * d.pitch[1]);
    if (PLANAR) {
        T* c1 = reinterpret_cast<T*>(d.p[2] + (size_t)by * d.pitch[2]);
        yuv_store4<PLANAR, DEPTH>(c0 + x / 2, cb);
        yuv_store4<PLANAR, DEPTH>(c1 + x / 2, cr);
    } else {
        int uv[8];
        for (int i = 0; i < 4; i++) { uv[2 * i] = cb[i]; uv[2 * i + 1] = cr[i]; }
        yuv_store8<PLANAR, DEPTH>(c0 + x, uv);
    }
}
// the x8 forms load / store 8 luma samples (8 bytes at depth 8, 16 at depth 10) and 4 samples of each planar chroma plane (4 / 8 bytes) or 8 interleaved ones
static inline bool planes_yuv_x8(const PlaneSet& s, int w, int fmt) {
    const unsigned a = yuv_depth(fmt) == 10 ? 16u : 8u;
    if ((w & 7) != 0 || !planes_aligned(s, 0, a)) return false;
    return yuv_planar(fmt) ? planes_aligned(s, 1, a / 2) && planes_aligned(s, 2, a / 2) : planes_aligned(s, 1, a);
}

// ---- out, RGB formats: the tight frame the quantising kernels wrote (row_bytes per row) -> the caller's plane; grid ((units + 255) / 256, h) ----
template <typename T>
__global__ void k_store_rows(const uint8_t* __restrict__ src, size_t row_bytes, uint8_t* __restrict__ dst, size_t pitch) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (i * sizeof(T) >= row_bytes) return;                                   // row_bytes is a multiple of sizeof(T): nothing past the row's last byte is written
    reinterpret_cast<T*>(dst + y * pitch)[i] = reinterpret_cast<const T*>(src + y * row_bytes)[i];
}
// timestep 0 / 1: what the canonical copy of a format does to a sample (host and device state it from this one enum)
enum CanonMode { CANON_BYTES = 0,      // the 8-bit formats: bytes unchanged (2-D copies, no kernel)
                 CANON_U16_CLAMP,      // RGB10_U16, I420P10, I422P10, I444P10: u16 clamped to 1023
                 CANON_PACKED_ALPHA,   // A2B10G10R10: dword | alpha bits 3
                 CANON_P010,           // P010: low six bits cleared
                 CANON_HALF,           // RGBPH: the half sample of its code, from10(to10(v)) (planar_rgb.h)
                 CANON_FLOAT };        // RGBPF: the float sample of its code
static inline size_t canon_elem(CanonMode mode) { return (mode == CANON_PACKED_ALPHA || mode == CANON_FLOAT) ? 4 : 2; }      // bytes of the unit a mode works on (CANON_BYTES: none)
static inline CanonMode canon_mode(int pixfmt) {
    const int b = pixfmt & 0xff;
    if (b == RIFE_HIP_PIX_RGBPH) return CANON_HALF;
    if (b == RIFE_HIP_PIX_RGBPF) return CANON_FLOAT;
    return (b == RIFE_HIP_PIX_RGBP10 || b == RIFE_HIP_PIX_RGB10_U16 || b == RIFE_HIP_PIX_I420P10 || b == RIFE_HIP_PIX_I422P10 || b == RIFE_HIP_PIX_I444P10) ? CANON_U16_CLAMP : b == RIFE_HIP_PIX_A2B10G10R10 ? CANON_PACKED_ALPHA : b == RIFE_HIP_PIX_P010 ? CANON_P010 : CANON_BYTES;
}
// strided in and out, one element per lane; n = elements per row; grid ((n + 255) / 256, rows).  MODE != CANON_BYTES
template <CanonMode MODE>
__global__ void k_canon_rows(const uint8_t* __restrict__ src, size_t spitch, uint8_t* __restrict__ dst, size_t dpitch, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t y = blockIdx.y;
    if (i >= n) return;
    if (MODE == CANON_PACKED_ALPHA) reinterpret_cast<uint32_t*>(dst + y * dpitch)[i] = reinterpret_cast<const uint32_t*>(src + y * spitch)[i] | 0xc0000000u;
    else if (MODE == CANON_FLOAT) reinterpret_cast<float*>(dst + y * dpitch)[i] = rgbp_canon<float>(reinterpret_cast<const float*>(src + y * spitch)[i]);
    else if (MODE == CANON_HALF) reinterpret_cast<_Float16*>(dst + y * dpitch)[i] = rgbp_canon<_Float16>(reinterpret_cast<const _Float16*>(src + y * spitch)[i]);
    else {
        const uint32_t v = reinterpret_cast<const uint16_t*>(src + y * spitch)[i];
        reinterpret_cast<uint16_t*>(dst + y * dpitch)[i] = (uint16_t)(MODE == CANON_P010 ? (v & 0xffc0u) : min(v, 1023u));
    }
}
// the same on the host: one row of rb bytes (src == dst is fine: element by element)
static inline void canon_row_host(CanonMode mode, const uint8_t* s, uint8_t* d, size_t rb) {
    if (mode == CANON_BYTES) std::memmove(d, s, rb);
    else if (mode == CANON_PACKED_ALPHA) { const uint32_t* a = reinterpret_cast<const uint32_t*>(s); uint32_t* b = reinterpret_cast<uint32_t*>(d); for (size_t i = 0; i < rb / 4; i++) b[i] = a[i] | 0xc0000000u; }
    else if (mode == CANON_FLOAT) { const float* a = reinterpret_cast<const float*>(s); float* b = reinterpret_cast<float*>(d); for (size_t i = 0; i < rb / 4; i++) b[i] = rgbp_canon<float>(a[i]); }
    else if (mode == CANON_HALF) { const _Float16* a = reinterpret_cast<const _Float16*>(s); _Float16* b = reinterpret_cast<_Float16*>(d); for (size_t i = 0; i < rb / 2; i++) b[i] = rgbp_canon<_Float16>(a[i]); }
    else { const uint16_t* a = reinterpret_cast<const uint16_t*>(s); uint16_t* b = reinterpret_cast<uint16_t*>(d); for (size_t i = 0; i < rb / 2; i++) b[i] = mode == CANON_P010 ? (uint16_t)(a[i] & 0xffc0u) : (uint16_t)(a[i] < 1023 ? a[i] : 1023); }
}
template <CanonMode MODE>
static inline void launch_canon_rows_m(hipStream_t st, const uint8_t* s, size_t sp, uint8_t* d, size_t dp, int n, int rows) {
    hipLaunchKernelGGL(k_canon_rows<MODE>, dim3((n + 255) / 256, rows), dim3(256), 0, st, s, sp, d, dp, n);
}
// rows x rb bytes, strided both ways; mode != CANON_BYTES
static inline void launch_canon_rows(hipStream_t st, CanonMode mode, const uint8_t* s, size_t sp, uint8_t* d, size_t dp, size_t rb, int rows) {
    const int n = (int)(rb / canon_elem(mode));
    if (mode == CANON_U16_CLAMP) launch_canon_rows_m<CANON_U16_CLAMP>(st, s, sp, d, dp, n, rows);
    else if (mode == CANON_PACKED_ALPHA) launch_canon_rows_m<CANON_PACKED_ALPHA>(st, s, sp, d, dp, n, rows);
    else if (mode == CANON_P010) launch_canon_rows_m<CANON_P010>(st, s, sp, d, dp, n, rows);
    else if (mode == CANON_HALF) launch_canon_rows_m<CANON_HALF>(st, s, sp, d, dp, n, rows);
    else launch_canon_rows_m<CANON_FLOAT>(st, s, sp, d, dp, n, rows);
}

// ---- host side.  force_scalar: the single-kernel tests run both forms on one frame ----
static inline void launch_preproc_planes(hipStream_t st, const PlaneSet& s, int w, int h, uint32_t* out, int wp, int hp, int pixfmt, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    if (rgbp_fmt(fmt)) { launch_preproc_rgbp(st, s, w, h, out, wp, hp, pixfmt, force_scalar); return; }      // planar RGB: planar_rgb.h, one kernel set for tight and pitched planes
    if (fmt >= RIFE_HIP_PIX_I422) { launch_preproc_yuvc(st, s, w, h, out, wp, hp, pixfmt, force_scalar); return; }      // 4:2:2 / 4:4:4: yuv.h, one kernel set for tight and pitched planes
    if (fmt >= RIFE_HIP_PIX_NV12) {
        const YuvCsp k = yuv_csp(pixfmt & ~0xff, yuv_depth(fmt));
        const bool x8 = !force_scalar && planes_yuv_x8(s, w, fmt);
        const dim3 g = x8 ? dim3((wp / 8 + 255) / 256, hp / 2) : dim3((wp / 2 + 255) / 256, hp / 2);
#define RIFE_PL_IN(P, D) do { if (x8) hipLaunchKernelGGL((k_preproc_yuv_pitch_x8<P, D>), g, dim3(256), 0, st, s, w, h, out, wp, hp, k); \
                              else hipLaunchKernelGGL((k_preproc_yuv_pitch<P, D>), g, dim3(256), 0, st, s, w, h, out, wp, hp, k); } while (0)
        if (fmt == RIFE_HIP_PIX_NV12) RIFE_PL_IN(false, 8); else if (fmt == RIFE_HIP_PIX_I420) RIFE_PL_IN(true, 8); else if (fmt == RIFE_HIP_PIX_P010) RIFE_PL_IN(false, 10); else RIFE_PL_IN(true, 10);
#undef RIFE_PL_IN
        return;
    }
    const bool wide = !force_scalar && planes_preproc_wide(s, w, fmt);
    const dim3 g = wide ? dim3((wp / 4 + 255) / 256, hp) : dim3((wp + 255) / 256, hp);
#define RIFE_PL_RGB(PX) do { if (wide) hipLaunchKernelGGL((k_preproc_pitch<PX, true>), g, dim3(256), 0, st, s.p[0], s.pitch[0], w, h, out, wp, hp); \
                             else hipLaunchKernelGGL((k_preproc_pitch<PX, false>), g, dim3(256), 0, st, s.p[0], s.pitch[0], w, h, out, wp, hp); } while (0)
    if (fmt == RIFE_HIP_PIX_RGB10_U16) RIFE_PL_RGB(RIFE_HIP_PIX_RGB10_U16); else if (fmt == RIFE_HIP_PIX_A2B10G10R10) RIFE_PL_RGB(RIFE_HIP_PIX_A2B10G10R10);
    else if (fmt == RIFE_HIP_PIX_RGBA8) RIFE_PL_RGB(RIFE_HIP_PIX_RGBA8); else RIFE_PL_RGB(RIFE_HIP_PIX_RGB8);
#undef RIFE_PL_RGB
}
// (YUV and planar RGB: every format whose output is converted from the pass's A2B10G10R10 frame)
static inline void launch_postproc_yuv_planes(hipStream_t st, const uint32_t* rgb, int w, int h, const PlaneSet& d, int pixfmt, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    if (rgbp_fmt(fmt)) { launch_postproc_rgbp(st, rgb, w, h, d, pixfmt, force_scalar); return; }
    if (fmt >= RIFE_HIP_PIX_I422) { launch_postproc_yuvc(st, rgb, w, h, d, pixfmt, force_scalar); return; }
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, yuv_depth(fmt));
    const bool x8 = !force_scalar && planes_yuv_x8(d, w, fmt);
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const dim3 g = x8 ? dim3((w / 8 + 255) / 256, ch) : dim3((cw + 255) / 256, ch);
#define RIFE_PL_OUT(P, D) do { if (x8) hipLaunchKernelGGL((k_postproc_yuv_pitch_x8<P, D>), g, dim3(256), 0, st, rgb, w, h, d, k); \
                               else hipLaunchKernelGGL((k_postproc_yuv_pitch<P, D>), g, dim3(256), 0, st, rgb, w, h, d, k); } while (0)
    if (fmt == RIFE_HIP_PIX_NV12) RIFE_PL_OUT(false, 8); else if (fmt == RIFE_HIP_PIX_I420) RIFE_PL_OUT(true, 8); else if (fmt == RIFE_HIP_PIX_P010) RIFE_PL_OUT(false, 10); else RIFE_PL_OUT(true, 10);
#undef RIFE_PL_OUT
}
// the widest unit (16, 4, 2, 1 bytes) that divides row_bytes and to which both frames and the pitch are aligned; `elem` (the format's element size) always qualifies
static inline void launch_store_rows(hipStream_t st, const uint8_t* tight, size_t row_bytes, int h, uint8_t* dst, size_t pitch, int elem, bool force_scalar = false) {
    const uintptr_t m = reinterpret_cast<uintptr_t>(dst) | pitch | reinterpret_cast<uintptr_t>(tight) | row_bytes;
    const int unit = force_scalar ? elem : (m & 15) == 0 ? 16 : (m & 3) == 0 ? 4 : (m & 1) == 0 ? 2 : 1;
    const dim3 g((unsigned)((row_bytes / unit + 255) / 256), h);
    if (unit == 16) hipLaunchKernelGGL(k_store_rows<uint4>, g, dim3(256), 0, st, tight, row_bytes, dst, pitch);
    else if (unit == 4) hipLaunchKernelGGL(k_store_rows<uint32_t>, g, dim3(256), 0, st, tight, row_bytes, dst, pitch);
    else if (unit == 2) hipLaunchKernelGGL(k_store_rows<uint16_t>, g, dim3(256), 0, st, tight, row_bytes, dst, pitch);
    else hipLaunchKernelGGL(k_store_rows<uint8_t>, g, dim3(256), 0, st, tight, row_bytes, dst, pitch);
}
// the three images of one call, as run_v4 takes them
struct PlaneIO {
    PlaneSet in0, in1, out;
};

}  // namespace rife
