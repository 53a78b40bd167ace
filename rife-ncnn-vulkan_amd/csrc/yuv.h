// 4:2:0 Y'CbCr at the frame boundary (include/rife_hip.h RIFE_HIP_PIX_NV12 / I420 / P010 / I420P10): the two streaming kernels that stand between the caller's
// planes and the depth-10 schedule, and the integer colour conversion they share.  tests/yuv_ref.py states the same arithmetic in numpy; the two agree bit for bit.
//   k_preproc_yuv<PLANAR, DEPTH>   the caller's planes -> resident 10:10:10 dwords (img0 / img1), zero-padded: replaces the RGB pre-processing for these formats
//   k_postproc_yuv<PLANAR, DEPTH>  the pass's A2B10G10R10 frame (tight, pitch w) -> the caller's planes, chroma from the 2x2 sum
// Each has a scalar form (one 2x2 block per lane, element loads and stores: any size, any element-aligned pointer) and an x8 form (a run of four 2x2 blocks per
// lane, dword and wider accesses: w % 8 == 0 and an 8- / 16-byte aligned frame, which makes every plane and every row start aligned).  The host picks the form.
// 4:2:2 and 4:4:4 (RIFE_HIP_PIX_I422 .. I444P10, planar only) have sibling kernels below: the same per-pixel device functions on 2x1 / 1x1 blocks.
//   k_preproc_yuvc<SUBX, DEPTH> / _x8    Y, Cb, Cr planes -> resident 10:10:10 dwords; SUBX = 1: a chroma row is (w + 1) / 2 samples (4:2:2), 0: w samples (4:4:4)
//   k_postproc_yuvc<SUBX, DEPTH> / _x8   the pass's tight A2B10G10R10 frame -> Y, Cb, Cr planes, chroma from the 2x1 sum or the pixel itself
// They take their planes as a PlaneSet (pointer and pitch per plane), so ONE set serves tight frames (yuv_tight_planes) and the caller's pitched planes (planes.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "../../include/rife_hip.h"

namespace rife {

// one frame's planes as the kernels take them (pitches in bytes; entries the format does not use are null / 0)
struct PlaneSet {
    uint8_t* p[3];
    size_t pitch[3];
};
static inline bool planes_aligned(const PlaneSet& s, int p, unsigned a) { return ((reinterpret_cast<uintptr_t>(s.p[p]) | s.pitch[p]) & (a - 1)) == 0; }

// Q16 coefficients of both directions and the offsets, in codes of the format's depth (tests/yuv_ref.py coefs())
struct YuvCsp {
    int yoff, coff;
    int iy, irv, igu, igv, ibu;                                   // in:  R = iy Y' + irv Cr', G = iy Y' + igu Cb' + igv Cr', B = iy Y' + ibu Cb'   (' = offset removed)
    int oyr, oyg, oyb, our, oug, oub, ovr, ovg, ovb;              // out: Y = oy . RGB, Cb = ou . RGB, Cr = ov . RGB, then the offsets
};
static inline int yuv_q16(double x) { return (int)std::floor(x * 65536.0 + 0.5); }
// the matrix's real coefficients times 1023 / range (in) and range / 1023 (out), rounded to Q16; csp = the colour bits of a pixfmt, depth 8 or 10
static inline YuvCsp yuv_csp(int csp, int depth) {
    const int m = (csp >> 8) & 15;
    const double kr = m == 1 ? 0.299 : m == 2 ? 0.2627 : 0.2126, kb = m == 1 ? 0.114 : m == 2 ? 0.0593 : 0.0722;
    const double kg = 1.0 - kr - kb;
    const int s = depth == 10 ? 4 : 1;
    const bool full = (csp & (1 << 12)) != 0;
    const int yr = full ? 255 * s + (s - 1) : 219 * s, cr = full ? 255 * s + (s - 1) : 224 * s;
    const double gi = 1023.0 / yr, gc = 1023.0 / cr, go = yr / 1023.0, gco = cr / 1023.0;
    YuvCsp k;
    k.yoff = full ? 0 : 16 * s; k.coff = 128 * s;
    k.iy = yuv_q16(gi); k.irv = yuv_q16(2 * (1 - kr) * gc); k.igu = yuv_q16(-2 * kb * (1 - kb) / kg * gc); k.igv = yuv_q16(-2 * kr * (1 - kr) / kg * gc);
    k.ibu = yuv_q16(2 * (1 - kb) * gc);
    k.oyr = yuv_q16(kr * go); k.oyg = yuv_q16(kg * go); k.oyb = yuv_q16(kb * go);
    k.our = yuv_q16(-kr / (2 * (1 - kb)) * gco); k.oug = yuv_q16(-kg / (2 * (1 - kb)) * gco); k.oub = yuv_q16(0.5 * gco);
    k.ovr = yuv_q16(0.5 * gco); k.ovg = yuv_q16(-kg / (2 * (1 - kr)) * gco); k.ovb = yuv_q16(-kb / (2 * (1 - kr)) * gco);
    return k;
}

template <int DEPTH> struct YuvElem { typedef uint8_t T; };
template <> struct YuvElem<10> { typedef uint16_t T; };

// a stored sample <-> its code: P010 (NV12 layout at depth 10) keeps the code in the HIGH ten bits; an I420P10 sample above 1023 is read as 1023 (like RGB10_U16)
template <bool PLANAR, int DEPTH>
__host__ __device__ __forceinline__ int yuv_code(uint32_t v) { return DEPTH == 8 ? (int)v : PLANAR ? (int)(v < 1023u ? v : 1023u) : (int)(v >> 6); }
template <bool PLANAR, int DEPTH>
__host__ __device__ __forceinline__ uint32_t yuv_sample(int code) { return (DEPTH == 10 && !PLANAR) ? (uint32_t)code << 6 : (uint32_t)code; }

__host__ __device__ __forceinline__ int yuv_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// one pixel in: codes -> the resident 10:10:10 dword (arithmetic shifts of signed sums)
__host__ __device__ __forceinline__ uint32_t yuv_to_pk10(const YuvCsp& k, int y, int cb, int cr) {
    const int yy = k.iy * (y - k.yoff), u = cb - k.coff, v = cr - k.coff;
    const int r = yuv_clamp((yy + k.irv * v + 0x8000) >> 16, 1023);
    const int g = yuv_clamp((yy + k.igu * u + k.igv * v + 0x8000) >> 16, 1023);
    const int b = yuv_clamp((yy + k.ibu * u + 0x8000) >> 16, 1023);
    return (uint32_t)r | ((uint32_t)g << 10) | ((uint32_t)b << 20);
}
// one pixel out: luma of a 10:10:10 dword (the alpha bits are ignored); the pixel's codes are added to the block's sums
template <int DEPTH>
__host__ __device__ __forceinline__ int yuv_luma(const YuvCsp& k, uint32_t pk, int& sr, int& sg, int& sb) {
    const int r = pk & 1023, g = (pk >> 10) & 1023, b = (pk >> 20) & 1023;
    sr += r; sg += g; sb += b;
    return yuv_clamp(((k.oyr * r + k.oyg * g + k.oyb * b + 0x8000) >> 16) + k.yoff, DEPTH == 10 ? 1023 : 255);
}
// chroma of a block from the sums over its 1 << lg pixels inside the frame
template <int DEPTH>
__host__ __device__ __forceinline__ void yuv_chroma(const YuvCsp& k, int sr, int sg, int sb, int lg, int& cb, int& cr) {
    const int rnd = 0x8000 << lg, sh = 16 + lg;
    cb = yuv_clamp(((k.our * sr + k.oug * sg + k.oub * sb + rnd) >> sh) + k.coff, DEPTH == 10 ? 1023 : 255);
    cr = yuv_clamp(((k.ovr * sr + k.ovg * sg + k.ovb * sb + rnd) >> sh) + k.coff, DEPTH == 10 ? 1023 : 255);
}

// ---- in, scalar: one 2x2 block of the PADDED frame per lane; grid ((wp / 2 + 255) / 256, hp / 2) ----
template <bool PLANAR, int DEPTH>
__global__ void k_preproc_yuv(const void* __restrict__ frame, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2, y = blockIdx.y * 2;
    if (x >= wp) return;
    uint2 r0 = make_uint2(0u, 0u), r1 = make_uint2(0u, 0u);
    if (x < w && y < h) {
        const int cw = (w + 1) / 2, ch = (h + 1) / 2;
        const T* Y = static_cast<const T*>(frame);
        const T* C = Y + (size_t)w * h;
        const size_t ci = (size_t)(y / 2) * cw + x / 2;
        const int cb = yuv_code<PLANAR, DEPTH>(PLANAR ? C[ci] : C[2 * ci]);
        const int cr = yuv_code<PLANAR, DEPTH>(PLANAR ? C[(size_t)cw * ch + ci] : C[2 * ci + 1]);
        const T* p = Y + (size_t)y * w + x;
        r0.x = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(p[0]), cb, cr);
        if (x + 1 < w) r0.y = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(p[1]), cb, cr);
        if (y + 1 < h) {
            r1.x = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(p[w]), cb, cr);
            if (x + 1 < w) r1.y = yuv_to_pk10(k, yuv_code<PLANAR, DEPTH>(p[w + 1]), cb, cr);
        }
    }
    *reinterpret_cast<uint2*>(out + (size_t)y * wp + x) = r0;                 // wp, hp are multiples of 32: rows y and y + 1 exist, x is even
    *reinterpret_cast<uint2*>(out + (size_t)(y + 1) * wp + x) = r1;
}

// eight consecutive samples from an aligned address (8 bytes at depth 8, 16 at depth 10) / four (4 bytes, 8 bytes), as codes
template <bool PLANAR, int DEPTH>
__device__ __forceinline__ void yuv_load8(const typename YuvElem<DEPTH>::T* p, int* c) {
    if (DEPTH == 8) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        for (int i = 0; i < 4; i++) { c[i] = (q.x >> (8 * i)) & 255; c[4 + i] = (q.y >> (8 * i)) & 255; }
    } else {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        for (int i = 0; i < 4; i++) { c[2 * i] = yuv_code<PLANAR, DEPTH>(d[i] & 0xffffu); c[2 * i + 1] = yuv_code<PLANAR, DEPTH>(d[i] >> 16); }
    }
}
template <bool PLANAR, int DEPTH>
__device__ __forceinline__ void yuv_load4(const typename YuvElem<DEPTH>::T* p, int* c) {
    if (DEPTH == 8) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
        for (int i = 0; i < 4; i++) c[i] = (q >> (8 * i)) & 255;
    } else {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        c[0] = yuv_code<PLANAR, DEPTH>(q.x & 0xffffu); c[1] = yuv_code<PLANAR, DEPTH>(q.x >> 16);
        c[2] = yuv_code<PLANAR, DEPTH>(q.y & 0xffffu); c[3] = yuv_code<PLANAR, DEPTH>(q.y >> 16);
    }
}
// ---- in, x8: eight columns x two rows of the PADDED frame per lane (w % 8 == 0, aligned frame); grid ((wp / 8 + 255) / 256, hp / 2) ----
template <bool PLANAR, int DEPTH>
__global__ void k_preproc_yuv_x8(const void* __restrict__ frame, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y * 2;
    if (x >= wp) return;
    uint32_t o[2][8];
    for (int i = 0; i < 8; i++) o[0][i] = o[1][i] = 0u;
    if (x < w && y < h) {
        const int cw = w / 2, ch = (h + 1) / 2;
        const T* Y = static_cast<const T*>(frame);
        const T* C = Y + (size_t)w * h;
        int cb[4], cr[4], yv[8];
        if (PLANAR) {
            const size_t ci = (size_t)(y / 2) * cw + x / 2;
            yuv_load4<PLANAR, DEPTH>(C + ci, cb);
            yuv_load4<PLANAR, DEPTH>(C + (size_t)cw * ch + ci, cr);
        } else {
            int uv[8];
            yuv_load8<PLANAR, DEPTH>(C + (size_t)(y / 2) * w + x, uv);
            for (int i = 0; i < 4; i++) { cb[i] = uv[2 * i]; cr[i] = uv[2 * i + 1]; }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if (y + r >= h) break;
            yuv_load8<PLANAR, DEPTH>(Y + (size_t)(y + r) * w + x, yv);
            for (int i = 0; i < 8; i++) o[r][i] = yuv_to_pk10(k, yv[i], cb[i / 2], cr[i / 2]);
        }
    }
    for (int r = 0; r < 2; r++) {
        uint4* d = reinterpret_cast<uint4*>(out + (size_t)(y + r) * wp + x);
        d[0] = make_uint4(o[r][0], o[r][1], o[r][2], o[r][3]);
        d[1] = make_uint4(o[r][4], o[r][5], o[r][6], o[r][7]);
    }
}

// ---- out, scalar: one 2x2 block of the frame per lane; rgb = A2B10G10R10, tight (pitch w); grid ((cw + 255) / 256, ch) ----
template <bool PLANAR, int DEPTH>
__global__ void k_postproc_yuv(const uint32_t* __restrict__ rgb, int w, int h, void* __restrict__ frame, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= cw || by >= ch) return;
    const int x = 2 * bx, y = 2 * by;                                            // inside the frame: bx < cw, by < ch
    const bool right = x + 1 < w, below = y + 1 < h;
    T* Y = static_cast<T*>(frame);
    T* C = Y + (size_t)w * h;
    const uint32_t* s = rgb + (size_t)y * w + x;
    T* p = Y + (size_t)y * w + x;
    int sr = 0, sg = 0, sb = 0;
    p[0] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[0], sr, sg, sb));
    if (right) p[1] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[1], sr, sg, sb));
    if (below) {
        p[w] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[w], sr, sg, sb));
        if (right) p[w + 1] = (T)yuv_sample<PLANAR, DEPTH>(yuv_luma<DEPTH>(k, s[w + 1], sr, sg, sb));
    }
    int cb, cr;
    yuv_chroma<DEPTH>(k, sr, sg, sb, (right ? 1 : 0) + (below ? 1 : 0), cb, cr);
    const size_t ci = (size_t)by * cw + bx;
    if (PLANAR) { C[ci] = (T)yuv_sample<PLANAR, DEPTH>(cb); C[(size_t)cw * ch + ci] = (T)yuv_sample<PLANAR, DEPTH>(cr); }
    else { C[2 * ci] = (T)yuv_sample<PLANAR, DEPTH>(cb); C[2 * ci + 1] = (T)yuv_sample<PLANAR, DEPTH>(cr); }
}

template <bool PLANAR, int DEPTH>
__device__ __forceinline__ void yuv_store8(typename YuvElem<DEPTH>::T* p, const int* c) {
    if (DEPTH == 8) {
        uint2 q = make_uint2(0u, 0u);
        for (int i = 0; i < 4; i++) { q.x |= (uint32_t)c[i] << (8 * i); q.y |= (uint32_t)c[4 + i] << (8 * i); }
        *reinterpret_cast<uint2*>(p) = q;
    } else {
        uint32_t d[4];
        for (int i = 0; i < 4; i++) d[i] = yuv_sample<PLANAR, DEPTH>(c[2 * i]) | (yuv_sample<PLANAR, DEPTH>(c[2 * i + 1]) << 16);
        *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]);
    }
}
template <bool PLANAR, int DEPTH>
__device__ __forceinline__ void yuv_store4(typename YuvElem<DEPTH>::T* p, const int* c) {
    if (DEPTH == 8) *reinterpret_cast<uint32_t*>(p) = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
    else *reinterpret_cast<uint2*>(p) = make_uint2(yuv_sample<PLANAR, DEPTH>(c[0]) | (yuv_sample<PLANAR, DEPTH>(c[1]) << 16),
                                                   yuv_sample<PLANAR, DEPTH>(c[2]) | (yuv_sample<PLANAR, DEPTH>(c[3]) << 16));
}
// ---- out, x8: eight columns x two rows per lane (w % 8 == 0, aligned frame); grid ((w / 8 + 255) / 256, ch) ----
template <bool PLANAR, int DEPTH>
__global__ void k_postproc_yuv_x8(const uint32_t* __restrict__ rgb, int w, int h, void* __restrict__ frame, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int cw = w / 2, ch = (h + 1) / 2;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, by = blockIdx.y, y = 2 * by;
    if (x >= w || by >= ch) return;
    const int rows = y + 1 < h ? 2 : 1;
    T* Y = static_cast<T*>(frame);
    T* C = Y + (size_t)w * h;
    int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r >= rows) break;
        const uint4* s = reinterpret_cast<const uint4*>(rgb + (size_t)(y + r) * w + x);
        const uint4 a = s[0], b = s[1];
        const uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        int yv[8];
        for (int i = 0; i < 8; i++) yv[i] = yuv_luma<DEPTH>(k, px[i], sr[i / 2], sg[i / 2], sb[i / 2]);
        yuv_store8<PLANAR, DEPTH>(Y + (size_t)(y + r) * w + x, yv);
    }
    int cb[4], cr[4];
    for (int i = 0; i < 4; i++) yuv_chroma<DEPTH>(k, sr[i], sg[i], sb[i], rows, cb[i], cr[i]);      // lg = 1 + (rows - 1): every block is two columns wide
    if (PLANAR) {
        const size_t ci = (size_t)by * cw + x / 2;
        yuv_store4<PLANAR, DEPTH>(C + ci, cb);
        yuv_store4<PLANAR, DEPTH>(C + (size_t)cw * ch + ci, cr);
    } else {
        int uv[8];
        for (int i = 0; i < 4; i++) { uv[2 * i] = cb[i]; uv[2 * i + 1] = cr[i]; }
        yuv_store8<PLANAR, DEPTH>(C + (size_t)by * w + x, uv);
    }
}

// ---- 4:2:2 / 4:4:4, planar.  Chroma planes have h rows; a pixel's chroma is the sample of its 2x1 block (SUBX = 1) or its own (SUBX = 0) ----
// in, scalar: two columns of one row of the PADDED frame per lane; grid ((wp / 2 + 255) / 256, hp)
template <int SUBX, int DEPTH>
__global__ void k_preproc_yuvc(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2, y = blockIdx.y;
    if (x >= wp) return;
    uint2 r = make_uint2(0u, 0u);
    if (x < w && y < h) {
        const T* p = reinterpret_cast<const T*>(s.p[0] + (size_t)y * s.pitch[0]) + x;
        const T* c0 = reinterpret_cast<const T*>(s.p[1] + (size_t)y * s.pitch[1]) + (SUBX ? x / 2 : x);
        const T* c1 = reinterpret_cast<const T*>(s.p[2] + (size_t)y * s.pitch[2]) + (SUBX ? x / 2 : x);
        int cb = yuv_code<true, DEPTH>(c0[0]), cr = yuv_code<true, DEPTH>(c1[0]);
        r.x = yuv_to_pk10(k, yuv_code<true, DEPTH>(p[0]), cb, cr);
        if (x + 1 < w) {
            if (!SUBX) { cb = yuv_code<true, DEPTH>(c0[1]); cr = yuv_code<true, DEPTH>(c1[1]); }
            r.y = yuv_to_pk10(k, yuv_code<true, DEPTH>(p[1]), cb, cr);
        }
    }
    *reinterpret_cast<uint2*>(out + (size_t)y * wp + x) = r;                  // wp is a multiple of 32, x is even
}
// in, x8: eight columns of one row of the PADDED frame per lane (w % 8 == 0, planes and pitches aligned to the loads); grid ((wp / 8 + 255) / 256, hp)
template <int SUBX, int DEPTH>
__global__ void k_preproc_yuvc_x8(PlaneSet s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y;
    if (x >= wp) return;
    uint32_t o[8];
    for (int i = 0; i < 8; i++) o[i] = 0u;
    if (x < w && y < h) {
        int cb[8], cr[8], yv[8];
        const T* c0 = reinterpret_cast<const T*>(s.p[1] + (size_t)y * s.pitch[1]);
        const T* c1 = reinterpret_cast<const T*>(s.p[2] + (size_t)y * s.pitch[2]);
        if (SUBX) { yuv_load4<true, DEPTH>(c0 + x / 2, cb); yuv_load4<true, DEPTH>(c1 + x / 2, cr); }
        else { yuv_load8<true, DEPTH>(c0 + x, cb); yuv_load8<true, DEPTH>(c1 + x, cr); }
        yuv_load8<true, DEPTH>(reinterpret_cast<const T*>(s.p[0] + (size_t)y * s.pitch[0]) + x, yv);
        for (int i = 0; i < 8; i++) o[i] = yuv_to_pk10(k, yv[i], cb[SUBX ? i / 2 : i], cr[SUBX ? i / 2 : i]);
    }
    uint4* d = reinterpret_cast<uint4*>(out + (size_t)y * wp + x);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
}
// out, scalar: two columns of one row of the frame per lane; rgb = A2B10G10R10, tight (pitch w); grid (((w + 1) / 2 + 255) / 256, h)
template <int SUBX, int DEPTH>
__global__ void k_postproc_yuvc(const uint32_t* __restrict__ rgb, int w, int h, PlaneSet d, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    const int x = 2 * bx;
    if (x >= w || y >= h) return;
    const bool right = x + 1 < w;
    const uint32_t* s = rgb + (size_t)y * w + x;
    T* p = reinterpret_cast<T*>(d.p[0] + (size_t)y * d.pitch[0]) + x;
    T* c0 = reinterpret_cast<T*>(d.p[1] + (size_t)y * d.pitch[1]) + (SUBX ? bx : x);
    T* c1 = reinterpret_cast<T*>(d.p[2] + (size_t)y * d.pitch[2]) + (SUBX ? bx : x);
    int sr = 0, sg = 0, sb = 0, cb, cr;
    p[0] = (T)yuv_sample<true, DEPTH>(yuv_luma<DEPTH>(k, s[0], sr, sg, sb));
    if (!SUBX) {
        yuv_chroma<DEPTH>(k, sr, sg, sb, 0, cb, cr);
        c0[0] = (T)yuv_sample<true, DEPTH>(cb); c1[0] = (T)yuv_sample<true, DEPTH>(cr);
        sr = sg = sb = 0;
    }
    if (right) p[1] = (T)yuv_sample<true, DEPTH>(yuv_luma<DEPTH>(k, s[1], sr, sg, sb));
    if (SUBX || right) {
        yuv_chroma<DEPTH>(k, sr, sg, sb, (SUBX && right) ? 1 : 0, cb, cr);
        c0[SUBX ? 0 : 1] = (T)yuv_sample<true, DEPTH>(cb); c1[SUBX ? 0 : 1] = (T)yuv_sample<true, DEPTH>(cr);
    }
}
// out, x8: eight columns of one row per lane (w % 8 == 0, planes and pitches aligned to the stores); grid ((w / 8 + 255) / 256, h)
template <int SUBX, int DEPTH>
__global__ void k_postproc_yuvc_x8(const uint32_t* __restrict__ rgb, int w, int h, PlaneSet d, YuvCsp k) {
    typedef typename YuvElem<DEPTH>::T T;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const uint4* s = reinterpret_cast<const uint4*>(rgb + (size_t)y * w + x);
    const uint4 a = s[0], b = s[1];
    const uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    int sr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int yv[8], cb[8], cr[8];
    for (int i = 0; i < 8; i++) { const int j = SUBX ? i / 2 : i; yv[i] = yuv_luma<DEPTH>(k, px[i], sr[j], sg[j], sb[j]); }
    yuv_store8<true, DEPTH>(reinterpret_cast<T*>(d.p[0] + (size_t)y * d.pitch[0]) + x, yv);
    for (int i = 0; i < (SUBX ? 4 : 8); i++) yuv_chroma<DEPTH>(k, sr[i], sg[i], sb[i], SUBX, cb[i], cr[i]);      // every block is inside the frame: n = 2 or 1
    T* c0 = reinterpret_cast<T*>(d.p[1] + (size_t)y * d.pitch[1]);
    T* c1 = reinterpret_cast<T*>(d.p[2] + (size_t)y * d.pitch[2]);
    if (SUBX) { yuv_store4<true, DEPTH>(c0 + x / 2, cb); yuv_store4<true, DEPTH>(c1 + x / 2, cr); }
    else { yuv_store8<true, DEPTH>(c0 + x, cb); yuv_store8<true, DEPTH>(c1 + x, cr); }
}

// timestep 0 / 1 at depth 10: the frame's samples as codes (P010: low six bits cleared; I420P10, I422P10, I444P10: clamped to 1023); n = samples of all three planes
template <bool PLANAR>
__global__ void k_canon_yuv10(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint16_t)yuv_sample<PLANAR, 10>(yuv_code<PLANAR, 10>(in[i]));
}

// host side: fmt = the format bits of a pixfmt (RIFE_HIP_PIX_NV12 .. I444P10 = 16 * class + 2 * (10 bits) + planar; class 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4), csp its colour bits.
// The 4:2:0 x8 forms need w % 8 == 0 and a frame aligned to 8 bytes (16 at depth 10): the planes follow each other at w * h elements, so that is what aligns every row of every plane.
static inline int yuv_class(int fmt) { return fmt >> 4; }
static inline bool yuv_planar(int fmt) { return (fmt & 1) != 0; }
static inline int yuv_depth(int fmt) { return (fmt & 2) ? 10 : 8; }
static inline bool yuv_x8_ok(const void* frame, int w, int fmt) { return (w & 7) == 0 && (reinterpret_cast<uintptr_t>(frame) & (yuv_depth(fmt) == 10 ? 15 : 7)) == 0; }

// 4:2:2 / 4:4:4: the planes of a tight frame (Y w x h, Cb and Cr cw x h one after the other)
static inline PlaneSet yuv_tight_planes(const void* frame, int w, int h, int fmt) {
    const size_t es = yuv_depth(fmt) == 10 ? 2 : 1, cw = yuv_class(fmt) == 2 ? ((size_t)w + 1) / 2 : (size_t)w;
    PlaneSet s;
    s.p[0] = static_cast<uint8_t*>(const_cast<void*>(frame)); s.pitch[0] = (size_t)w * es;
    s.p[1] = s.p[0] + (size_t)w * h * es; s.pitch[1] = cw * es;
    s.p[2] = s.p[1] + cw * h * es; s.pitch[2] = cw * es;
    return s;
}
// the x8 forms load / store 8 luma samples (8 bytes at depth 8, 16 at depth 10) and, per chroma plane, 4 samples (4:2:2: 4 / 8 bytes) or 8 (4:4:4: 8 / 16 bytes): every
// plane pointer and pitch is aligned to its own access.  A tight frame with w % 8 == 0 at an 8- / 16-byte aligned address qualifies: its 4:2:2 chroma rows are w / 2 samples,
// a multiple of the 4-sample access, and the chroma planes start w * h and w * h + (w / 2) * h samples in.
static inline bool yuvc_x8_ok(const PlaneSet& s, int w, int fmt) {
    const unsigned a = yuv_depth(fmt) == 10 ? 16u : 8u, ac = yuv_class(fmt) == 2 ? a / 2 : a;
    return (w & 7) == 0 && planes_aligned(s, 0, a) && planes_aligned(s, 1, ac) && planes_aligned(s, 2, ac);
}
static inline void launch_preproc_yuvc(hipStream_t st, const PlaneSet& s, int w, int h, uint32_t* out, int wp, int hp, int pixfmt, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, yuv_depth(fmt));
    const bool x8 = !force_scalar && yuvc_x8_ok(s, w, fmt);
    const dim3 g = x8 ? dim3((wp / 8 + 255) / 256, hp) : dim3((wp / 2 + 255) / 256, hp);
#define RIFE_YUVC_IN(S, D) do { if (x8) hipLaunchKernelGGL((k_preproc_yuvc_x8<S, D>), g, dim3(256), 0, st, s, w, h, out, wp, hp, k); \
                                else hipLaunchKernelGGL((k_preproc_yuvc<S, D>), g, dim3(256), 0, st, s, w, h, out, wp, hp, k); } while (0)
    if (fmt == RIFE_HIP_PIX_I422) RIFE_YUVC_IN(1, 8); else if (fmt == RIFE_HIP_PIX_I422P10) RIFE_YUVC_IN(1, 10); else if (fmt == RIFE_HIP_PIX_I444) RIFE_YUVC_IN(0, 8); else RIFE_YUVC_IN(0, 10);
#undef RIFE_YUVC_IN
}
static inline void launch_postproc_yuvc(hipStream_t st, const uint32_t* rgb, int w, int h, const PlaneSet& d, int pixfmt, bool force_scalar = false) {
    const int fmt = pixfmt & 0xff;
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, yuv_depth(fmt));
    const bool x8 = !force_scalar && yuvc_x8_ok(d, w, fmt);
    const dim3 g = x8 ? dim3((w / 8 + 255) / 256, h) : dim3(((w + 1) / 2 + 255) / 256, h);
#define RIFE_YUVC_OUT(S, D) do { if (x8) hipLaunchKernelGGL((k_postproc_yuvc_x8<S, D>), g, dim3(256), 0, st, rgb, w, h, d, k); \
                                 else hipLaunchKernelGGL((k_postproc_yuvc<S, D>), g, dim3(256), 0, st, rgb, w, h, d, k); } while (0)
    if (fmt == RIFE_HIP_PIX_I422) RIFE_YUVC_OUT(1, 8); else if (fmt == RIFE_HIP_PIX_I422P10) RIFE_YUVC_OUT(1, 10); else if (fmt == RIFE_HIP_PIX_I444) RIFE_YUVC_OUT(0, 8); else RIFE_YUVC_OUT(0, 10);
#undef RIFE_YUVC_OUT
}

static inline void launch_preproc_yuv(hipStream_t st, const void* frame, int w, int h, uint32_t* out, int wp, int hp, int pixfmt) {
    const int fmt = pixfmt & 0xff;
    if (yuv_class(fmt) != 1) { launch_preproc_yuvc(st, yuv_tight_planes(frame, w, h, fmt), w, h, out, wp, hp, pixfmt); return; }
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, yuv_depth(fmt));
    const bool x8 = yuv_x8_ok(frame, w, fmt);
    const dim3 g = x8 ? dim3((wp / 8 + 255) / 256, hp / 2) : dim3((wp / 2 + 255) / 256, hp / 2);
#define RIFE_YUV_IN(P, D) do { if (x8) hipLaunchKernelGGL((k_preproc_yuv_x8<P, D>), g, dim3(256), 0, st, frame, w, h, out, wp, hp, k); \
                               else hipLaunchKernelGGL((k_preproc_yuv<P, D>), g, dim3(256), 0, st, frame, w, h, out, wp, hp, k); } while (0)
    if (fmt == RIFE_HIP_PIX_NV12) RIFE_YUV_IN(false, 8); else if (fmt == RIFE_HIP_PIX_I420) RIFE_YUV_IN(true, 8); else if (fmt == RIFE_HIP_PIX_P010) RIFE_YUV_IN(false, 10); else RIFE_YUV_IN(true, 10);
#undef RIFE_YUV_IN
}
static inline void launch_postproc_yuv(hipStream_t st, const uint32_t* rgb, int w, int h, void* frame, int pixfmt) {
    const int fmt = pixfmt & 0xff;
    if (yuv_class(fmt) != 1) { launch_postproc_yuvc(st, rgb, w, h, yuv_tight_planes(frame, w, h, fmt), pixfmt); return; }
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, yuv_depth(fmt));
    const bool x8 = yuv_x8_ok(frame, w, fmt);
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const dim3 g = x8 ? dim3((w / 8 + 255) / 256, ch) : dim3((cw + 255) / 256, ch);
#define RIFE_YUV_OUT(P, D) do { if (x8) hipLaunchKernelGGL((k_postproc_yuv_x8<P, D>), g, dim3(256), 0, st, rgb, w, h, frame, k); \
                                else hipLaunchKernelGGL((k_postproc_yuv<P, D>), g, dim3(256), 0, st, rgb, w, h, frame, k); } while (0)
    if (fmt == RIFE_HIP_PIX_NV12) RIFE_YUV_OUT(false, 8); else if (fmt == RIFE_HIP_PIX_I420) RIFE_YUV_OUT(true, 8); else if (fmt == RIFE_HIP_PIX_P010) RIFE_YUV_OUT(false, 10); else RIFE_YUV_OUT(true, 10);
#undef RIFE_YUV_OUT
}

}  // namespace rife
