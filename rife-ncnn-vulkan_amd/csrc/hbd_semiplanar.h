// hbd_semiplanar.h: semi-planar, MSB-aligned high-bit-depth surfaces at the frame boundary (include/rife_hip.h "semi-planar high bit depth": rife_hip_semiplanar_t) -
// a Y plane and ONE plane of interleaved Cb, Cr pairs, codes of `depth` bits in the HIGH bits of u16 (P010 / P012 / P016, P210 / P212 / P216).  sh = 16 - depth.
//   k_preproc_sp<SUBY> / _vec       the caller's pitched rows -> the resident 10:10:10 dwords the network estimates motion on: hbd_code(v >> sh) per sample (hbd.h), then
//                                   yuv_to_pk10, exactly as k_preproc_hbd<1, SUBY> does on the de-interleaved, shifted planes; the padding is written as zero.  Scalar
//                                   form: two padded columns x (1 + SUBY) rows per lane, element-aligned planes, any size.  Vector form: eight columns per lane, one
//                                   16-byte luma load per row and ONE 16-byte load for the four Cb, Cr pairs (the planar x8 form: two 8-byte loads); the host picks
//                                   it where w % 8 == 0 and both pointers and pitches are 16-byte aligned (sp_vec_ok).
//   k_apply_sp<R, ROWS2, PY, PC>    the fused luma + chroma blend of k_apply_yuv (apply_yuv.h) on interleaved chroma.  A lane owns R chroma pixels of one chroma row and
//                                   the 2 R x 2 (4:2:2: 2 R x 1) luma pixels under them, reads their motion once - apply_flow, scaled_mask_span - blends luma on the
//                                   motion as loaded and chroma on scaled_fetch_down's box mean (the same sums in the same order).  A chroma tap row is ONE load of
//                                   2 * 2 contiguous samples Cb, Cr, Cb, Cr (PackedTaps<2, PAIR> / packed_issue of hbd_packed.h) against one load per plane in
//                                   k_apply_yuv.  Samples are shifted right by sh before apply_finish, the code of apply_quant<uint16_t> left by sh before the store;
//                                   apply_taps, apply_finish, warp_lerp, the * m + ... * (1 - m) sum and apply_quant are the planar kernel's, in its order: the bytes
//                                   are those of k_apply_yuv on split(img), joined back.  R = 2 is the vector form (one 8-byte luma store per luma row and one 8-byte
//                                   CbCr store; both output planes' pointers and pitches aligned to 8, w >= 4), R = 1 the scalar form (u16 luma stores, one Cb, Cr
//                                   pair per store) for everything else, 1 x 1 upward: PY / PC = false are the single-column taps of a luma plane of one column
//                                   (w == 1) and a chroma plane of one column (w <= 2).  The ragged end of a row stores sample by sample / pair by pair; for odd h
//                                   the last luma row of a 4:2:0 pair does not exist.
//   k_copy_sp                       timestep 0 / 1: (v >> sh) << sh of n samples per row of one pitched plane
// No LDS, no scratch, no atomics; register arrays are indexed by compile-time constants only.  Pitches in bytes; offsets are 32-bit (rows * pitch < 2^32,
// semiplanar_check.h).  Nothing outside the rows' own samples of the output planes is written.
#pragma once
#include "hbd.h"
#include "apply_motion.h"
#include "apply_scaled.h"
#include "hbd_packed.h"

namespace rife {

struct SpPlanes { const uint8_t* y; const uint8_t* c; unsigned pitch_y, pitch_c; };

// ---- pre-processing ----
// scalar: two columns x (1 + SUBY) rows of the PADDED frame per lane; grid ((wp / 2 + 255) / 256, hp / (1 + SUBY))
template <int SUBY>
__global__ void k_preproc_sp(SpPlanes s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k, HbdShift r, int sh) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2, y = blockIdx.y * (1 + SUBY);
    if (x >= wp) return;
    uint2 o[1 + SUBY];
#pragma unroll
    for (int i = 0; i <= SUBY; i++) o[i] = make_uint2(0u, 0u);
    if (x < w && y < h) {
        const int cy = SUBY ? y / 2 : y;
        uint16_t c[2];                                                        // the pair Cb, Cr of chroma pixel x / 2: samples x, x + 1 of the row (x is even)
        __builtin_memcpy(c, __builtin_assume_aligned(s.c + ((unsigned)cy * s.pitch_c + (unsigned)x * 2u), 2), 4);
        const int cb = hbd_code((uint32_t)c[0] >> sh, r), cr = hbd_code((uint32_t)c[1] >> sh, r);
#pragma unroll
        for (int i = 0; i <= SUBY; i++) {
            if (y + i >= h) break;
            const uint16_t* p = reinterpret_cast<const uint16_t*>(s.y + ((unsigned)(y + i) * s.pitch_y + (unsigned)x * 2u));
            o[i].x = yuv_to_pk10(k, hbd_code((uint32_t)p[0] >> sh, r), cb, cr);
            if (x + 1 < w) o[i].y = yuv_to_pk10(k, hbd_code((uint32_t)p[1] >> sh, r), cb, cr);
        }
    }
#pragma unroll
    for (int i = 0; i <= SUBY; i++) *reinterpret_cast<uint2*>(out + (size_t)(y + i) * wp + x) = o[i];      // wp, hp are multiples of 32: x is even, row y + SUBY exists
}
// eight consecutive u16 samples from an address aligned to 16 bytes, as codes of the samples shifted right by sh
__device__ __forceinline__ void sp_load8(const uint8_t* p, HbdShift r, int sh, int* c) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; i++) { c[2 * i] = hbd_code((d[i] & 0xffffu) >> sh, r); c[2 * i + 1] = hbd_code(d[i] >> (16 + sh), r); }
}
// vector: eight columns x (1 + SUBY) rows of the PADDED frame per lane (w % 8 == 0, planes and pitches 16-byte aligned); grid ((wp / 8 + 255) / 256, hp / (1 + SUBY))
template <int SUBY>
__global__ void k_preproc_sp_vec(SpPlanes s, int w, int h, uint32_t* __restrict__ out, int wp, int hp, YuvCsp k, HbdShift r, int sh) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 8, y = blockIdx.y * (1 + SUBY);
    if (x >= wp) return;                                                      // wp is a multiple of 32: a lane's run is inside the row or past it
    uint32_t o[1 + SUBY][8];
#pragma unroll
    for (int i = 0; i <= SUBY; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) o[i][j] = 0u;
    if (x < w && y < h) {                                                     // w is a multiple of 8: the whole run is inside the frame
        int cc[8], yv[8];                                                     // cc: Cb, Cr of the four chroma pixels x / 2 .. x / 2 + 3
        const int cy = SUBY ? y / 2 : y;
        sp_load8(s.c + ((unsigned)cy * s.pitch_c + (unsigned)x * 2u), r, sh, cc);
#pragma unroll
        for (int i = 0; i <= SUBY; i++) {
            if (y + i >= h) break;
            sp_load8(s.y + ((unsigned)(y + i) * s.pitch_y + (unsigned)x * 2u), r, sh, yv);
#pragma unroll
            for (int j = 0; j < 8; j++) o[i][j] = yuv_to_pk10(k, yv[j], cc[(j / 2) * 2], cc[(j / 2) * 2 + 1]);
        }
    }
#pragma unroll
    for (int i = 0; i <= SUBY; i++) {
        uint4* d = reinterpret_cast<uint4*>(out + (size_t)(y + i) * wp + x);
        d[0] = make_uint4(o[i][0], o[i][1], o[i][2], o[i][3]);
        d[1] = make_uint4(o[i][4], o[i][5], o[i][6], o[i][7]);
    }
}

// ---- the blend ----
struct ApplySpArgs {
    ApplyScaledArgs c;            // the interleaved chroma plane in plane 0 of c.a: w, h = the chroma size in PAIRS x rows, extent = that size; the motion, mw x mh, mask_wide
    ApplyArgs y;                  // the luma plane in plane 0: w x h = mw x mh, the same motion
    int sh;                       // 16 - depth
};
// apply_scaled_blend (apply_scaled.h) on the luma plane with the samples shifted: the run x .. x + R - 1 of luma row y on the motion f, m
template <int R, bool PAIR, bool VEC>
__device__ __forceinline__ void sp_luma_blend(const ApplyArgs& a, int sh, int x, int y, const float4 (&f)[R], const float (&m)[R]) {
    const int nv = min(R, a.w - x);
    ApplyTaps t0[R], t1[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        const int xi = min(x + i, a.w - 1);
        t0[i] = apply_taps(xi, y, f[i].x, f[i].y, a.w, a.h, a.wp, a.hp);
        t1[i] = apply_taps(xi, y, f[i].z, f[i].w, a.w, a.h, a.wp, a.hp);
    }
    ApplyQuad<uint16_t> q0[R], q1[R];
#pragma unroll
    for (int i = 0; i < R; i++) { q0[i] = apply_issue<uint16_t, PAIR>(a.p0[0], a.pitch0[0], t0[i]); q1[i] = apply_issue<uint16_t, PAIR>(a.p1[0], a.pitch1[0], t1[i]); }
    uint16_t o[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        q0[i].a >>= sh; q0[i].b >>= sh; q0[i].c >>= sh; q0[i].d >>= sh;
        q1[i].a >>= sh; q1[i].b >>= sh; q1[i].c >>= sh; q1[i].d >>= sh;
        const float v = apply_finish<uint16_t, PAIR>(q0[i], t0[i]) * m[i] + apply_finish<uint16_t, PAIR>(q1[i], t1[i]) * (1 - m[i]);
        o[i] = (uint16_t)(apply_quant<uint16_t>(v, a.maxval) << sh);
    }
    uint8_t* row = a.out[0] + ((unsigned)y * a.pitcho[0] + (unsigned)x * 2u);
    if (VEC && nv == R) {         // R = 4: x is a multiple of 4, pointer and pitch aligned to 8
        uint2 v;
        __builtin_memcpy(&v, o, 8);
        *reinterpret_cast<uint2*>(row) = v;
    } else {
#pragma unroll
        for (int i = 0; i < R; i++) if (i < nv) reinterpret_cast<uint16_t*>(row)[i] = o[i];
    }
}
template <bool PAIR, int K>
__device__ __forceinline__ float sp_finish(const PackedTaps<2, PAIR>& q, const ApplyTaps& t, int sh) {
    ApplyQuad<uint16_t> s;
    if constexpr (PAIR) { s.a = q.r0[K] >> sh; s.b = q.r0[2 + K] >> sh; s.c = q.r1[K] >> sh; s.d = q.r1[2 + K] >> sh; }
    else { s.a = q.r0[K] >> sh; s.b = s.a; s.c = q.r1[K] >> sh; s.d = s.c; }      // one column: x0 = x1 = 0
    return apply_finish<uint16_t, PAIR>(s, t);
}
template <bool PAIR, int K>
__device__ __forceinline__ uint16_t sp_blend(const PackedTaps<2, PAIR>& q0, const ApplyTaps& t0, const PackedTaps<2, PAIR>& q1, const ApplyTaps& t1, float m, int maxval, int sh) {
    const float v = sp_finish<PAIR, K>(q0, t0, sh) * m + sp_finish<PAIR, K>(q1, t1, sh) * (1 - m);
    return (uint16_t)(apply_quant<uint16_t>(v, maxval) << sh);
}
// the run of R chroma pixels x .. x + R - 1 of chroma row y on the resampled motion f, m; a.w, a.h in chroma pixels
template <int R, bool PAIR, bool VEC>
__device__ __forceinline__ void sp_chroma_blend(const ApplyArgs& a, int sh, int x, int y, const float4 (&f)[R], const float (&m)[R]) {
    const int nv = min(R, a.w - x);
    ApplyTaps t0[R], t1[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        const int xi = min(x + i, a.w - 1);
        t0[i] = apply_taps(xi, y, f[i].x, f[i].y, a.w, a.h, a.wp, a.hp);
        t1[i] = apply_taps(xi, y, f[i].z, f[i].w, a.w, a.h, a.wp, a.hp);
    }
    PackedTaps<2, PAIR> q0[R], q1[R];
#pragma unroll
    for (int i = 0; i < R; i++) { q0[i] = packed_issue<2, PAIR>(a.p0[0], a.pitch0[0], t0[i]); q1[i] = packed_issue<2, PAIR>(a.p1[0], a.pitch1[0], t1[i]); }
    uint16_t o[2 * R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        o[2 * i] = sp_blend<PAIR, 0>(q0[i], t0[i], q1[i], t1[i], m[i], a.maxval, sh);
        o[2 * i + 1] = sp_blend<PAIR, 1>(q0[i], t0[i], q1[i], t1[i], m[i], a.maxval, sh);
    }
    uint8_t* row = a.out[0] + ((unsigned)y * a.pitcho[0] + (unsigned)x * 4u);
    if (VEC && nv == R) {         // R = 2: x is even, pointer and pitch aligned to 8
        uint2 v;
        __builtin_memcpy(&v, o, 8);
        *reinterpret_cast<uint2*>(row) = v;
    } else {
#pragma unroll
        for (int i = 0; i < R; i++) if (i < nv) __builtin_memcpy(__builtin_assume_aligned(row + 4 * i, 2), o + 2 * i, 4);      // one pair, at element alignment
    }
}
// grid: apply_blocks_x(cw, R) * ch workgroups of 256 chroma runs of one chroma row, remapped to bands of rows per XCD
template <int R, bool ROWS2, bool PY, bool PC>
__global__ void __launch_bounds__(256) k_apply_sp(const ApplySpArgs s, int nbx) {
    const int L = apply_block_index();
    const int cy = L / nbx, bx = L - cy * nbx;
    const int cx = (bx * 256 + (int)threadIdx.x) * R;
    if (cx >= s.c.a.w || cy >= s.c.a.h) return;
    const ApplyArgs& a = s.c.a;                                               // the motion's pointers, pitches and format
    const int cb = 2 * cx;                                                    // < mw: cx < (mw + 1) / 2
    const int r0 = ROWS2 ? 2 * cy : cy, r1 = min(2 * cy + 1, s.c.mh - 1);
    float4 F0[2 * R], F1[ROWS2 ? 2 * R : 1];
    float M0[2 * R], M1[2 * R];
#pragma unroll
    for (int k = 0; k < 2 * R; k++) {
        const int c = min(cb + k, s.c.mw - 1);
        F0[k] = apply_flow(a, c, r0);
        if constexpr (ROWS2) F1[k] = apply_flow(a, c, r1);
    }
    scaled_mask_span<R>(s.c, r0, cb, M0);
    if constexpr (ROWS2) scaled_mask_span<R>(s.c, r1, cb, M1);
    // the chroma motion: scaled_fetch_down's sums in its order
    float4 f[R];
    float m[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        if constexpr (ROWS2) {
            const float4 q = scaled_mul(scaled_add(scaled_add(F0[2 * i], F0[2 * i + 1]), scaled_add(F1[2 * i], F1[2 * i + 1])), 0.25f);
            f[i] = scaled_mul(q, 0.5f);
            m[i] = ((M0[2 * i] + M0[2 * i + 1]) + (M1[2 * i] + M1[2 * i + 1])) * 0.25f;
        } else {
            const float4 q = scaled_mul(scaled_add(F0[2 * i], F0[2 * i + 1]), 0.5f);
            f[i] = make_float4(q.x * 0.5f, q.y, q.z * 0.5f, q.w);
            m[i] = (M0[2 * i] + M0[2 * i + 1]) * 0.5f;
        }
    }
    // luma, one row at a time, on the motion as loaded
    sp_luma_blend<2 * R, PY, R == 2>(s.y, s.sh, cb, r0, F0, M0);
    if constexpr (ROWS2) {
        if (2 * cy + 1 < s.y.h) sp_luma_blend<2 * R, PY, R == 2>(s.y, s.sh, cb, 2 * cy + 1, F1, M1);      // r1 == 2 cy + 1 here
    }
    sp_chroma_blend<R, PC, R == 2>(a, s.sh, cx, cy, f, m);
}

// ---- timestep 0 / 1: (v >> sh) << sh of n samples per row; grid apply_blocks_x(n, 1) * rows workgroups of 256 lanes ----
__global__ void k_copy_sp(const uint8_t* __restrict__ in, unsigned pitch_in, uint8_t* __restrict__ out, unsigned pitch_out, int n, int rows, int sh, int nbx) {
    const int y = blockIdx.x / nbx, x = (blockIdx.x - y * nbx) * 256 + (int)threadIdx.x;
    if (x >= n || y >= rows) return;
    const uint32_t v = *reinterpret_cast<const uint16_t*>(in + ((unsigned)y * pitch_in + (unsigned)x * 2u));
    *reinterpret_cast<uint16_t*>(out + ((unsigned)y * pitch_out + (unsigned)x * 2u)) = (uint16_t)((v >> sh) << sh);
}

// ---- host side ----
static inline bool sp_vec_ok(const SpPlanes& s, int w) {
    return (w & 7) == 0 && ((reinterpret_cast<uintptr_t>(s.y) | reinterpret_cast<uintptr_t>(s.c) | s.pitch_y | s.pitch_c) & 15u) == 0;
}
// pixfmt: RIFE_HIP_PIX_I420P10 or _I422P10 with the colour bits; returns whether the vector form ran; force_scalar: the single-kernel test runs both forms on one image
static inline bool launch_preproc_sp(hipStream_t st, const SpPlanes& s, int w, int h, uint32_t* out, int wp, int hp, int pixfmt, int depth, bool force_scalar = false) {
    const HbdShift r = hbd_shift(depth);
    const int sh = 16 - depth;
    const bool vec = !force_scalar && sp_vec_ok(s, w);
    const YuvCsp k = yuv_csp(pixfmt & ~0xff, 10);
    const int suby = (pixfmt & 0xff) == RIFE_HIP_PIX_I420P10 ? 1 : 0;
    const dim3 g = vec ? dim3((wp / 8 + 255) / 256, hp / (1 + suby)) : dim3((wp / 2 + 255) / 256, hp / (1 + suby));
    if (suby) {
        if (vec) hipLaunchKernelGGL(k_preproc_sp_vec<1>, g, dim3(256), 0, st, s, w, h, out, wp, hp, k, r, sh);
        else hipLaunchKernelGGL(k_preproc_sp<1>, g, dim3(256), 0, st, s, w, h, out, wp, hp, k, r, sh);
    } else {
        if (vec) hipLaunchKernelGGL(k_preproc_sp_vec<0>, g, dim3(256), 0, st, s, w, h, out, wp, hp, k, r, sh);
        else hipLaunchKernelGGL(k_preproc_sp<0>, g, dim3(256), 0, st, s, w, h, out, wp, hp, k, r, sh);
    }
    return vec;
}
// the vector form stores 8 bytes per luma run and per chroma run: both output pointers and pitches are aligned to 8, and the luma plane has at least 4 columns
static inline bool apply_sp_vector_ok(const ApplySpArgs& s) {
    return s.y.w >= 4 && ((reinterpret_cast<uintptr_t>(s.y.out[0]) | reinterpret_cast<uintptr_t>(s.c.a.out[0]) | s.y.pitcho[0] | s.c.a.pitcho[0]) & 7u) == 0;
}
template <int R, bool PY, bool PC>
static inline void launch_apply_sp_r(hipStream_t st, const ApplySpArgs& s) {
    const int nbx = apply_blocks_x(s.c.a.w, R);
    const dim3 g((unsigned)nbx * (unsigned)s.c.a.h);
    if (s.c.rows2) hipLaunchKernelGGL((k_apply_sp<R, true, PY, PC>), g, dim3(256), 0, st, s, nbx);
    else hipLaunchKernelGGL((k_apply_sp<R, false, PY, PC>), g, dim3(256), 0, st, s, nbx);
}
// s.c.a / s.y on the SAME motion of s.c.mw x s.c.mh = the luma size; rows2 = 4:2:0; returns whether the vector form ran
static inline bool launch_apply_sp(hipStream_t st, ApplySpArgs s, bool rows2, bool force_scalar = false) {
    s.c.rows2 = rows2;
    s.c.mask_wide = reinterpret_cast<uintptr_t>(s.c.a.mask) % 16 == 0 && s.c.a.mask_pitch % 16 == 0;
    const bool vec = !force_scalar && apply_sp_vector_ok(s);
    if (vec) launch_apply_sp_r<2, true, true>(st, s);
    else if (s.y.w >= 3) launch_apply_sp_r<1, true, true>(st, s);
    else if (s.y.w == 2) launch_apply_sp_r<1, true, false>(st, s);            // a chroma plane of one column
    else launch_apply_sp_r<1, false, false>(st, s);                           // and a luma plane of one column
    return vec;
}
static inline void launch_copy_sp(hipStream_t st, const uint8_t* in, size_t pitch_in, uint8_t* out, size_t pitch_out, int n, int rows, int depth) {
    const int nbx = apply_blocks_x(n, 1);
    hipLaunchKernelGGL(k_copy_sp, dim3((unsigned)nbx * (unsigned)rows), dim3(256), 0, st, in, (unsigned)pitch_in, out, (unsigned)pitch_out, n, rows, 16 - depth, nbx);
}

}  // namespace rife
