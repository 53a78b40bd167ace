// hbd_packed.h: packed (interleaved) 16-bit RGB / RGBA frames at the frame boundary (include/rife_hip.h "16-bit packed RGB and RGBA": rife_hip_packed_t).
//   k_preproc_packed<CH> / _vec     the caller's pitched rows of CH interleaved u16 samples at 10..16 bits -> the resident 10:10:10 dwords the network estimates motion
//                                   on: hbd_code (hbd.h) per colour sample, packed as k_preproc_hbd_rgb packs them; alpha never reaches the network.  Scalar form: one
//                                   padded pixel per lane, element-aligned rows, any size.  Vector form: CH = 4 four pixels per lane from two 16-byte loads and one
//                                   16-byte store; CH = 3 eight pixels per lane from three 16-byte loads and two 16-byte stores; the host picks it where the data
//                                   pointer and pitch are 16-byte aligned and w % 4 == 0 (CH 4) / w % 8 == 0 (CH 3) (packed_vec_ok).
//   k_apply_packed<CH, R, PAIR>     the blend of apply_motion.h on packed samples, edge semantics (extent = w x h).  A lane owns R adjacent pixels of a row, reads
//                                   their flow and mask once, computes apply_taps once per pixel and frame, and loads each tap row ONCE: the two neighbouring pixels
//                                   at xb are 2 * CH contiguous samples (12 or 16 bytes at element alignment), against one two-sample load per plane in the planar
//                                   kernel.  All loads of a run are issued before its first blend.  Per channel the selects and validity of apply_finish, warp_lerp,
//                                   the * m + ... * (1 - m) sum and apply_quant<uint16_t> are the planar kernel's, in its order: the bytes are those of
//                                   k_apply_motion<uint16_t> on the de-interleaved planes.  R = 2 is the vector form (stores of 8 bytes per pixel for CH = 4, 12 bytes
//                                   per run for CH = 3), R = 1 the scalar form with u16 stores; PAIR = false serves w == 1; the ragged end of a row stores sample by
//                                   sample.
// No LDS, no scratch, no atomics; register arrays are indexed by compile-time constants only.  Pitches in bytes; offsets are 32-bit (h * pitch < 2^32, packed_check.h).
// Nothing outside the w x h pixels of the output is written.
#pragma once
#include "hbd.h"
#include "apply_motion.h"

namespace rife {

// ---- pre-processing ----
__device__ __forceinline__ uint32_t packed_pk10(uint32_t r, uint32_t g, uint32_t b, HbdShift s) {
    return (uint32_t)hbd_code(r, s) | ((uint32_t)hbd_code(g, s) << 10) | ((uint32_t)hbd_code(b, s) << 20);
}
// scalar: one pixel of the PADDED frame per lane; grid ((wp + 255) / 256, hp)
template <int CH>
__global__ void k_preproc_packed(const uint8_t* __restrict__ in, unsigned pitch, int w, int h, uint32_t* __restrict__ out, int wp, int hp, HbdShift r) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= wp) return;
    uint32_t v = 0u;
    if (x < w && y < h) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(in + ((unsigned)y * pitch + (unsigned)x * (unsigned)(CH * 2)));
        v = packed_pk10(p[0], p[1], p[2], r);
    }
    out[(size_t)y * wp + x] = v;                                              // blockIdx.y < hp: the grid has hp rows
}
// vector: NP = 4 (CH 4) / 8 (CH 3) pixels of one row of the PADDED frame per lane (w % NP == 0, data and pitch 16-byte aligned); grid ((wp / NP + 255) / 256, hp)
template <int CH>
__global__ void k_preproc_packed_vec(const uint8_t* __restrict__ in, unsigned pitch, int w, int h, uint32_t* __restrict__ out, int wp, int hp, HbdShift r) {
    constexpr int NP = CH == 4 ? 4 : 8, NQ = NP * CH / 8;                     // pixels per lane; 16-byte loads per lane (2 / 3)
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * NP, y = blockIdx.y;
    if (x >= wp) return;                                                      // wp is a multiple of 32: a lane's run is inside the row or past it
    uint32_t o[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) o[j] = 0u;
    if (x < w && y < h) {                                                     // w is a multiple of NP: the whole run is inside the frame
        const uint4* src = reinterpret_cast<const uint4*>(in + ((unsigned)y * pitch + (unsigned)x * (unsigned)(CH * 2)));
        uint32_t d[NQ * 4];
#pragma unroll
        for (int i = 0; i < NQ; i++) { const uint4 q = src[i]; d[4 * i] = q.x; d[4 * i + 1] = q.y; d[4 * i + 2] = q.z; d[4 * i + 3] = q.w; }
#pragma unroll
        for (int j = 0; j < NP; j++) {
            const int s = j * CH;                                             // sample index of the pixel's R: a compile-time constant after unrolling
            const uint32_t cr = (d[s >> 1] >> ((s & 1) * 16)) & 0xffffu;
            const uint32_t cg = (d[(s + 1) >> 1] >> (((s + 1) & 1) * 16)) & 0xffffu;
            const uint32_t cb = (d[(s + 2) >> 1] >> (((s + 2) & 1) * 16)) & 0xffffu;
            o[j] = packed_pk10(cr, cg, cb, r);
        }
    }
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)y * wp + x);
#pragma unroll
    for (int i = 0; i < NP / 4; i++) dst[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}

// ---- the blend ----
// the two tap rows of one pixel of one frame: 2 * CH samples each (PAIR), or CH (a frame of one column)
template <int CH, bool PAIR> struct PackedTaps { uint16_t r0[(PAIR ? 2 : 1) * CH], r1[(PAIR ? 2 : 1) * CH]; };
template <int CH, bool PAIR>
__device__ __forceinline__ PackedTaps<CH, PAIR> packed_issue(const uint8_t* __restrict__ p, unsigned pitch, const ApplyTaps& t) {
    PackedTaps<CH, PAIR> q;
    constexpr unsigned PX = CH * 2u, NB = (PAIR ? 2u : 1u) * PX;              // bytes of a pixel; bytes of a tap row
    const unsigned xo = (unsigned)(PAIR ? t.xb : t.x0) * PX;                  // the row sits at an element-aligned address
    __builtin_memcpy(q.r0, __builtin_assume_aligned(p + ((unsigned)t.y0 * pitch + xo), 2), NB);
    __builtin_memcpy(q.r1, __builtin_assume_aligned(p + ((unsigned)t.y1 * pitch + xo), 2), NB);
    return q;
}
template <int CH, bool PAIR, int K>
__device__ __forceinline__ float packed_finish(const PackedTaps<CH, PAIR>& q, const ApplyTaps& t) {
    ApplyQuad<uint16_t> s;
    if constexpr (PAIR) { s.a = q.r0[K]; s.b = q.r0[CH + K]; s.c = q.r1[K]; s.d = q.r1[CH + K]; }
    else { s.a = q.r0[K]; s.b = q.r0[K]; s.c = q.r1[K]; s.d = q.r1[K]; }      // one column: x0 = x1 = 0
    return apply_finish<uint16_t, PAIR>(s, t);
}
template <int CH, bool PAIR, int K>
__device__ __forceinline__ uint16_t packed_blend(const PackedTaps<CH, PAIR>& q0, const ApplyTaps& t0, const PackedTaps<CH, PAIR>& q1, const ApplyTaps& t1, float m, int maxval) {
    const float v = packed_finish<CH, PAIR, K>(q0, t0) * m + packed_finish<CH, PAIR, K>(q1, t1) * (1 - m);
    return apply_quant<uint16_t>(v, maxval);
}
// the run of R pixels x .. x + R - 1 of row y (x < w, y < h); a: plane 0 of ApplyArgs holds the packed frames, w, h in pixels, wp, hp = w, h
template <int CH, int R, bool PAIR>
__device__ __forceinline__ void apply_packed_run(const ApplyArgs& a, int x, int y) {
    const int nv = min(R, a.w - x);                                           // < R: the ragged end of the row
    ApplyTaps t0[R], t1[R];
    float m[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        const int xi = min(x + i, a.w - 1);                                   // a lane past the end repeats the last pixel; its result is not stored
        const float4 f = apply_flow(a, xi, y);
        m[i] = apply_mask(a, xi, y);
        t0[i] = apply_taps(xi, y, f.x, f.y, a.w, a.h, a.wp, a.hp);
        t1[i] = apply_taps(xi, y, f.z, f.w, a.w, a.h, a.wp, a.hp);
    }
    PackedTaps<CH, PAIR> q0[R], q1[R];
#pragma unroll
    for (int i = 0; i < R; i++) { q0[i] = packed_issue<CH, PAIR>(a.p0[0], a.pitch0[0], t0[i]); q1[i] = packed_issue<CH, PAIR>(a.p1[0], a.pitch1[0], t1[i]); }
    uint16_t o[R * CH];
#pragma unroll
    for (int i = 0; i < R; i++) {
        o[i * CH + 0] = packed_blend<CH, PAIR, 0>(q0[i], t0[i], q1[i], t1[i], m[i], a.maxval);
        o[i * CH + 1] = packed_blend<CH, PAIR, 1>(q0[i], t0[i], q1[i], t1[i], m[i], a.maxval);
        o[i * CH + 2] = packed_blend<CH, PAIR, 2>(q0[i], t0[i], q1[i], t1[i], m[i], a.maxval);
        if constexpr (CH == 4) o[i * CH + 3] = packed_blend<CH, PAIR, 3>(q0[i], t0[i], q1[i], t1[i], m[i], a.maxval);
    }
    uint8_t* row = a.out[0] + ((unsigned)y * a.pitcho[0] + (unsigned)x * (unsigned)(CH * 2));
    if (R == 2 && nv == R) {
        if constexpr (CH == 4) {      // x is even: 16 x bytes from a pointer and pitch aligned to 8
            uint2 v[2];
            __builtin_memcpy(v, o, 16);
            reinterpret_cast<uint2*>(row)[0] = v[0]; reinterpret_cast<uint2*>(row)[1] = v[1];
        } else {                      // 12 x bytes from a pointer and pitch aligned to 4
            uint32_t v[3];
            __builtin_memcpy(v, o, 12);
            reinterpret_cast<uint32_t*>(row)[0] = v[0]; reinterpret_cast<uint32_t*>(row)[1] = v[1]; reinterpret_cast<uint32_t*>(row)[2] = v[2];
        }
    } else {
#pragma unroll
        for (int i = 0; i < R; i++)
            if (i < nv) {
#pragma unroll
                for (int k = 0; k < CH; k++) reinterpret_cast<uint16_t*>(row)[i * CH + k] = o[i * CH + k];
            }
    }
}
// the grid of k_apply_motion: apply_blocks_x(w, R) * h workgroups of 256 lanes, the index remapped to bands of rows per XCD (apply_block_index)
template <int CH, int R, bool PAIR>
__global__ void __launch_bounds__(256) k_apply_packed(const ApplyArgs a, int nbx) {
    const int L = apply_block_index();
    const int y = L / nbx, bx = L - y * nbx;
    const int x = (bx * 256 + (int)threadIdx.x) * R;
    if (x >= a.w || y >= a.h) return;
    apply_packed_run<CH, R, PAIR>(a, x, y);
}

// ---- host side ----
static inline bool packed_vec_ok(const uint8_t* in, size_t pitch, int w, int ch) {
    return ((reinterpret_cast<uintptr_t>(in) | pitch) & 15u) == 0 && (w % (ch == 4 ? 4 : 8)) == 0;
}
// returns whether the vector form ran; force_scalar: the single-kernel test runs both forms on one image
static inline bool launch_preproc_packed(hipStream_t st, const uint8_t* in, size_t pitch, int ch, int w, int h, uint32_t* out, int wp, int hp, int depth, bool force_scalar = false) {
    const HbdShift r = hbd_shift(depth);
    const bool vec = !force_scalar && packed_vec_ok(in, pitch, w, ch);
    const unsigned pb = (unsigned)pitch;
    if (ch == 4) {
        if (vec) hipLaunchKernelGGL(k_preproc_packed_vec<4>, dim3((wp / 4 + 255) / 256, hp), dim3(256), 0, st, in, pb, w, h, out, wp, hp, r);
        else hipLaunchKernelGGL(k_preproc_packed<4>, dim3((wp + 255) / 256, hp), dim3(256), 0, st, in, pb, w, h, out, wp, hp, r);
    } else {
        if (vec) hipLaunchKernelGGL(k_preproc_packed_vec<3>, dim3((wp / 8 + 255) / 256, hp), dim3(256), 0, st, in, pb, w, h, out, wp, hp, r);
        else hipLaunchKernelGGL(k_preproc_packed<3>, dim3((wp + 255) / 256, hp), dim3(256), 0, st, in, pb, w, h, out, wp, hp, r);
    }
    return vec;
}
// the vector form stores 8 bytes per pixel (CH 4) or 12 bytes per run of two pixels (CH 3): the output pointer and pitch are aligned to 8 / 4 bytes
static inline bool apply_packed_vector_ok(const ApplyArgs& a, int ch) {
    const unsigned unit = ch == 4 ? 8u : 4u;
    return reinterpret_cast<uintptr_t>(a.out[0]) % unit == 0 && a.pitcho[0] % unit == 0;
}
template <int CH, int R>
static inline void launch_apply_packed_r(hipStream_t st, const ApplyArgs& a) {
    const int nbx = apply_blocks_x(a.w, R);
    const dim3 g((unsigned)nbx * (unsigned)a.h);
    if (a.w >= 2) hipLaunchKernelGGL((k_apply_packed<CH, R, true>), g, dim3(256), 0, st, a, nbx);
    else hipLaunchKernelGGL((k_apply_packed<CH, R, false>), g, dim3(256), 0, st, a, nbx);
}
// returns whether the vector form ran
static inline bool launch_apply_packed(hipStream_t st, const ApplyArgs& a, int ch, bool force_scalar = false) {
    const bool vec = !force_scalar && apply_packed_vector_ok(a, ch);
    if (ch == 4) { if (vec) launch_apply_packed_r<4, 2>(st, a); else launch_apply_packed_r<4, 1>(st, a); }
    else { if (vec) launch_apply_packed_r<3, 2>(st, a); else launch_apply_packed_r<3, 1>(st, a); }
    return vec;
}

}  // namespace rife
