// apply_motion.h: a motion field applied to the caller's own planes (include/rife_hip.h "apply motion") - the tail of rife-v4.6,
//     v = Warp(p0[k], dx0, dy0) * m + Warp(p1[k], dx1, dy1) * (1 - m)
// on n <= 4 planes of u8 / u16 / half / float samples at full fp32 precision, with rife.Warp's clamp-then-alpha rule (elementwise.h warp_taps) over an EXTENT wp x hp
// that the planes are zero-padded to: extent = the padded frame is the engine's colour path, extent = w x h is edge clamping, the engine's alpha path.
// Memory-bound: per pixel 20 B of motion (F32) in and n samples out; the eight taps per plane come mostly from cache.  A lane owns a run of R adjacent pixels of one
// row, so a full run is ONE store of R samples per plane (u8: 4 B, u16 / half: 4 B, float: 8 B); R = 1 is the scalar form, for planes whose pointer or pitch is not
// store-aligned (and the force_scalar hook of rife_hip_op_apply); the ragged end of a row stores its samples one by one.  All tap loads of a run of one plane - one two-sample load per
// tap row - are issued before its first blend.  Products and sums are rounded separately (the build has no contraction).  No LDS, no atomics; the block index is remapped
// to contiguous bands of rows per XCD, as in the other tile kernels.
// Pitches in bytes; offsets are 32-bit (h * pitch < 2^32, apply_check.h).  Nothing outside the w x h samples of the output planes is written.
#pragma once
#include <type_traits>

namespace rife {

struct ApplyArgs {
    const uint8_t* p0[4]; const uint8_t* p1[4]; uint8_t* out[4];
    unsigned pitch0[4], pitch1[4], pitcho[4];
    const uint8_t* flow; const uint8_t* mask;      // both required
    unsigned flow_pitch, mask_pitch;
    int format;                                    // RIFE_HIP_MOTION_F32 / _F16 (wave-uniform)
    int w, h, wp, hp, n, maxval;
};

// the run of the vector form: every store is at least 4 bytes
template <typename T> struct ApplyRun { static constexpr int R = sizeof(T) == 1 ? 4 : 2; };

// one warp of one pixel: the tap columns and rows inside the plane, whether each lies in the w x h samples (else it reads the virtual zero padding), and the weights
// from the tap clamped to the extent.  The two taps of a row are neighbours - or the same sample where the position leaves the extent or meets the plane's last column -
// so, as warp_issue does (elementwise.h), a row is ONE load of two samples at column xb = min(x0, w - 2) and a select: half the gather instructions, the same values.
// PAIR = false (planes of one column): four single loads.
struct ApplyTaps { int x0, x1, xb, y0, y1; bool vx0, vx1, vy0, vy1, l0, l1; float alpha, beta; };
__device__ __forceinline__ ApplyTaps apply_taps(int x, int y, float dx, float dy, int w, int h, int wp, int hp) {
    const float sx = (float)x + dx, sy = (float)y + dy;
    int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = min(max(x0, 0), wp - 1); x1 = min(max(x1, 0), wp - 1);
    y0 = min(max(y0, 0), hp - 1); y1 = min(max(y1, 0), hp - 1);
    ApplyTaps t;
    t.alpha = sx - (float)x0; t.beta = sy - (float)y0;      // clamp, THEN alpha
    t.vx0 = x0 < w; t.vx1 = x1 < w; t.vy0 = y0 < h; t.vy1 = y1 < h;
    t.x0 = min(x0, w - 1); t.x1 = min(x1, w - 1); t.y0 = min(y0, h - 1); t.y1 = min(y1, h - 1);      // the address stays inside the plane; the value is dropped
    t.xb = max(min(t.x0, w - 2), 0);                        // x1 is x0 or x0 + 1: both lie in xb, xb + 1
    t.l0 = t.x0 == t.xb; t.l1 = t.x1 == t.xb;
    return t;
}
template <typename T>
__device__ __forceinline__ T apply_ld(const uint8_t* __restrict__ p, unsigned pitch, int xi, int yi) {
    return *reinterpret_cast<const T*>(p + ((unsigned)yi * pitch + (unsigned)xi * (unsigned)sizeof(T)));
}
template <typename T> struct ApplyQuad { T a, b, c, d; };      // (x0, y0), (x1, y0), (x0, y1), (x1, y1)
template <typename T, bool PAIR>
__device__ __forceinline__ ApplyQuad<T> apply_issue(const uint8_t* __restrict__ p, unsigned pitch, const ApplyTaps& t) {
    ApplyQuad<T> q;
    if constexpr (PAIR) {      // the pair sits at an element-aligned address, not at twice that
        __builtin_memcpy(&q.a, __builtin_assume_aligned(p + ((unsigned)t.y0 * pitch + (unsigned)t.xb * (unsigned)sizeof(T)), sizeof(T)), 2 * sizeof(T));
        __builtin_memcpy(&q.c, __builtin_assume_aligned(p + ((unsigned)t.y1 * pitch + (unsigned)t.xb * (unsigned)sizeof(T)), sizeof(T)), 2 * sizeof(T));
    } else {
        q.a = apply_ld<T>(p, pitch, t.x0, t.y0); q.b = apply_ld<T>(p, pitch, t.x1, t.y0);
        q.c = apply_ld<T>(p, pitch, t.x0, t.y1); q.d = apply_ld<T>(p, pitch, t.x1, t.y1);
    }
    return q;
}
template <typename T, bool PAIR>
__device__ __forceinline__ float apply_finish(const ApplyQuad<T>& q, const ApplyTaps& t) {
    T s00 = q.a, s10 = q.b, s01 = q.c, s11 = q.d;
    if constexpr (PAIR) { s00 = t.l0 ? q.a : q.b; s10 = t.l1 ? q.a : q.b; s01 = t.l0 ? q.c : q.d; s11 = t.l1 ? q.c : q.d; }
    const float a = (t.vx0 && t.vy0) ? (float)s00 : 0.f, b = (t.vx1 && t.vy0) ? (float)s10 : 0.f;
    const float c = (t.vx0 && t.vy1) ? (float)s01 : 0.f, d = (t.vx1 && t.vy1) ? (float)s11 : 0.f;
    return warp_lerp(a, b, c, d, t.alpha, t.beta);
}
template <typename T> __device__ __forceinline__ T apply_quant(float v, int maxval);
template <> __device__ __forceinline__ uint8_t apply_quant<uint8_t>(float v, int maxval) { return (uint8_t)min(max((int)(v + 0.5f), 0), maxval); }
template <> __device__ __forceinline__ uint16_t apply_quant<uint16_t>(float v, int maxval) { return (uint16_t)min(max((int)(v + 0.5f), 0), maxval); }
template <> __device__ __forceinline__ _Float16 apply_quant<_Float16>(float v, int) { return (_Float16)v; }      // round to nearest even
template <> __device__ __forceinline__ float apply_quant<float>(float v, int) { return v; }

__device__ __forceinline__ float4 apply_flow(const ApplyArgs& a, int x, int y) {
    if (a.format == RIFE_HIP_MOTION_F16) {
        const uint2 q = *reinterpret_cast<const uint2*>(a.flow + ((unsigned)y * a.flow_pitch + (unsigned)x * 8u));
        _Float16 hv[4];
        __builtin_memcpy(hv, &q, 8);
        return make_float4((float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]);
    }
    return *reinterpret_cast<const float4*>(a.flow + ((unsigned)y * a.flow_pitch + (unsigned)x * 16u));
}
__device__ __forceinline__ float apply_mask(const ApplyArgs& a, int x, int y) {
    if (a.format == RIFE_HIP_MOTION_F16) return (float)*reinterpret_cast<const _Float16*>(a.mask + ((unsigned)y * a.mask_pitch + (unsigned)x * 2u));
    return *reinterpret_cast<const float*>(a.mask + ((unsigned)y * a.mask_pitch + (unsigned)x * 4u));
}

// the run of R pixels x .. x + R - 1 of row y (x < w, y < h)
template <typename T, int R, bool PAIR>
__device__ __forceinline__ void apply_run(const ApplyArgs& a, int x, int y) {
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
    for (int k = 0; k < a.n; k++) {
        ApplyQuad<T> q0[R], q1[R];
#pragma unroll
        for (int i = 0; i < R; i++) { q0[i] = apply_issue<T, PAIR>(a.p0[k], a.pitch0[k], t0[i]); q1[i] = apply_issue<T, PAIR>(a.p1[k], a.pitch1[k], t1[i]); }
        T o[R];
#pragma unroll
        for (int i = 0; i < R; i++) {
            const float v = apply_finish<T, PAIR>(q0[i], t0[i]) * m[i] + apply_finish<T, PAIR>(q1[i], t1[i]) * (1 - m[i]);
            o[i] = apply_quant<T>(v, a.maxval);
        }
        uint8_t* row = a.out[k] + ((unsigned)y * a.pitcho[k] + (unsigned)x * (unsigned)sizeof(T));
        if (nv == R) {
            if constexpr (R * sizeof(T) == 8) { uint2 v; __builtin_memcpy(&v, o, 8); *reinterpret_cast<uint2*>(row) = v; }
            else if constexpr (R * sizeof(T) == 4) { uint32_t v; __builtin_memcpy(&v, o, 4); *reinterpret_cast<uint32_t*>(row) = v; }
            else reinterpret_cast<T*>(row)[0] = o[0];
        } else {
#pragma unroll
            for (int i = 0; i < R; i++) if (i < nv) reinterpret_cast<T*>(row)[i] = o[i];
        }
    }
}
// 1-D grid of apply_blocks_x * h workgroups of 256 lanes: workgroup -> 256 runs of one row.  Workgroup b runs on XCD b % 8, and every XCD has an L2 of its own: the
// index is remapped as in the other per-pixel tile kernels (conv_row.h), so that an XCD walks a contiguous band of rows and the tap rows a row shares with its
// neighbours come from that XCD's L2.
static inline int apply_blocks_x(int w, int R) { return ((w + R - 1) / R + 255) / 256; }
__device__ __forceinline__ int apply_block_index() {
    const int n = gridDim.x, b = blockIdx.x;
    const int q = n >> 3, r = n & 7, xcd = b & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}
template <typename T, int R, bool PAIR>
__global__ void __launch_bounds__(256) k_apply_motion(const ApplyArgs a, int nbx) {
    const int L = apply_block_index();
    const int y = L / nbx, bx = L - y * nbx;
    const int x = (bx * 256 + (int)threadIdx.x) * R;
    if (x >= a.w || y >= a.h) return;
    apply_run<T, R, PAIR>(a, x, y);
}

// timestep 0 / 1 of the combined calls: a copy of one plane set, integer samples clamped to maxval; one sample per lane
template <typename T>
__global__ void k_apply_copy(const ApplyArgs a, int nbx) {
    const int y = blockIdx.x / nbx, x = (blockIdx.x - y * nbx) * 256 + (int)threadIdx.x;
    if (x >= a.w || y >= a.h) return;
    for (int k = 0; k < a.n; k++) {
        T v = apply_ld<T>(a.p0[k], a.pitch0[k], x, y);
        if constexpr (std::is_integral<T>::value) v = (T)min((int)v, a.maxval);
        *reinterpret_cast<T*>(a.out[k] + ((unsigned)y * a.pitcho[k] + (unsigned)x * (unsigned)sizeof(T))) = v;
    }
}

// ---- host side ----
// the vector form stores R samples at once: every output pointer and pitch is aligned to that store
template <typename T>
static inline bool apply_vector_ok(const ApplyArgs& a) {
    const unsigned unit = ApplyRun<T>::R * (unsigned)sizeof(T);
    for (int k = 0; k < a.n; k++) if (reinterpret_cast<uintptr_t>(a.out[k]) % unit || a.pitcho[k] % unit) return false;
    return true;
}
template <typename T, int R>
static inline void launch_apply_r(hipStream_t st, const ApplyArgs& a) {
    const int nbx = apply_blocks_x(a.w, R);
    const dim3 g((unsigned)nbx * (unsigned)a.h);
    if (a.w >= 2) hipLaunchKernelGGL((k_apply_motion<T, R, true>), g, dim3(256), 0, st, a, nbx);
    else hipLaunchKernelGGL((k_apply_motion<T, R, false>), g, dim3(256), 0, st, a, nbx);
}
template <typename T>
static inline void launch_apply_t(hipStream_t st, const ApplyArgs& a, bool force_scalar) {
    if (!force_scalar && apply_vector_ok<T>(a)) launch_apply_r<T, ApplyRun<T>::R>(st, a);
    else launch_apply_r<T, 1>(st, a);
}
// force_scalar: the single-kernel tests run both forms on one input
static inline void launch_apply(hipStream_t st, const ApplyArgs& a, int sample, bool force_scalar = false) {
    if (sample == RIFE_HIP_SAMPLE_U8) launch_apply_t<uint8_t>(st, a, force_scalar);
    else if (sample == RIFE_HIP_SAMPLE_U16) launch_apply_t<uint16_t>(st, a, force_scalar);
    else if (sample == RIFE_HIP_SAMPLE_F16) launch_apply_t<_Float16>(st, a, force_scalar);
    else launch_apply_t<float>(st, a, force_scalar);
}
static inline void launch_apply_copy(hipStream_t st, const ApplyArgs& a, int sample) {
    const int nbx = apply_blocks_x(a.w, 1);
    const dim3 g((unsigned)nbx * (unsigned)a.h);
    if (sample == RIFE_HIP_SAMPLE_U8) hipLaunchKernelGGL(k_apply_copy<uint8_t>, g, dim3(256), 0, st, a, nbx);
    else if (sample == RIFE_HIP_SAMPLE_U16) hipLaunchKernelGGL(k_apply_copy<uint16_t>, g, dim3(256), 0, st, a, nbx);
    else if (sample == RIFE_HIP_SAMPLE_F16) hipLaunchKernelGGL(k_apply_copy<_Float16>, g, dim3(256), 0, st, a, nbx);
    else hipLaunchKernelGGL(k_apply_copy<float>, g, dim3(256), 0, st, a, nbx);
}

}  // namespace rife
