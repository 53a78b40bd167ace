// apply_scaled.h: a motion field applied to planes at HALF or TWICE its resolution (include/rife_hip.h "apply motion at another resolution": 4:2:0 / 4:2:2 chroma,
// proxy upscaling).  The result is apply_motion.h's definition, unchanged, in the planes' own coordinates on a RESAMPLED motion of the planes' size; only the
// per-pixel motion fetch is new, and everything after it - apply_taps, apply_issue, apply_finish, apply_quant, the run / store scheme, the XCD band remap - is
// apply_motion.h's code, in apply_run's order (the single-launch tests demand apply_run's bytes on the resampled motion).
// The resampled motion in fp32, every product and sum rounded separately (the build has no contraction); M = any of dx0, dy0, dx1, dy1, m; mw x mh = the motion:
//   MODE_DOWN, rows2 (4:2:0)   c0 = 2x, c1 = min(2x + 1, mw - 1), r0 = 2y, r1 = min(2y + 1, mh - 1):  s = ((M[r0][c0] + M[r0][c1]) + (M[r1][c0] + M[r1][c1])) * 0.25f,
//                              dx' = s.dx * 0.5f, dy' = s.dy * 0.5f, m' = s.m
//   MODE_DOWN, !rows2 (4:2:2)  s = (M[y][c0] + M[y][c1]) * 0.5f,  dx' = s.dx * 0.5f, dy' = s.dy, m' = s.m
//   MODE_UP (x2 bilinear, half-pixel centres, edge clamp)   j = x >> 1, jn = (x & 1) ? min(j + 1, mw - 1) : max(j - 1, 0), i / in from y and mh likewise:
//                              H(r) = M[r][j] * 0.75f + M[r][jn] * 0.25f,  s = H(i) * 0.75f + H(in) * 0.25f,  dx' = s.dx * 2.f, dy' = s.dy * 2.f, m' = s.m
// rows2 is a wave-uniform run-time value, not a template parameter.  A lane owns a run of R plane pixels (ApplyRun<T>::R, or 1):
//   down   2 R adjacent motion pixels of one row (two rows for 4:2:0), each flow pixel ONE 16-byte (F32) / 8-byte (F16) load, adjacent lanes reading adjacent
//          spans; the 2 R mask samples of a row as whole 16- / 8- / 4-byte loads where the mask pointer and pitch are 16-byte aligned (the rules ask only for
//          element alignment) and the span lies inside the row, else element by element with the clamped index.  All loads of a run are issued before its first add.
//   up     a run that starts at even x reads motion columns j - 1 .. j + R / 2 (clamped) of two rows, R / 2 + 2 flow loads per row for R pixels; neighbours in a
//          wave share them from cache.  R = 1: the two columns j, jn.
// Every motion index is clamped into mw x mh and every tap address into the plane (apply_taps); nothing but the ws x hs output samples is written.  32-bit byte
// offsets as in apply_motion.h.  No LDS, no atomics.
#pragma once

namespace rife {

enum { APPLY_MODE_DOWN = 0, APPLY_MODE_UP = 1 };

struct ApplyScaledArgs {
    ApplyArgs a;                  // w, h: the PLANE size ws x hs; flow, mask and their pitches: the motion of mw x mh
    int mw, mh;
    int rows2;                    // down: 1 = 4:2:0 (two motion rows per plane row), 0 = 4:2:2
    int mask_wide;                // down: mask pointer and pitch are 16-byte aligned
};

__device__ __forceinline__ float4 scaled_add(const float4& p, const float4& q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); }
__device__ __forceinline__ float4 scaled_mul(const float4& p, float s) { return make_float4(p.x * s, p.y * s, p.z * s, p.w * s); }

// 2 R mask samples of motion row r from column cb (cb = 2 x, x a multiple of R)
template <int R>
__device__ __forceinline__ void scaled_mask_span(const ApplyScaledArgs& s, int r, int cb, float (&m)[2 * R]) {
    const ApplyArgs& a = s.a;
    if (s.mask_wide && cb + 2 * R <= s.mw) {
        if (a.format == RIFE_HIP_MOTION_F16) {
            _Float16 hv[2 * R];
            __builtin_memcpy(hv, __builtin_assume_aligned(a.mask + ((unsigned)r * a.mask_pitch + (unsigned)cb * 2u), 4 * R), 4 * R);
#pragma unroll
            for (int k = 0; k < 2 * R; k++) m[k] = (float)hv[k];
        } else {
            __builtin_memcpy(m, __builtin_assume_aligned(a.mask + ((unsigned)r * a.mask_pitch + (unsigned)cb * 4u), R >= 2 ? 16 : 8), 8 * R);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2 * R; k++) m[k] = apply_mask(a, min(cb + k, s.mw - 1), r);
    }
}

// the resampled motion of the run x .. x + R - 1 of plane row y; a pixel past the end of the row gets some in-bounds value, which is not stored
template <int R>
__device__ __forceinline__ void scaled_fetch_down(const ApplyScaledArgs& s, int x, int y, float4 (&f)[R], float (&m)[R]) {
    const ApplyArgs& a = s.a;
    const int cb = 2 * x;
    float4 F0[2 * R];
    float M0[2 * R];
    if (s.rows2) {
        const int r0 = 2 * y, r1 = min(2 * y + 1, s.mh - 1);
        float4 F1[2 * R];
        float M1[2 * R];
#pragma unroll
        for (int k = 0; k < 2 * R; k++) { const int c = min(cb + k, s.mw - 1); F0[k] = apply_flow(a, c, r0); F1[k] = apply_flow(a, c, r1); }
        scaled_mask_span<R>(s, r0, cb, M0);
        scaled_mask_span<R>(s, r1, cb, M1);
#pragma unroll
        for (int i = 0; i < R; i++) {
            const float4 q = scaled_mul(scaled_add(scaled_add(F0[2 * i], F0[2 * i + 1]), scaled_add(F1[2 * i], F1[2 * i + 1])), 0.25f);
            f[i] = scaled_mul(q, 0.5f);
            m[i] = ((M0[2 * i] + M0[2 * i + 1]) + (M1[2 * i] + M1[2 * i + 1])) * 0.25f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2 * R; k++) F0[k] = apply_flow(a, min(cb + k, s.mw - 1), y);
        scaled_mask_span<R>(s, y, cb, M0);
#pragma unroll
        for (int i = 0; i < R; i++) {
            const float4 q = scaled_mul(scaled_add(F0[2 * i], F0[2 * i + 1]), 0.5f);
            f[i] = make_float4(q.x * 0.5f, q.y, q.z * 0.5f, q.w);
            m[i] = (M0[2 * i] + M0[2 * i + 1]) * 0.5f;
        }
    }
}

template <int R>
__device__ __forceinline__ void scaled_fetch_up(const ApplyScaledArgs& s, int x, int y, float4 (&f)[R], float (&m)[R]) {
    const ApplyArgs& a = s.a;
    const int i0 = y >> 1, in = (y & 1) ? min(i0 + 1, s.mh - 1) : max(i0 - 1, 0);
    if constexpr (R == 1) {
        const int j = min(x >> 1, s.mw - 1), jn = (x & 1) ? min(j + 1, s.mw - 1) : max(j - 1, 0);
        const float4 a0 = apply_flow(a, j, i0), a1 = apply_flow(a, jn, i0), b0 = apply_flow(a, j, in), b1 = apply_flow(a, jn, in);
        const float ma0 = apply_mask(a, j, i0), ma1 = apply_mask(a, jn, i0), mb0 = apply_mask(a, j, in), mb1 = apply_mask(a, jn, in);
        const float4 h0 = scaled_add(scaled_mul(a0, 0.75f), scaled_mul(a1, 0.25f)), h1 = scaled_add(scaled_mul(b0, 0.75f), scaled_mul(b1, 0.25f));
        f[0] = scaled_mul(scaled_add(scaled_mul(h0, 0.75f), scaled_mul(h1, 0.25f)), 2.f);
        m[0] = (ma0 * 0.75f + ma1 * 0.25f) * 0.75f + (mb0 * 0.75f + mb1 * 0.25f) * 0.25f;
    } else {      // x is even: pixel x + i sits in column j0 + i / 2, its neighbour is the next column for odd i and the one before for even i
        constexpr int C = R / 2 + 2;
        const int j0 = x >> 1;
        float4 A[C], B[C];
        float MA[C], MB[C];
#pragma unroll
        for (int k = 0; k < C; k++) {
            const int c = min(max(j0 - 1 + k, 0), s.mw - 1);
            A[k] = apply_flow(a, c, i0); B[k] = apply_flow(a, c, in);
            MA[k] = apply_mask(a, c, i0); MB[k] = apply_mask(a, c, in);
        }
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int kj = 1 + i / 2, kn = (i & 1) ? kj + 1 : kj - 1;
            const float4 h0 = scaled_add(scaled_mul(A[kj], 0.75f), scaled_mul(A[kn], 0.25f)), h1 = scaled_add(scaled_mul(B[kj], 0.75f), scaled_mul(B[kn], 0.25f));
            f[i] = scaled_mul(scaled_add(scaled_mul(h0, 0.75f), scaled_mul(h1, 0.25f)), 2.f);
            m[i] = (MA[kj] * 0.75f + MA[kn] * 0.25f) * 0.75f + (MB[kj] * 0.75f + MB[kn] * 0.25f) * 0.25f;
        }
    }
}

// apply_run (apply_motion.h) from its taps on, on the motion f, m of the run: the same operations in the same order
template <typename T, int R, bool PAIR>
__device__ __forceinline__ void apply_scaled_blend(const ApplyArgs& a, int x, int y, const float4 (&f)[R], const float (&m)[R]) {
    const int nv = min(R, a.w - x);
    ApplyTaps t0[R], t1[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        const int xi = min(x + i, a.w - 1);
        t0[i] = apply_taps(xi, y, f[i].x, f[i].y, a.w, a.h, a.wp, a.hp);
        t1[i] = apply_taps(xi, y, f[i].z, f[i].w, a.w, a.h, a.wp, a.hp);
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

// the grid of k_apply_motion over the PLANE: apply_blocks_x(ws, R) * hs workgroups of 256 runs of one plane row, remapped to bands of rows per XCD
template <typename T, int R, bool PAIR, int MODE>
__global__ void __launch_bounds__(256) k_apply_motion_scaled(const ApplyScaledArgs s, int nbx) {
    const int L = apply_block_index();
    const int y = L / nbx, bx = L - y * nbx;
    const int x = (bx * 256 + (int)threadIdx.x) * R;
    if (x >= s.a.w || y >= s.a.h) return;
    float4 f[R];
    float m[R];
    if constexpr (MODE == APPLY_MODE_DOWN) scaled_fetch_down<R>(s, x, y, f, m);
    else scaled_fetch_up<R>(s, x, y, f, m);
    apply_scaled_blend<T, R, PAIR>(s.a, x, y, f, m);
}

// ---- host side ----
// planes of one column take the one-pixel form with four single tap loads; every other plane the vector form where its stores are aligned, else the one-pixel form
template <typename T, int MODE>
static inline void launch_apply_scaled_t(hipStream_t st, const ApplyScaledArgs& s, bool force_scalar) {
    const ApplyArgs& a = s.a;
    constexpr int RV = ApplyRun<T>::R;
    const bool vec = a.w >= 2 && !force_scalar && apply_vector_ok<T>(a);
    const int nbx = apply_blocks_x(a.w, vec ? RV : 1);
    const dim3 g((unsigned)nbx * (unsigned)a.h);
    if (vec) hipLaunchKernelGGL((k_apply_motion_scaled<T, RV, true, MODE>), g, dim3(256), 0, st, s, nbx);
    else if (a.w >= 2) hipLaunchKernelGGL((k_apply_motion_scaled<T, 1, true, MODE>), g, dim3(256), 0, st, s, nbx);
    else hipLaunchKernelGGL((k_apply_motion_scaled<T, 1, false, MODE>), g, dim3(256), 0, st, s, nbx);
}
template <int MODE>
static inline void launch_apply_scaled_m(hipStream_t st, const ApplyScaledArgs& s, int sample, bool force_scalar) {
    if (sample == RIFE_HIP_SAMPLE_U8) launch_apply_scaled_t<uint8_t, MODE>(st, s, force_scalar);
    else if (sample == RIFE_HIP_SAMPLE_U16) launch_apply_scaled_t<uint16_t, MODE>(st, s, force_scalar);
    else if (sample == RIFE_HIP_SAMPLE_F16) launch_apply_scaled_t<_Float16, MODE>(st, s, force_scalar);
    else launch_apply_scaled_t<float, MODE>(st, s, force_scalar);
}
// shift_x = -1 (shift_y = -1: 4:2:0, 0: 4:2:2) or +1; shift 0 is launch_apply
static inline void launch_apply_scaled(hipStream_t st, ApplyScaledArgs s, int shift_x, int shift_y, int sample, bool force_scalar = false) {
    s.rows2 = shift_y < 0;
    s.mask_wide = reinterpret_cast<uintptr_t>(s.a.mask) % 16 == 0 && s.a.mask_pitch % 16 == 0;
    if (shift_x < 0) launch_apply_scaled_m<APPLY_MODE_DOWN>(st, s, sample, force_scalar);
    else launch_apply_scaled_m<APPLY_MODE_UP>(st, s, sample, force_scalar);
}

}  // namespace rife
