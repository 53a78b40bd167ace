// apply_yuv.h: the luma plane AND both chroma planes of a 4:2:0 / 4:2:2 image in ONE launch (include/rife_hip.h "high bit depth"): the bytes of launch_apply on the
// luma set followed by launch_apply_scaled on the chroma set (apply_motion.h, apply_scaled.h), with the motion read once instead of twice.
// A lane owns a run of R chroma pixels of one chroma row and the 2 R x 2 (4:2:2: 2 R x 1) luma pixels under it.  It issues the 2 R motion pixels of each of its
// motion rows once - flow pixels as apply_flow loads them, the mask spans as scaled_mask_span loads them - all before the first add, then
//   luma     one luma row at a time (the taps of the two rows never coexist), apply_scaled_blend<T, 2 R> on the motion AS LOADED: apply_run's operations from the taps on;
//   chroma   scaled_fetch_down's box mean of the same registers (the same sums in the same order), then apply_scaled_blend<T, R> on the chroma planes.
// Nothing of apply_taps / apply_issue / apply_finish / apply_quant or of the XCD band remap is restated.  A full luma run is one 8-byte store, a full chroma run one
// 4-byte store per plane (T = u16, R = 2); the host launches this kernel only where those stores are aligned and the luma plane has at least 4 columns (so both
// planes take the paired tap loads), and the two existing launches everywhere else.  Every motion index is clamped into mw x mh, every tap address into its plane
// (apply_taps); nothing but the output samples is written.  32-bit byte offsets as in apply_motion.h.  No LDS, no atomics.
#pragma once

namespace rife {

struct ApplyYuvArgs {
    ApplyScaledArgs c;            // the chroma set as launch_apply_scaled takes it: a = the chroma planes and the motion, mw x mh, rows2, mask_wide
    ApplyArgs y;                  // the luma set as launch_apply takes it: w x h = mw x mh, the same motion
};

// grid: apply_blocks_x(cw, R) * ch workgroups of 256 chroma runs of one chroma row, remapped to bands of rows per XCD
template <typename T, int R, bool ROWS2>
__global__ void __launch_bounds__(256) k_apply_yuv(const ApplyYuvArgs s, int nbx) {
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
    // the chroma motion first, while both rows are at hand (F0 is dead after the first luma row): scaled_fetch_down's sums in its order
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
    apply_scaled_blend<T, 2 * R, true>(s.y, cb, r0, F0, M0);
    if constexpr (ROWS2) {
        if (2 * cy + 1 < s.y.h) apply_scaled_blend<T, 2 * R, true>(s.y, cb, 2 * cy + 1, F1, M1);      // r1 == 2 cy + 1 here
    }
    apply_scaled_blend<T, R, true>(a, cx, cy, f, m);
}

// ---- host side ----
// the fused launch serves u16 sets whose luma stores (8 bytes) and chroma stores (4 bytes) are aligned and whose luma plane has at least 4 columns
static inline bool apply_yuv_ok(const ApplyArgs& y, const ApplyArgs& c, int sample) {
    if (sample != RIFE_HIP_SAMPLE_U16 || y.w < 4) return false;
    for (int k = 0; k < y.n; k++) if (reinterpret_cast<uintptr_t>(y.out[k]) % 8 || y.pitcho[k] % 8) return false;
    for (int k = 0; k < c.n; k++) if (reinterpret_cast<uintptr_t>(c.out[k]) % 4 || c.pitcho[k] % 4) return false;
    return true;
}
// s.c.a / s.y: apply_args of the chroma and the luma set on the SAME motion of s.c.mw x s.c.mh; shift_y = -1 (4:2:0) or 0 (4:2:2); the caller has asked apply_yuv_ok
static inline void launch_apply_yuv(hipStream_t st, ApplyYuvArgs s, int shift_y) {
    constexpr int R = ApplyRun<uint16_t>::R;
    s.c.rows2 = shift_y < 0;
    s.c.mask_wide = reinterpret_cast<uintptr_t>(s.c.a.mask) % 16 == 0 && s.c.a.mask_pitch % 16 == 0;
    const int nbx = apply_blocks_x(s.c.a.w, R);
    const dim3 g((unsigned)nbx * (unsigned)s.c.a.h);
    if (s.c.rows2) hipLaunchKernelGGL((k_apply_yuv<uint16_t, R, true>), g, dim3(256), 0, st, s, nbx);
    else hipLaunchKernelGGL((k_apply_yuv<uint16_t, R, false>), g, dim3(256), 0, st, s, nbx);
}

}  // namespace rife
