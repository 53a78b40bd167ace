// flow_cascade.h: F, M at full resolution from the coarse flows alone (rife-v4.6; flownet.param:47-58, 99-105, 152-158).
//
// After blocks 0 and 1 (and 2) F, M are a pure function of flow0, flow1 (and flow2): k_flow_update<8, true>, then k_flow_update<4, false>
// (then k_flow_update<2, false>).  k_flow_cascade<NL> evaluates that sequence per pixel - up_coeff, RIFE_UP, flow_first, flow_accumulate of elementwise.h in the
// sequence's order, under -ffp-contract=off - so the tensors are the sequence's bit for bit, and F, M are only written, never read:
//   NL = 2 replaces k_flow_update2<8, 4> after block 1;
//   NL = 3 replaces k_flow_update<2, false> after block 2 (20 B / pixel of reads less).
// The loads are shared through LDS: a workgroup owns a TILE_W x TILE_H tile of pixels, copies the flow cells its pixels can touch (flow_cascade_geom.h: the
// range comes from up_coeff's own clamped index at the tile's first and last pixel) as the 32-byte records of flow_b, and after one barrier every thread
// interpolates its pixels from LDS: 488 records (15.6 KB) per 1024 pixels instead of 12 global records per pixel.  One wave stores one row of 64 pixels:
// 1 KB of F and 256 B of M per instruction, as full lines.  No communication between workgroups.
// A thread owns one column of four consecutive rows.  With three levels it forms the horizontal half of the interpolation once per cell row these rows
// touch and the vertical half per pixel (cascade_sample_rows); the first and the last row group of the image, where up_coeff's clamps move the cell rows,
// and the kernel with two levels go pixel by pixel (cascade_sample).
#pragma once
#include <hip/hip_runtime.h>

#include "elementwise.h"
#include "flow_cascade_geom.h"

namespace rife {

// level L of the tile at (x0, y0) into LDS: rows of pitch(L) records, of which the first sx.n x sy.n exist.  In two steps, so that the kernel has the loads
// of all its levels in flight at once and waits for memory one time per tile, not once per 256 half records: cascade_stage_load issues this thread's
// stage_loads(L) loads (a half record outside the staged range re-reads the range's last row / column, so no load is conditional), cascade_stage_write
// puts those inside the range where they belong.
template <int L>
__device__ __forceinline__ void cascade_stage_load(const float* __restrict__ flow, int x0, int y0, int wp, int hp, fcg::Span& sx, fcg::Span& sy,
                                                   float4 (&v)[fcg::stage_loads(L)]) {
    constexpr int S = fcg::scale(L), P2 = fcg::pitch(L) * 2;
    const int Wb = wp / S;
    sx = fcg::span(x0, fcg::TILE_W, wp, S);
    sy = fcg::span(y0, fcg::TILE_H, hp, S);
    const float4* src = reinterpret_cast<const float4*>(flow) + ((size_t)sy.lo * Wb + sx.lo) * 2;
#pragma unroll
    for (int i = 0; i < fcg::stage_loads(L); i++) {
        const int j = threadIdx.x + i * fcg::THREADS;
        const int r = j / P2, q = j - r * P2;
        v[i] = src[(size_t)min(r, sy.n - 1) * Wb * 2 + min(q, 2 * sx.n - 1)];
    }
}
// (the loaded values pass through an empty asm before the conditional writes: otherwise the compiler sinks each load into the branch of its write, behind
// a wait for the one before it)
template <int L>
__device__ __forceinline__ void cascade_stage_arrive(float4 (&v)[fcg::stage_loads(L)]) {
#pragma unroll
    for (int i = 0; i < fcg::stage_loads(L); i++) asm volatile("" : "+v"(v[i].x), "+v"(v[i].y), "+v"(v[i].z), "+v"(v[i].w));
}
template <int L>
__device__ __forceinline__ void cascade_stage_write(float4* cells, const fcg::Span& sx, const fcg::Span& sy, const float4 (&v)[fcg::stage_loads(L)]) {
    constexpr int P2 = fcg::pitch(L) * 2, N2 = fcg::records(L) * 2;
    float4* dst = cells + fcg::offset(L) * 2;
#pragma unroll
    for (int i = 0; i < fcg::stage_loads(L); i++) {
        const int j = threadIdx.x + i * fcg::THREADS;
        const int r = j / P2, q = j - r * P2;
        if (j < N2 && r < sy.n && q < 2 * sx.n) dst[j] = v[i];
    }
}

// u = Interp(S)(flow_L) at pixel (x, y), from the staged cells
template <int L>
__device__ __forceinline__ void cascade_sample(const float4* cells, const fcg::Span& sx, const fcg::Span& sy, int wp, int hp, int x, int y, float4& u, float& um) {
    constexpr int S = fcg::scale(L);
    int cx, cy; float a0, a1, b0, b1;
    up_coeff(x, S, wp / S, cx, a0, a1);
    up_coeff(y, S, hp / S, cy, b0, b1);
    const float* p00 = reinterpret_cast<const float*>(cells + (fcg::offset(L) + (cy - sy.lo) * fcg::pitch(L) + (cx - sx.lo)) * 2);
    flow_upsampled_cells(p00, p00 + fcg::pitch(L) * 8, a0, a1, b0, b1, u, um);
}

// u[k] = Interp(S)(flow_L) at the pixels (x, yw + k) of one thread, from the staged cells, for a row group away from up_coeff's two vertical clamps
// (fcg::group_inner: every group but the first and the last of the image).  The rows of a thread share the column, so RIFE_UP's horizontal stage
// (elementwise.h flow_cell_row) runs once per cell row the group touches - 2, 3, 4 of them for the three levels of k_flow_cascade<3>, its only caller,
// instead of 8 each - and its vertical stage per pixel: the same sub-expressions in the same order, so the bits of flow_upsampled_cells.  Which cell rows
// row k blends is a constant of k and the level
// (flow_cascade_geom.h; tests/sanitize/flow_cascade_rows_main.cpp holds it against up_coeff for every height).
template <int L>
__device__ __forceinline__ void cascade_sample_rows(const float4* cells, const fcg::Span& sx, const fcg::Span& sy, int wp, int hp, int x, int yw,
                                                    float4 (&u)[fcg::ROWS], float (&um)[fcg::ROWS]) {
    constexpr int S = fcg::scale(L), NR = fcg::group_rows(L);
    int cx; float a0, a1;
    up_coeff(x, S, wp / S, cx, a0, a1);
    const float* p = reinterpret_cast<const float*>(cells + (fcg::offset(L) + (fcg::group_first(yw, L, hp) - sy.lo) * fcg::pitch(L) + (cx - sx.lo)) * 2);
    FlowCellRow h[NR];
#pragma unroll
    for (int j = 0; j < NR; j++) h[j] = flow_cell_row(p + j * (fcg::pitch(L) * 8), a0, a1);
#pragma unroll
    for (int k = 0; k < fcg::ROWS; k++) {
        int cy; float b0, b1;
        up_coeff(yw + k, S, hp / S, cy, b0, b1);
        flow_cell_rows_blend(h[fcg::group_rel_inner(k, L)], h[fcg::group_rel_inner(k, L) + 1], b0, b1, u[k], um[k]);
    }
}

template <int NL>
__global__ __launch_bounds__(fcg::THREADS) void k_flow_cascade(const float* __restrict__ flow0, const float* __restrict__ flow1, const float* __restrict__ flow2,
                                                               float4* __restrict__ F, float* __restrict__ M, int wp, int hp) {
    static_assert(NL == 2 || NL == 3, "the cascade after block 1 or after block 2");
    __shared__ float4 cells[fcg::lds_records(NL) * 2];
    const int x0 = blockIdx.x * fcg::TILE_W, y0 = blockIdx.y * fcg::TILE_H;
    fcg::Span sx0, sy0, sx1, sy1, sx2 = {0, 0}, sy2 = {0, 0};
    {
        float4 v0[fcg::stage_loads(0)], v1[fcg::stage_loads(1)], v2[fcg::stage_loads(2)];
        cascade_stage_load<0>(flow0, x0, y0, wp, hp, sx0, sy0, v0);
        cascade_stage_load<1>(flow1, x0, y0, wp, hp, sx1, sy1, v1);
        if (NL == 3) cascade_stage_load<2>(flow2, x0, y0, wp, hp, sx2, sy2, v2);
        cascade_stage_arrive<0>(v0);
        cascade_stage_arrive<1>(v1);
        if (NL == 3) cascade_stage_arrive<2>(v2);
        cascade_stage_write<0>(cells, sx0, sy0, v0);
        cascade_stage_write<1>(cells, sx1, sy1, v1);
        if (NL == 3) cascade_stage_write<2>(cells, sx2, sy2, v2);
    }
    __syncthreads();
    const int x = x0 + (threadIdx.x & 63);
    if (x >= wp) return;
    constexpr int ROWS = fcg::ROWS;                               // rows of one wave
    const int yw = y0 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * ROWS;
    // (measured at 4K: the shared rows take 2.4 us off NL = 3 and add 0.8 us to NL = 2, which stays pixel by pixel)
    if (NL == 3 && fcg::group_inner(yw, hp)) {                    // level by level, in the sequence's order per pixel
        float4 f[ROWS], u[ROWS]; float m[ROWS], um[ROWS];
        cascade_sample_rows<0>(cells, sx0, sy0, wp, hp, x, yw, u, um);
#pragma unroll
        for (int k = 0; k < ROWS; k++) flow_first_of<8>(u[k], um[k], f[k], m[k]);
        cascade_sample_rows<1>(cells, sx1, sy1, wp, hp, x, yw, u, um);
#pragma unroll
        for (int k = 0; k < ROWS; k++) flow_accumulate<4>(u[k], um[k], f[k], m[k]);
        cascade_sample_rows<2>(cells, sx2, sy2, wp, hp, x, yw, u, um);
#pragma unroll
        for (int k = 0; k < ROWS; k++) flow_accumulate<2>(u[k], um[k], f[k], m[k]);
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            const int y = yw + k;
            if (y >= hp) break;
            const size_t i = (size_t)y * wp + x;
            F[i] = f[k];
            M[i] = m[k];
        }
        return;
    }
    // pixel by pixel: NL = 2, and the image's first and last row group (up_coeff's clamps move the cell rows)
#pragma unroll
    for (int k = 0; k < ROWS; k++) {
        const int y = yw + k;
        if (y >= hp) break;
        float4 f, u; float m, um;
        cascade_sample<0>(cells, sx0, sy0, wp, hp, x, y, u, um);
        flow_first_of<8>(u, um, f, m);
        cascade_sample<1>(cells, sx1, sy1, wp, hp, x, y, u, um);
        flow_accumulate<4>(u, um, f, m);
        if (NL == 3) {
            cascade_sample<2>(cells, sx2, sy2, wp, hp, x, y, u, um);
            flow_accumulate<2>(u, um, f, m);
        }
        const size_t i = (size_t)y * wp + x;
        F[i] = f;
        M[i] = m;
    }
}

template <int NL>
static inline void launch_flow_cascade(hipStream_t st, const float* flow0, const float* flow1, const float* flow2, float4* F, float* M, int wp, int hp) {
    const dim3 g(fcg::tiles(wp, fcg::TILE_W), fcg::tiles(hp, fcg::TILE_H));
    hipLaunchKernelGGL((k_flow_cascade<NL>), g, dim3(fcg::THREADS), 0, st, flow0, flow1, flow2, F, M, wp, hp);
}

}  // namespace rife
