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
#pragma once
#include <hip/hip_runtime.h>

#include "elementwise.h"
#include "flow_cascade_geom.h"

namespace rife {

// level L of the tile at (x0, y0) into LDS: rows of pitch(L) records, of which the first sx.n x sy.n exist
template <int L>
__device__ __forceinline__ void cascade_stage(const float* __restrict__ flow, float4* cells, int x0, int y0, int wp, int hp, fcg::Span& sx, fcg::Span& sy) {
    constexpr int S = fcg::scale(L), P2 = fcg::pitch(L) * 2, N2 = fcg::records(L) * 2;
    const int Wb = wp / S;
    sx = fcg::span(x0, fcg::TILE_W, wp, S);
    sy = fcg::span(y0, fcg::TILE_H, hp, S);
    const float4* src = reinterpret_cast<const float4*>(flow) + ((size_t)sy.lo * Wb + sx.lo) * 2;
    float4* dst = cells + fcg::offset(L) * 2;
    for (int j = threadIdx.x; j < N2; j += fcg::THREADS) {
        const int r = j / P2, q = j - r * P2;
        if (r < sy.n && q < 2 * sx.n) dst[j] = src[(size_t)r * Wb * 2 + q];
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

template <int NL>
__global__ __launch_bounds__(fcg::THREADS) void k_flow_cascade(const float* __restrict__ flow0, const float* __restrict__ flow1, const float* __restrict__ flow2,
                                                               float4* __restrict__ F, float* __restrict__ M, int wp, int hp) {
    static_assert(NL == 2 || NL == 3, "the cascade after block 1 or after block 2");
    __shared__ float4 cells[fcg::lds_records(NL) * 2];
    const int x0 = blockIdx.x * fcg::TILE_W, y0 = blockIdx.y * fcg::TILE_H;
    fcg::Span sx0, sy0, sx1, sy1, sx2 = {0, 0}, sy2 = {0, 0};
    cascade_stage<0>(flow0, cells, x0, y0, wp, hp, sx0, sy0);
    cascade_stage<1>(flow1, cells, x0, y0, wp, hp, sx1, sy1);
    if (NL == 3) cascade_stage<2>(flow2, cells, x0, y0, wp, hp, sx2, sy2);
    __syncthreads();
    const int x = x0 + (threadIdx.x & 63);
    if (x >= wp) return;
    constexpr int ROWS = fcg::TILE_H / (fcg::THREADS / 64);      // rows of one wave
    const int yw = y0 + (threadIdx.x >> 6) * ROWS;
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
