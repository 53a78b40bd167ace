// head_h2_kernel<TAG>: the IFBlock head of rife-v4 — Deconvolution 4x4 stride 2 pad 1 (C -> 24) + PixelShuffle(2)
// (flownet.param:45-46, 97-98, 150-151, 200-201) on the f16 matrix pipe with the split-f16 scheme of conv_h2_kernel.
// All four output parities of the transposed convolution are computed by one workgroup from one staged input tile:
// parity (py, px) is a 2x2-tap convolution over the 3x3 neighbourhood, so each of the 9 neighbourhood taps feeds 1, 2
// or 4 of the four 32-wide accumulators (16 (tap, parity) pairs in total; 24 of 32 channels are real).
//   8 waves, tile = 8 rows x 32 columns of trunk pixels, chunk = 16 channels, input double buffered, weight slab single
//   buffered (2 x 27.2 KB + 16 KB = 70.4 KB -> two workgroups per CU).
//   Epilogue: + bias, PixelShuffle scatter into the flow tensor [4H][4W][8].
#pragma once
#include "conv_mfma.h"
#include "elementwise.h"

namespace rife {

// (tap, parity) pair table: tap = dy*3 + dx over the 3x3 neighbourhood (dy, dx in 0..2 <-> offsets -1..+1).
// parity p uses offset 0 and (p ? +1 : -1) in each axis (see pack_weights: out(2y+p) <- in(y+d) through kernel row k).
__device__ __forceinline__ constexpr bool head_uses(int t, int par) {
    const int dy = t / 3 - 1, dx = t % 3 - 1, py = par >> 1, px = par & 1;
    const bool uy = dy == 0 || dy == (py ? 1 : -1);
    const bool ux = dx == 0 || dx == (px ? 1 : -1);
    return uy && ux;
}
__device__ __forceinline__ constexpr int head_pair_index(int t, int par) {   // position of (t, par) in the packed order
    int n = 0;
    for (int tt = 0; tt < 9; tt++)
        for (int pp = 0; pp < 4; pp++) {
            if (tt == t && pp == par) return n;
            if (head_uses(tt, pp)) n++;
        }
    return -1;
}

// extra inputs of the fused tail (EPI_FINAL): everything k_final needs besides flow3
struct FinalArgs {
    const uint32_t *img0, *img1;
    const float4* F; const float* M;
    uint8_t* out;           // u8 HWC RGB, w x h (pixfmt 0); RGB10_U16 / A2B10G10R10 / RGBA8 otherwise
    int w, h, wp, hp;
    int pixfmt = 0;         // include/rife_hip.h RIFE_HIP_PIX_*: read by the host code that picks the kernel instantiation, never by a kernel
};
enum { EPI_FINAL = 7 };      // head of block 3 + flownet.param:202-217 + postproc, no flow3 in HBM

constexpr int headh2_lds_bytes() { return 2 * 10 * 34 * 80 + 16 * 2 * 32 * 16; }

// EPI: EPI_DECONV_PS (v4 heads: + PixelShuffle scatter, 24 channels), EPI_DECONV (+ per-channel slope, NHWC store at
// (2y+py, 2x+px)), EPI_DECONV_SIG (sigmoid).  Output channels are tiled by 32 over the grid (a.nz N-tiles per pixel tile).
// S16IN: the input is an S16 tensor (conv_t64.h; a.s16_pitch pixels per row, zero border): staging is a plain 16-byte copy.
// PX (EPI_FINAL only): 0 = u8 frames; 1 / 2 = 10:10:10 frames in, RGB10_U16 / A2B10G10R10 out; 4 = RGBA8 frames (k_final_px<PX>'s arithmetic)
template <int EPI, bool S16IN = false, int PX = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void head_h2_kernel(ConvArgs a, FinalArgs fa) {
#define HD_MOTION(FX, FY, F, M)
#include "head_h2_body.h"
#undef HD_MOTION
}
// A motion call's fused tail (include/rife_hip.h "motion export"): the same body on the same grid, + the motion stores of the lane that finishes the pixel.  A kernel of
// its own, so that the plain kernel keeps its name, its arguments and its machine code.
template <bool S16IN, int PX>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void head_h2_motion_kernel(ConvArgs a, FinalArgs fa, MotionArgs mo) {
    constexpr int EPI = EPI_FINAL;
#define HD_MOTION(FX, FY, F, M) { motion_put_flow(mo, FX, FY, F); motion_put_mask(mo, FX, FY, M); }
#include "head_h2_body.h"
#undef HD_MOTION
}

}  // namespace rife
