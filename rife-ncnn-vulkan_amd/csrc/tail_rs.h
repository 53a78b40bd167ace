// tail_rs_kernel: the output side of rife-v4.6 in one row-streaming kernel - the head of the finest IFBlock (Deconvolution 4x4 stride 2 pad 1,
// 64 -> 24 channels, + PixelShuffle(2): reference models/rife-v4.6/flownet.param:200-201) and the tail of the graph (:202-217: F += flow3[0:4],
// M += flow3[4], Sigmoid, 2x rife.Warp (src/warp.cpp:96-168), blend) + the postproc (src/rife_postproc.comp:39-62), from the last S16 trunk tensor,
// F, M and the frames straight to the u8 frame.  Round 3; replaces head_h2_kernel<EPI_FINAL, true> (head_h2.h), a tile kernel that re-staged its
// weights per 8 x 32 tile and finished its eight pixels per lane one after the other - sixteen dependent memory round trips per lane.
//
// A workgroup (512 threads, two per CU) walks DOWN a strip of 32 quarter-resolution columns; one step = one quarter-resolution row of the trunk
// = a 4 x 128 block of output pixels, ONE PIXEL PER THREAD:
//   deconv   wave w: output parity w & 3 (a 2 x 2-tap convolution over the 3 x 3 neighbourhood, head_uses) x K half w >> 2 (two of the four
//            16-channel chunks): 16 MFMAs on 8 register-resident weight fragments; the pixel operands come from an LDS ring of four trunk
//            rows (conv_rs.h's row layout; one new row per step, loaded a step ahead).  Waves 4-7 hand their partial sums to waves 0-3
//            through LDS, which add the bias and scatter the PixelShuffle result as five planes (dx, dy, dz, dw, dm) x 4 rows x 128 columns.
//   tail     every thread: F, M of its pixel (loaded a step ahead) + the deltas -> the two warps' tap loads are ISSUED (warp_issue) and stay
//            in flight until the next step, where the pixel is finished (warp_finish, sigmoid, blend, quantise) and a wave's 64 pixels leave
//            as 48 dwords.
// Three LDS-only barriers per step.  Arithmetic per pixel is k_final's in its order; the deconvolution sums its four K chunks as two partial
// sums instead of one chain: last-bit differences of the flow deltas against head_h2_kernel (tests/test_gpu_tail_rs.py holds the two together).
// LDS: ring 4 x 8,704 B + partial sums 16 KB + delta planes 10 KB + bias = 61,568 B: two workgroups per CU.
#pragma once
#include "head_h2.h"

namespace rife {

constexpr int TRS_ROWB = 8 * 34 * 32;                 // one trunk row of the strip: [chunk 4][hi | lo][34 px][32 B] = 8,704
constexpr int TRS_SEG = 34 * 32;
constexpr int TRS_LDS_PART = 4 * TRS_ROWB;            // 34,816: partial sums of waves 4-7, [parity 4][quad 4][lane 64][16 B]
constexpr int TRS_LDS_DELTA = TRS_LDS_PART + 4 * 4096; // 51,200: [plane 5][row 4][column 128] fp32
constexpr int TRS_LDS_BIAS = TRS_LDS_DELTA + 5 * 4 * 128 * 4;    // 61,440: bias[32]
constexpr int TRS_LDS = TRS_LDS_BIAS + 128;               // 61,568
constexpr int TRS_NTHR = 512;

struct TailRsArgs {
    const unsigned char* in;     // S16 trunk tensor (64 channels), allocation start
    const void* w;               // head weights: f16 [chunk 4][pair 16][k half 2][32][8] (pack_weights_head_h2)
    const float* bias;           // [32] (24 real)
    const uint32_t *img0, *img1;
    const float4* F; const float* M;
    uint8_t* out;                // u8 HWC RGB, w x h
    int w_, h_, wp, hp;          // frame, padded frame
    int Hq, Wq;                  // trunk resolution (hp / 4, wp / 4)
    int pitch; unsigned plane;   // S16 geometry
    int nunits;                  // strips x Hq
};

// bench-only ablation bits of TAG (rife_hip_bench_tail_rs; results are garbage).  The product instantiates TAG = 0.
enum { TRS_NOTAPS = 1, TRS_NOFM = 2, TRS_NOMATH = 4, TRS_NOSTORE = 8, TRS_NOPIX = 16, TRS_NOROW = 32 };

// Global stores the compiler does not see.  vmcnt counts loads and stores together and they retire out of order with respect to each other, so
// with a store it knows to be in flight the compiler waits vmcnt(0) before the next use of ANY loaded value - in a loop that keeps loads in flight
// across iterations that drains the prefetch every step (measured: 165 -> ... us).  An untracked store only makes the compiler's counted waits
// conservative (the counter also holds the store: reaching "at most N outstanding" then needs one more completion, and loads still complete in
// order), and nobody in this kernel reads what it stored.
__device__ __forceinline__ void trs_store_dword(uint8_t* base, unsigned off, uint32_t v) {
    asm volatile("global_store_dword %0, %1, %2" :: "v"(off), "v"(v), "s"(base) : "memory");
}
__device__ __forceinline__ void trs_store_byte(uint8_t* base, unsigned off, uint32_t v) {
    asm volatile("global_store_byte %0, %1, %2" :: "v"(off), "v"(v), "s"(base) : "memory");
}

#define TRS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

__device__ __forceinline__ void trs_put_short(uint8_t* base, unsigned off, uint32_t v) {
    asm volatile("global_store_short %0, %1, %2" :: "v"(off), "v"(v), "s"(base) : "memory");
}
// One finished pixel of a deep-colour frame (PX = 1: three u16 codes, 2: one A2B10G10R10 dword, alpha 3), pixel index i = oy * w + ox: the packed
// format leaves as one aligned dword per lane - 256 contiguous bytes per wave - instead of depth 8's shuffled 48 dwords.
template <int PX>
__device__ __forceinline__ void trs_put_px10(uint8_t* base, unsigned i, uint32_t pk) {
    if (PX == 2) trs_store_dword(base, i * 4u, pk | 0xc0000000u);
    else { trs_put_short(base, i * 6u, pk & 0x3ffu); trs_put_short(base, i * 6u + 2u, (pk >> 10) & 0x3ffu); trs_put_short(base, i * 6u + 4u, (pk >> 20) & 0x3ffu); }
}

// The motion stores (MotionArgs, elementwise.h; include/rife_hip.h "motion export"), untracked like the frame's: one vector store per pixel for the flow (16 bytes, or 8
// as halves), one element for the mask.  A store of more than 8 bytes needs TWO wait states on gfx950 before a VALU instruction may overwrite its data registers; the
// compiler inserts them for stores it emits, not for one it cannot see: the s_nop 1 is those wait states (stem_rs.h srs_store_b128).
__device__ __forceinline__ void trs_store_dwordx4(uint8_t* base, unsigned off, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" :: "v"(off), "v"(v), "s"(base) : "memory");
}
typedef uint32_t trs_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void trs_store_dwordx2(uint8_t* base, unsigned off, trs_u32x2 v) {
    asm volatile("global_store_dwordx2 %0, %1, %2" :: "v"(off), "v"(v), "s"(base) : "memory");
}
__device__ __forceinline__ void trs_put_flow(const MotionArgs& mo, int x, int y, const float4 f) {
    if (!mo.flow) return;                                                // wave-uniform, like the format
    if (mo.format == RIFE_HIP_MOTION_F16) { const uint2 hh = motion_half4(f); trs_store_dwordx2(mo.flow, (unsigned)y * mo.flow_pitch + (unsigned)x * 8u, trs_u32x2{hh.x, hh.y}); }
    else trs_store_dwordx4(mo.flow, (unsigned)y * mo.flow_pitch + (unsigned)x * 16u, f32x4{f.x, f.y, f.z, f.w});
}
__device__ __forceinline__ void trs_put_mask(const MotionArgs& mo, int x, int y, const float m) {
    if (!mo.mask) return;
    if (mo.format == RIFE_HIP_MOTION_F16) trs_put_short(mo.mask, (unsigned)y * mo.mask_pitch + (unsigned)x * 2u, motion_half(m));
    else trs_store_dword(mo.mask, (unsigned)y * mo.mask_pitch + (unsigned)x * 4u, __float_as_uint(m));
}

// PX (include/rife_hip.h RIFE_HIP_PIX_*): 0 = u8 frames; 1 / 2 = 10:10:10 frames in, RGB10_U16 / A2B10G10R10 out (k_final_px<PX>'s arithmetic);
// 4 = RGBA8: depth-8 frames with alpha in byte 3, finished from the taps already loaded (warp_finish_a) and stored as one aligned dword per lane
template <int TAG, int PX = 0>
__global__ __launch_bounds__(TRS_NTHR) __attribute__((amdgpu_waves_per_eu(4, 4))) void tail_rs_kernel(TailRsArgs a) {
#define TRS_MOTION_FLOW(FX, FY, F)
#define TRS_MOTION_MASK(OX, OY, M)
#include "tail_rs_body.h"
#undef TRS_MOTION_FLOW
#undef TRS_MOTION_MASK
}
// A motion call's kernel (include/rife_hip.h "motion export"): the same body on the same grid, + the motion stores under the frame's validity test.  A kernel of its own,
// so that the plain kernel keeps its name, its argument struct and its machine code.
template <int PX>
__global__ __launch_bounds__(TRS_NTHR) __attribute__((amdgpu_waves_per_eu(4, 4))) void tail_rs_motion_kernel(TailRsArgs a, MotionArgs mo) {
    [[maybe_unused]] constexpr int TAG = 0;      // the bench-only ablation bits of the plain kernel: none here
#define TRS_MOTION_FLOW(FX, FY, F) if ((FY) < a.h_ && (FX) < a.w_) trs_put_flow(mo, FX, FY, F);
#define TRS_MOTION_MASK(OX, OY, M) if (valid) trs_put_mask(mo, OX, OY, M);
#include "tail_rs_body.h"
#undef TRS_MOTION_FLOW
#undef TRS_MOTION_MASK
}

}  // namespace rife
