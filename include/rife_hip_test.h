/* rife_hip_test.h - TEST SURFACE of librife_hip.so: stage taps and single-kernel entry points that exist for the parity tests (tests/test_gpu_*.py)
 * and tools/parity_report.py.  The product header include/rife_hip.h does not include this file, and a drop-in for src/rife.cpp needs none of it.
 * The symbols are exported by the same library because they must run the PRODUCT's kernels; tests/test_host_and_sharding.py checks that the library
 * exports exactly what the two headers declare. */
#ifndef RIFE_HIP_TEST_H
#define RIFE_HIP_TEST_H

#include "rife_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- stage taps for parity tests (the reference's Extractor can extract / inject `flow0..flow3`,
 * src/rife.cpp:2653-2669; these do the same for the v4 schedule).  Planar CHW fp32 host arrays. ------------- */
int rife_hip_v4_extract_flow(const rife_hip_t* r, const uint8_t* in0_rgb, const uint8_t* in1_rgb, int w, int h,
                             float timestep, int fi, const float* const* inject, int n_inject, float* out6chw);
/* shape of blob flow{fi} for frames of w x h: rife-v4.6 6 x hp/s x wp/s (PixelShuffle output, models/rife-v4.6/flownet.param:46),
 * rife-v4 5 x hp/2s x wp/2s (Deconvolution output, models/rife-v4/flownet.param:33); s = 8, 4, 2, 1. */
int rife_hip_v4_flow_dims(const rife_hip_t* r, int w, int h, int fi, int* channels, int* fh, int* fw);
/* Taps of the gather code on injected flows (rife-v4.6; parity tests of rife.Warp + Interp + Concat as the hot path runs them,
 * src/warp.cpp:96-168, models/rife-v4.6/flownet.param:52-62, 107-115, 160-165, 202-217).  what = 0: the 12-channel input of IFBlock b
 * (1..3) from the unfused assembly kernel; 1: the same tensor read back through the product's fused stem kernel (one-hot weights; values
 * to 2^-22 relative); both 12 x hp/S x wp/S, n_inject = b.  what = 2: blob out0 before the postproc, 3 x hp x wp, n_inject = 4.
 * what = 4 / 3: the running flow F (4 channels) and mask M that IFBlock b's stem reads, 5 x hp x wp, after the flow-update kernel / as
 * written by the stem kernel that applies the last update itself (blocks 2 and 3; flownet.param:99-105, 152-158).
 * what = 5 (b = 3): the 12-channel input of IFBlock 3 read back through the product's row-streaming stem kernel (both of its convolutions with
 * one-hot weights, eight launches; values to 2^-21 relative), 12 x hp x wp.
 * what = 6 (b = 2, 3): F and M, 5 x hp x wp, written by the flow cascade kernel from the b injected flows alone; what = 4 is its reference.
 * what = 7 (b = 0..3, n_inject = b, RGB8): the FIRST S16 trunk tensor of IFBlock b, raw and whole, after the block's stems as a plain pass runs them (assembly +
 * stem-0 + stem-1 for block 0, the fused stem-0 kernel + the S16 stride-2 kernel for blocks 1 - 3, the row-streaming stem kernel where the product uses it;
 * RIFE_HIP_STEM_RS=0 at create time: the two-kernel sequence for block 3).  out_chw then takes rife_hip_op_s16_geom(C, hp / 4 s, wp / 4 s) bytes, C = 192, 128, 96, 64
 * and s = 8, 4, 2, 1 for b = 0..3.  A block that is not on the S16 path at that frame size: -RIFE_HIP_EINVAL. */
int rife_hip_v4_tap(const rife_hip_t* r, const uint8_t* in0_rgb, const uint8_t* in1_rgb, int w, int h, float timestep, int what, int b,
                    const float* const* inject, int n_inject, float* out_chw);
/* The plain pass with blobs flow0 .. flow{n_inject - 1} injected (n_inject = 0..3): the remaining blocks and the fused tail run as in
 * rife_hip_process.  out_rgb: w x h u8 RGB. */
int rife_hip_v4_process_injected(const rife_hip_t* r, const uint8_t* in0_rgb, const uint8_t* in1_rgb, int w, int h, float timestep,
                                 const float* const* inject, int n_inject, uint8_t* out_rgb);
/* The first two taps on frames of format `pixfmt` (include/rife_hip.h RIFE_HIP_PIX_*; rife-v4.6 for the 10-bit formats and RGBA8): the 10-bit gather code
 * under the checks of the 8-bit one.  pixfmt = RIFE_HIP_PIX_RGB8: the calls above.  RIFE_HIP_PIX_RGBA8: the colour taps are those of the RGB8 frames (alpha
 * reaches no stem), and tap what = 2 (the unfused tail before quantisation) returns FOUR planes, 4 x hp x wp: out0's three and the alpha plane. */
int rife_hip_v4_extract_flow_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, int fi, const float* const* inject,
                                int n_inject, float* out6chw, int pixfmt);
int rife_hip_v4_tap_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, int what, int b, const float* const* inject,
                       int n_inject, float* out_chw, int pixfmt);
/* Flow scale (include/rife_hip.h rife_hip_set_flow_scale): rife_hip_v4_extract_flow, rife_hip_v4_flow_dims and rife_hip_v4_process_injected honour the engine's
 * divisor - at 2 the blobs flow0..3 are hp/16 .. hp/2 of the frame padded to 64n.  So do the gather taps (rife_hip_v4_tap, rife_hip_v4_tap_px): at divisor 2 hp, wp
 * are the frame padded to 64n and s = 16, 8, 4, 2, and the taps run the launches of that mode - what = 0 the unfused assembly kernels at 1/16 .. 1/2, what = 1 the
 * fused stem kernels of the mode (one-hot weights, the 10-bit forms for the 10-bit formats), what = 4 F and M after the three plain flow-update launches, what = 7 the
 * block stems as a plain pass runs them.  what = 2, 3, 5, 6 are kernels of the divisor-1 schedule which the product does not launch at divisor 2: -RIFE_HIP_EINVAL
 * with a message that says so.  At either divisor what = 0 also takes b = 0 (n_inject = 0): the 7-channel input of IFBlock 0, 7 x hp/s x wp/s (s = 8 or 16).
 * rife_hip_v4_process_injected_px: flow injection with frames of an RGB format `pixfmt` (out: the same format).  At divisor 2 n_inject may be 4: block 3's update
 * and the tail then run on the four injected blobs alone, in the product's final kernel (k_final_scaled).  At divisor 1: RGB8 and n_inject <= 3, the call above. */
int rife_hip_v4_process_injected_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep,
                                    const float* const* inject, int n_inject, void* out, int pixfmt);

/* ---- single-kernel entry points for per-kernel parity tests (host arrays, planar CHW fp32 like ncnn::Mat) --- */
/* 3x3 conv, pad 1, stride 1|2, + bias, optional residual add (same shape as output), per-channel negative slope
 * (1.0 = none, 0.2 = LeakyReLU(0.2), PReLU slopes otherwise): ncnn Convolution (+BinaryOp add +ReLU/PReLU). */
int rife_hip_op_conv3x3(int gpuid, const float* x_chw, int c, int h, int w, const float* weight_oihw, const float* bias,
                        int outc, int stride, const float* residual_chw, const float* slope, float* out_chw);
/* 4x4 stride-2 pad-1 transposed conv (ncnn Deconvolution, weights [oc][ic][4][4]) + per-channel slope. */
int rife_hip_op_deconv4x4(int gpuid, const float* x_chw, int c, int h, int w, const float* weight_oihw, const float* bias,
                          int outc, const float* slope, float* out_chw);
/* rife.Warp (src/warp.cpp:96-168): image c x h x w, flow 2 x h x w. */
int rife_hip_op_warp(int gpuid, const float* image_chw, const float* flow_chw, int c, int h, int w, float* out_chw);

/* The YUV kernels alone (csrc/yuv.h; pixfmt = a RIFE_HIP_PIX_NV12 .. I420P10, I422, I422P10, I444 or I444P10 format with its colour description): k_preproc_yuv
 * (4:2:2 / 4:4:4: k_preproc_yuvc) on one host frame -> the resident form, hp x wp dwords R | G << 10 | B << 20, zero outside w x h; k_postproc_yuv (k_postproc_yuvc)
 * on h x w A2B10G10R10 dwords -> one frame of `pixfmt`. */
int rife_hip_op_yuv_to_rgb10(int gpuid, const void* yuv, int w, int h, int pixfmt, uint32_t* out_padded);
int rife_hip_op_rgb10_to_yuv(int gpuid, const uint32_t* a2b10g10r10, int w, int h, int pixfmt, void* yuv_out);

/* The pitched kernels alone (csrc/planes.h), on an image whose planes are in HOST memory: the call uploads every plane, gaps between rows included, into one
 * device allocation with the same pitches and the same pointer alignment modulo 16, so the form the host picks is the one it would pick for the caller's planes.
 * force_scalar: 0 = the host's choice, 1 = the scalar form, 2 (image_to_resident only, a TIGHT image) = the tight kernels of the _px path, the reference.
 * image_to_resident: the pre-processing kernel -> the resident form, hp x wp dwords (depth 8: R | G << 8 | B << 16 | A << 24, depth 10: R | G << 10 | B << 20).
 * resident_to_image: tight_frame = what the pass leaves behind - for a YUV or planar RGB format h x w A2B10G10R10 dwords (k_postproc_yuv's / k_postproc_rgbp's
 * input; csrc/planar_rgb.h serves tight frames and pitched planes with one kernel set, so these two calls reach every form of it), for a packed RGB format the tight
 * frame of that format (the store kernel's input); the planes come back with every byte the kernel did not write as it went in. */
int rife_hip_op_image_to_resident(int gpuid, const rife_hip_image_t* host_img, int force_scalar, uint32_t* out_padded);
int rife_hip_op_resident_to_image(int gpuid, const uint32_t* tight_frame, const rife_hip_image_t* host_img_out, int force_scalar);

/* ---- the pre-split {hi, lo} f16 ("S16") trunk kernels alone (csrc/conv_t64.h, conv_rs.h, conv_rs2.h, conv_row.h, conv_ks.h), one launch per layer, on RAW S16
 * tensors in host memory: 2 C / 16 planes [16-channel chunk][hi | lo] of rows x pitch pixels of 32 bytes, pixel (y, x) at (y + 1, x + 1), zero borders.
 * op_s16_geom: the geometry of the tensor of a C x H x W trunk (S16Geom, csrc/engine_dispatch.h); needs no device. */
int rife_hip_op_s16_geom(int C, int H, int W, int* pitch, int* rows, unsigned* plane_bytes, size_t* bytes);
/* n_layers (1, 2) residual layers y = leaky(conv3x3(x) + bias + x) through the product's launcher of `kernel`, built by the product's layer upload as the engine
 * builds a trunk layer.  weight [n][C][C][3][3] (exactly fp16 values), bias [n][C], slope [n] (one slope per layer).  in_s16[nb] / out_s16[nb]: tensors of `bytes`
 * each; out_s16 is uploaded as given, the launches run in_s16 -> out_s16 (-> in_s16 for the second layer; RIFE_HIP_TRUNK_RS2: both layers in one launch), and the
 * final tensor comes back in out_s16.  flip: the walking direction of the first launch (conv_t64: reverse, conv_rs / conv_rs2: descend), alternating per launch.
 * cus > 0: persistent grids sized for that many compute units during the call (0 = the chip).  nb = 1 .. 4 tensors; nb > 1: the batched form of ROW / KS only.
 * Shapes a launcher refuses (conv_rs below 7 rows, conv_rs2 below RS2_MIN_ROWS rows per segment, a channel count the kernel does not serve, weights that are not
 * fp16, nb > 4) return -RIFE_HIP_EINVAL before anything is launched. */
enum { RIFE_HIP_TRUNK_T64 = 0, RIFE_HIP_TRUNK_RS = 1, RIFE_HIP_TRUNK_RS2 = 2, RIFE_HIP_TRUNK_ROW = 3, RIFE_HIP_TRUNK_KS = 4 };
int rife_hip_op_trunk(int gpuid, int kernel, int C, int H, int W, int n_layers, const float* weight, const float* bias, const float* slope, int flip, int cus,
                      int nb, const void* const* in_s16, void* const* out_s16);
/* the same with the launchers' precision (include/rife_hip.h RIFE_HIP_PRECISION_*): FULL is rife_hip_op_trunk byte for byte, FAST launches the fast-precision
 * instantiation of the same kernel on the same grid - acc = sum over the weight taps of W . hi(x) + I . (hi(x) + lo(x)), the epilogue unchanged.  conv_ks has no
 * fast form (-RIFE_HIP_ENOSYS); an unknown precision is -RIFE_HIP_EINVAL. */
int rife_hip_op_trunk_prec(int gpuid, int kernel, int C, int H, int W, int n_layers, const float* weight, const float* bias, const float* slope, int flip, int cus,
                           int nb, const void* const* in_s16, void* const* out_s16, int precision);

/* ---- the two ENDS of the S16 trunk alone: the kernel that writes the first S16 tensor of a block and the kernel that reads the last one, one launch each, through
 * the product's layer upload with the flags rife_hip_load sets and the product's launcher (launch_conv).  C = 64, 96, 128, 192; anything else, and weights that are
 * not exactly fp16, return -RIFE_HIP_EINVAL before anything is uploaded or launched.
 * op_stem1_s16: stem-1, the 3x3 stride-2 convolution C/2 -> C + bias + LeakyReLU(slope) with the S16 epilogue (conv_h2s2_kernel<NS, true>, weights packed with the
 * row permutation of the S16 kernels).  x_chw: C/2 x 2 Ht x 2 Wt fp32 (the kernel reads it as NHWC, ld = C/2); weight [C][C/2][3][3], bias [C]; out_s16: a raw S16
 * tensor of op_s16_geom(C, Ht, Wt), uploaded as given, and the whole tensor comes back after the launch. */
int rife_hip_op_stem1_s16(int gpuid, int C, int Ht, int Wt, const float* x_chw, const float* weight, const float* bias, float slope, void* out_s16);
/* op_head_ps: the head, 4x4 stride-2 pad-1 transposed convolution C -> 24 + bias + PixelShuffle(2) into the flow tensor [4 Ht][4 Wt][8] (head_h2_kernel<EPI_DECONV_PS,
 * S16IN>).  s16 = 1: input is a raw S16 tensor of op_s16_geom(C, Ht, Wt); s16 = 0: input is C x Ht x Wt fp32 (read as NHWC, ld = C).  weight [24][C][4][4],
 * bias [24].  out8hw: 8 x 4 Ht x 4 Wt planar; it is uploaded into the device flow tensor before the launch and all 8 planes come back - the kernel writes
 * planes 0 - 5 and must leave 6 and 7 alone. */
int rife_hip_op_head_ps(int gpuid, int C, int Ht, int Wt, int s16, const void* input, const float* weight, const float* bias, float* out8hw);
/* op_tail: the kernels that read the LAST trunk tensor of block 3 and write the quantised frame, one launch of the kernel under test per call.  kernel =
 * RIFE_HIP_TAIL_RS: launch_tail_rs (tail_rs_kernel<0, PX>); RIFE_HIP_TAIL_HEAD_S16: launch_conv with the fused tail and the S16 geometry (head_h2_kernel<EPI_FINAL,
 * true, PX>); RIFE_HIP_TAIL_HEAD_F32: the same on an fp32 tensor (head_h2_kernel<EPI_FINAL, false, PX>); RIFE_HIP_TAIL_UNFUSED: launch_conv with EPI_DECONV_PS into a
 * flow tensor, then k_final / k_final_px<PX>, as a pass launches them when the tail is not fused.  pixfmt: RIFE_HIP_PIX_RGB8, RGB10_U16, A2B10G10R10 or RGBA8.
 * Frame w x h, padded to wp x hp (32n); C = 64 and the trunk is hp / 4 x wp / 4.  trunk: the raw S16 tensor of op_s16_geom(64, hp / 4, wp / 4), for
 * RIFE_HIP_TAIL_HEAD_F32 64 x hp / 4 x wp / 4 fp32 (read as NHWC).  weight [24][64][4][4] (exactly fp16), bias [24]; F [hp][wp][4] and M [hp][wp]: the running flow
 * and mask logit before block 3's update; img0, img1: the resident frames, hp x wp dwords (depth 8: R | G << 8 | B << 16 | A << 24, depth 10: R | G << 10 | B << 20).
 * cus > 0: persistent grids sized for that many compute units during the call (0 = the chip), as in rife_hip_op_trunk.  out: RIFE_HIP_TAIL_GUARD bytes, the frame
 * (w x h pixels of 3, 6, 4 or 4 bytes), RIFE_HIP_TAIL_GUARD bytes; uploaded as given, the launch writes at the frame's offset, the whole buffer comes back.
 * A null argument, a frame of 2^27 padded pixels or more, an unknown kernel or pixfmt, weights that are not fp16, and RIFE_HIP_TAIL_RS where the product would
 * not run that kernel on this head (RIFE_HIP_TAIL_RS=0, RIFE_HIP_T64=0, RIFE_HIP_TRUNK=f32) return -RIFE_HIP_EINVAL before anything is uploaded. */
enum { RIFE_HIP_TAIL_RS = 0, RIFE_HIP_TAIL_HEAD_S16 = 1, RIFE_HIP_TAIL_HEAD_F32 = 2, RIFE_HIP_TAIL_UNFUSED = 3 };
enum { RIFE_HIP_TAIL_GUARD = 256 };
int rife_hip_op_tail(int gpuid, int kernel, int pixfmt, int w, int h, const void* trunk, const float* weight, const float* bias, const float* F, const float* M,
                     const uint32_t* img0, const uint32_t* img1, int cus, void* out);

/* op_tail_motion: rife_hip_op_tail with the motion export (include/rife_hip.h rife_hip_motion_t) - ONE launch of the motion form of the kernel under test
 * (tail_rs_motion_kernel, head_h2_motion_kernel; the unfused pair: the head as before, then k_final_motion<PX>), which writes the frame AND each pixel's final flow and blend weight.  motion_format:
 * RIFE_HIP_MOTION_F32 / _F16.  flow, mask: HOST buffers of RIFE_HIP_TAIL_GUARD bytes, h rows of flow_pitch / mask_pitch bytes, RIFE_HIP_TAIL_GUARD bytes; uploaded as
 * given, the launch writes at the guard's offset, the whole buffers come back (guards and the gaps of padded rows with them).  Either may be null (not wanted); both null,
 * an unknown format and a pitch the product's motion calls refuse are -RIFE_HIP_EINVAL before anything is uploaded.  Everything else as in rife_hip_op_tail. */
int rife_hip_op_tail_motion(int gpuid, int kernel, int pixfmt, int w, int h, const void* trunk, const float* weight, const float* bias, const float* F, const float* M,
                            const uint32_t* img0, const uint32_t* img1, int cus, void* out, int motion_format, void* flow, size_t flow_pitch, void* mask, size_t mask_pitch);

/* op_apply: the apply kernel alone (csrc/apply_motion.h; include/rife_hip.h "apply motion"), ONE launch, on planes and motion in HOST memory: the call uploads every
 * plane and both motion buffers, gaps between rows included, into device allocations with the same pitches and the same pointer alignment modulo 16, so the form
 * the host picks is the one it would pick for the caller's planes, and the output planes come back with every byte the kernel did not write as it went in.
 * force_scalar: 0 = the host's choice, 1 = the one-pixel-per-lane form.  The rules of rife_hip_apply_motion hold (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_apply(int gpuid, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* host_motion, int wp, int hp,
                      const rife_hip_planes_t* out, int force_scalar);
/* op_apply_scaled: the scaled apply kernel alone (csrc/apply_scaled.h; include/rife_hip.h "apply motion at another resolution"), ONE launch of one set on planes and
 * a motion of mw x mh in HOST memory, uploaded as op_apply uploads them (pitches and pointer alignment modulo 16 kept; the output planes come back with every byte
 * the kernel did not write as it went in).  A set of shift 0, 0 is the launch of op_apply.  force_scalar: 0 = the host's choice, 1 = the one-pixel-per-lane form.
 * The rules of the sets calls hold (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_apply_scaled(int gpuid, const rife_hip_apply_set_t* set, const rife_hip_motion_t* host_motion, int mw, int mh, int force_scalar);
/* op_hbd_to_rgb10: the high-bit-depth pre-processing kernel alone (csrc/hbd.h; include/rife_hip.h "high bit depth"), ONE launch on an hbd image of HOST planes, uploaded
 * as op_image_to_resident uploads them (pitches and pointer alignment modulo 16 kept, so the form the host picks is the one it would pick for the caller's planes):
 * out_padded takes the resident form, hp x wp dwords R | G << 10 | B << 20 (hp, wp = h, w rounded up to 32n), padding included.  force_scalar: 0 = the host's choice,
 * 1 = the scalar form.  The rules of rife_hip_hbd_check hold (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_hbd_to_rgb10(int gpuid, const rife_hip_image_t* img, int depth, uint32_t* out_padded, int force_scalar);
/* op_apply_yuv: the apply launches of a subsampled high-bit-depth image alone (csrc/apply_yuv.h), on a luma set (shift 0, 0), a chroma set (shift -1, -1 or -1, 0) and a
 * motion of mw x mh in HOST memory, uploaded as op_apply_scaled uploads them (pitches and pointer alignment modulo 16 kept; the output planes come back with every byte
 * the launch did not write as it went in).  Where the host's rule admits it - u16 samples, at least 4 luma columns, luma output pointers and pitches aligned to 8 bytes
 * and chroma ones to 4, RIFE_HIP_APPLY_YUV not 0 - this is ONE launch of k_apply_yuv and the call returns 1; everywhere else it is the two launches of the sets calls
 * and the call returns 0.  The rules of the sets calls hold (-RIFE_HIP_EINVAL before anything is uploaded), and the two shifts must be as named. */
int rife_hip_op_apply_yuv(int gpuid, const rife_hip_apply_set_t* luma_set, const rife_hip_apply_set_t* chroma_set, const rife_hip_motion_t* host_motion, int mw, int mh);
/* op_packed_to_rgb10: the packed pre-processing kernel alone (csrc/hbd_packed.h; include/rife_hip.h "16-bit packed RGB and RGBA"), ONE launch on a packed image in HOST
 * memory, uploaded as op_apply uploads a plane (pitch and pointer alignment modulo 16 kept, so the form the host picks is the one it would pick for the caller's frame):
 * out_padded takes the resident form, hp x wp dwords R | G << 10 | B << 20 (hp, wp = h, w rounded up to 32n), padding included.  force_scalar: 0 = the host's choice,
 * 1 = the scalar form.  Returns 1 where the vector form ran, 0 for the scalar form.  The rules of rife_hip_packed_check hold (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_packed_to_rgb10(int gpuid, const rife_hip_packed_t* img, uint32_t* out_padded, int force_scalar);
/* op_apply_packed: the packed blend alone (csrc/hbd_packed.h), ONE launch on three packed images and a motion of w x h in HOST memory, uploaded as op_apply uploads them
 * (the output comes back with every byte the kernel did not write as it went in).  force_scalar: 0 = the host's choice, 1 = the one-pixel-per-lane form.  Returns 1 where
 * the vector form ran, 0 for the scalar form.  The rules of the packed calls and of the motion hold (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_apply_packed(int gpuid, const rife_hip_packed_t* p0, const rife_hip_packed_t* p1, const rife_hip_packed_t* out, const rife_hip_motion_t* host_motion,
                             int force_scalar);
/* op_sp_to_rgb10: the semi-planar pre-processing kernel alone (csrc/hbd_semiplanar.h; include/rife_hip.h "semi-planar high bit depth"), ONE launch on a semi-planar
 * image in HOST memory, both planes uploaded as op_apply uploads a plane (pitches and pointer alignment modulo 16 kept, so the form the host picks is the one it would
 * pick for the caller's surface): out_padded takes the resident form, hp x wp dwords R | G << 10 | B << 20 (hp, wp = h, w rounded up to 32n), padding included.
 * force_scalar: 0 = the host's choice, 1 = the scalar form.  Returns 1 where the vector form ran, 0 for the scalar form.  The rules of rife_hip_semiplanar_check hold
 * (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_sp_to_rgb10(int gpuid, const rife_hip_semiplanar_t* img, uint32_t* out_padded, int force_scalar);
/* op_apply_sp: the semi-planar blend alone (csrc/hbd_semiplanar.h), ONE launch on three semi-planar images and a motion of mw x mh = the luma size in HOST memory,
 * uploaded as op_apply uploads them (both output planes come back with every byte the kernel did not write as it went in).  force_scalar: 0 = the host's choice, 1 = the
 * one-chroma-pixel-per-lane form.  Returns 1 where the vector form ran, 0 for the scalar form.  The rules of the semi-planar calls and of the motion hold
 * (-RIFE_HIP_EINVAL before anything is uploaded). */
int rife_hip_op_apply_sp(int gpuid, const rife_hip_semiplanar_t* p0, const rife_hip_semiplanar_t* p1, const rife_hip_semiplanar_t* out, const rife_hip_motion_t* host_motion,
                         int mw, int mh, int force_scalar);

/* ---- the rife-v2.x / v3.x schedule's own kernels alone (csrc/elementwise_v2.h, stem_fused_v2.h, conv_img.h, and the two-tensor / second-destination forms of
 * launch_conv; csrc/engine_v2_ops.h), ONE launch of the kernel under test per call - the launches of run_v2_ifnet / run_v2_flow / run_v2_synth with their grids.
 * Host arrays in device layout go in and out; every OUTPUT buffer is uploaded as given and comes back whole, so a store outside the kernel's domain shows up in the
 * caller's sentinels.  Layers are built by the product's layer upload with the flags rife_hip_load sets for the v2 family and launched by the product's launchers.
 * What the product would not launch is -RIFE_HIP_EINVAL before anything is uploaded.
 * Frames: wp x hp, multiples of 32, below 2^27 pixels.  imgf4 = 0: resident dwords R | G << 8 | B << 16 (ImgU8); imgf4 = 1: float4 per pixel (ImgF4, the half frames of
 * UHD mode: multiples of 16).  acc: the running flow, [hp / 2][wp / 2][4].
 * op_v2_assemble: first != 0: k2_assemble0<S, IMG> (S = 8, 4; acc unused) -> out [hp / S][wp / S][8]; else k2_assemble<S, IMG, FSCALE> (S = 4, 2, 1; fscale: S = 2 only)
 * -> out [hp / S][wp / S][16], pad channels included. */
int rife_hip_op_v2_assemble(int gpuid, int S, int first, int fscale, int imgf4, const void* img0, const void* img1, int wp, int hp, const float* acc, float* out);
/* op_v2_stem: the 10 -> cout (4n <= 96) stride-2 convolution + PReLU on that block input, S = 1, 2.  weight [cout][10][3][3] (exactly fp16), bias, slope [cout];
 * out [hp / 2S][wp / 2S][out_ld].  route = RIFE_HIP_V2_STEM_PRODUCT: stem2_fusable + launch_stem2_fused, the R64 form where the product picks it; _NO_R64: the R64 form
 * off, as RIFE_HIP_V2_STEM_R64=0; _UNFUSED: k2_assemble, then launch_conv on conv_h2s2_kernel, as RIFE_HIP_V2_FUSED_STEM=0. */
enum { RIFE_HIP_V2_STEM_PRODUCT = 0, RIFE_HIP_V2_STEM_NO_R64 = 1, RIFE_HIP_V2_STEM_UNFUSED = 2 };
int rife_hip_op_v2_stem(int gpuid, int route, int S, int fscale, int imgf4, const void* img0, const void* img1, int wp, int hp, const float* acc, const float* weight,
                        const float* bias, const float* slope, int cout, int out_ld, float* out);
/* op_v2_flow_accum: k2_flow_accum<S, FIRST, MUL> for the triples run_v2_ifnet launches - (8, 1, 0), (4, 0, 0), (2, 0, 0), (1, 0, 0) and, rife-v3.x, (4, 1, 1), (2, 0, 1).
 * D [hh / S][wh / S][4]; acc [hh][wh][4] goes in and comes out; wh, hh multiples of 16. */
int rife_hip_op_v2_flow_accum(int gpuid, int S, int first, int mul, const float* D, int wh, int hh, float* acc);
/* op_v2_ctx_warps: the k2_flow_half<true> / <false> chains of both frames, then batch = 0: the four-plus-four k2_warp_nhwc launches, batch = 1: the one k2_warp_nhwc_batch
 * launch, with the out_ld / out_coff table of run_v2_synth.  feat[4 frame + level]: [hp >> (level + 2)][wp >> (level + 2)][32 << level]; fl[4 frame + level]: the flow
 * pyramids, [..][..][2], in and out; cat[level]: the concat buffers B1..B4, [..][..][128 << level], in and out. */
int rife_hip_op_v2_ctx_warps(int gpuid, int batch, const float* acc, int wp, int hp, const float* const* feat, float* const* fl, float* const* cat);
/* op_v2_final: float_form = 0: k2_final, the u8 RGB frame of w x h from the padded inputs (wp, hp = w, h rounded up to 32n); 1: k2_final_float, [hp][wp] float4.
 * head [hp][wp][4] (the sigmoid head's output).  out: RIFE_HIP_TAIL_GUARD bytes, the frame, RIFE_HIP_TAIL_GUARD bytes. */
int rife_hip_op_v2_final(int gpuid, int float_form, const uint32_t* img0, const uint32_t* img1, int w, int h, const float* acc, const float* head, void* out);
/* op_v2_uhd: what = 0: k2_image_half, a resident frame wp x hp -> float4 [hp / 2][wp / 2]; what = 1: k2_flow_up2_double, float4 [hp / 2][wp / 2] -> [hp][wp] (16n). */
int rife_hip_op_v2_uhd(int gpuid, int what, const void* in, int wp, int hp, float* out);
/* op_v2_conv_img: conv_img_s2_kernel, the ContextNet's 3 -> 32 stride-2 convolution + PReLU straight from the resident frame.  two = 0: one frame, gridDim.y = 1; 1: both
 * frames, gridDim.y = 2.  The grid is capped as run_v2_synth caps it (8 / 4 workgroups per CU); cus > 0: that many compute units instead of the chip's.
 * weight [32][3][3][3] (exactly fp16); out0, out1 [hp / 2][wp / 2][32]. */
int rife_hip_op_v2_conv_img(int gpuid, int two, int cus, const uint32_t* img0, const uint32_t* img1, int wp, int hp, const float* weight, const float* bias, const float* slope,
                            float* out0, float* out1);
/* op_conv_pair: launch_conv on a cin (16n) -> cout (4n) layer, 3x3 stride 1 | 2 or (deconv) 4x4 stride-2 transposed, with x1 / y1 non-null: the second tensor pair of the
 * launch; y2 non-null (one tensor, stride 1): the second destination view.  x [H][W][cin]; y0, y1 [Ho][Wo][y_ld] with the layer's channels at y_coff; y2 [Ho][Wo][y2_ld] at
 * y2_coff.  A second destination where run_v2_synth would copy the skip instead (its dual_ok), and either form on a transposed layer: -RIFE_HIP_EINVAL. */
int rife_hip_op_conv_pair(int gpuid, int cin, int cout, int stride, int deconv, int H, int W, const float* weight, const float* bias, const float* slope, const float* x0,
                          const float* x1, float* y0, float* y1, int y_ld, int y_coff, float* y2, int y2_ld, int y2_coff);

/* ---- the generic layer-wise graph executor (csrc/graph_exec.h, graph_run.h, graph_kernels.h: the v1 family) on any .param / .bin pair, one graph_run per call.
 * graph_plan needs no device: it parses <base>.param as rife_hip_graph_check does and writes what the loader settled on, one line per layer, tab-separated:
 *   <layer name> <kind> fold=<the layer that executes this one | -> out=<the blob the launch writes | -> class=<g_conv3x3 | g_conv3x3_s2 | g_conv5x5 | g_deconv4x4 | direct | ->
 *   padded=<1: zero filters pad the output channels to a multiple of 4>
 * into buf (cap bytes, NUL-terminated; too small: -RIFE_HIP_EINVAL).
 * graph_eval loads <base>.param / .bin with the product's loader and runs the product's graph_run once.  Bound blobs: n_in names, planar CHW fp32 host arrays and
 * in_dims[3 i .. 3 i + 2] = c, h, w; each is uploaded into a blob allocated as the executor allocates its own (pixel stride = channels rounded up to 16, pad
 * channels zero; a 1 x 1 x C blob is a vector).  Wanted blobs: n_out names; out_chw[i] takes the blob as planar CHW if it has at most out_caps[i] ELEMENTS, and
 * out_dims[3 i ..] its c, h, w.  keep != 0: the loaded net and its blob storage stay for the next call with the same base and gpuid, which then runs on them (the
 * re-use of blob buffers across geometries); a call with keep = 0 releases them.
 * Refused by name before anything is uploaded or launched, -RIFE_HIP_EINVAL: a wanted blob that no launch writes (the tops of the two BinaryOps folded into an SE
 * tail, the top of a Convolution whose result goes to its PReLU's top), and a binding of such a blob (it would cut a fused pair or an SE tail).  -RIFE_HIP_EMODEL
 * from graph_run: Interp from a blob one pixel wide or high, global Pooling over a channel count that is not a multiple of 4. */
int rife_hip_graph_plan(const char* base, char* buf, size_t cap);
int rife_hip_graph_eval(int gpuid, const char* base, int n_in, const char* const* in_names, const float* const* in_chw, const int* in_dims, int n_out,
                        const char* const* out_names, float* const* out_chw, const size_t* out_caps, int* out_dims, int keep);

/* ---- workspace pool of the host-buffer entry points (csrc/engine_abi.h: lease_ctx / release_ctx): pooled = idle workspaces the engine holds,
 * leased = workspaces in use by callers right now, high_water = the most callers in flight at any of the last 32 leases (the pool is trimmed to it). */
int rife_hip_pool_state(const rife_hip_t* r, int* pooled, int* leased, int* high_water);

#ifdef __cplusplus
}
#endif

#endif  /* RIFE_HIP_TEST_H */
