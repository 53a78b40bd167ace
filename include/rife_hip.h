/* librife_hip — C-ABI of the MI355X-native RIFE engine.
 *
 * This is the drop-in boundary for the reference's hot path `RIFE::load()` / `RIFE::process()`
 * (nihui/rife-ncnn-vulkan src/rife.h:11-52, src/rife.cpp:127-379, 381-1212, 2462-3202): every entry point
 * below replaces one member of that class.  Plain pointers and sizes only; no C++/torch types cross it.
 * The C++ class `RIFE` in rife-ncnn-vulkan_amd/csrc/rife.h (same name, same signatures as the reference)
 * is a thin shim over these calls, and INTEGRATION.md shows the binding a maintainer of the reference adds.
 *
 * Error convention (reference: `int` return, 0 = ok, src/rife.cpp:378,1211,3201): 0 on success, negative
 * on failure; rife_hip_last_error() returns a thread-local message.  Nothing throws across this boundary.
 * There is NO CPU fallback: every compute entry point fails (-RIFE_HIP_ENODEV) when no HIP device exists.
 */
#ifndef RIFE_HIP_H
#define RIFE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIFE_HIP_EINVAL   1   /* bad argument */
#define RIFE_HIP_ENODEV   2   /* no such HIP device / no GPU */
#define RIFE_HIP_EIO      3   /* model file missing or malformed */
#define RIFE_HIP_EMODEL   4   /* graph is not a supported RIFE family */
#define RIFE_HIP_EHIP     5   /* HIP runtime error */
#define RIFE_HIP_ENOSYS   6   /* mode not implemented */

typedef struct rife_hip rife_hip_t;

/* ncnn::get_gpu_count() as used by the reference CLI (src/main.cpp:792-802). */
int rife_hip_device_count(void);

/* RIFE::RIFE(gpuid, tta_mode, tta_temporal_mode, uhd_mode, num_threads, rife_v2, rife_v4)  src/rife.cpp:27-47.
 * gpuid = HIP device ordinal (the reference's -1 = CPU device is not served by this library). */
rife_hip_t* rife_hip_create(int gpuid, int tta_mode, int tta_temporal_mode, int uhd_mode, int num_threads,
                            int rife_v2, int rife_v4);

/* RIFE::~RIFE()  src/rife.cpp:49-78 */
void rife_hip_destroy(rife_hip_t* r);

/* RIFE::load(modeldir)  src/rife.cpp:127-379 — reads <modeldir>/flownet.{param,bin} (+ contextnet, fusionnet
 * unless rife_v4), validates the topology against the compiled-in schedules, packs and uploads the weights. */
int rife_hip_load(rife_hip_t* r, const char* modeldir);

/* RIFE::process(in0image, in1image, timestep, outimage)  src/rife.cpp:381-1212 / 2462-3202.
 * Host buffers: tightly packed u8 HWC RGB, w*h*3 bytes each (the ncnn::Mat the CLI builds, src/main.cpp:187,332).
 * Re-entrant on a const object from several host threads (src/main.cpp:860-863). */
int rife_hip_process(const rife_hip_t* r, const uint8_t* in0_rgb, const uint8_t* in1_rgb, int w, int h,
                     float timestep, uint8_t* out_rgb);

/* Optional throughput entry point: n independent pairs from host memory in one call, spread over internal
 * streams so that the copies of one pair overlap the kernels of the others - what the reference gets from its proc threads
 * (src/main.cpp:849-866).  Same pixels as n rife_hip_process() calls; timestep 0 / 1 entries are copies.  A host frame that
 * appears in several pairs of the batch (in0[i + 1] == in1[i] in a sequence) is uploaded once. */
int rife_hip_process_batch(const rife_hip_t* r, int n, const uint8_t* const* in0_rgb, const uint8_t* const* in1_rgb, const float* timestep,
                           uint8_t* const* out_rgb, int w, int h);

/* Same, with all three frames already resident in device memory (what ncnn's VkMat path does internally between
 * record_clone and submit, src/rife.cpp:2522-2530,3176-3186).  Work is enqueued on `hip_stream` (a hipStream_t;
 * NULL = the engine's own stream) and the call returns without synchronising when a stream is given. */
int rife_hip_process_device(const rife_hip_t* r, const void* d_in0_rgb, const void* d_in1_rgb, int w, int h,
                            float timestep, void* d_out_rgb, void* hip_stream);

/* Streams that own a PART of the chip.  The reference keeps a GPU busy with several proc threads per device (-j, src/main.cpp:849-866), whose
 * command buffers share the whole device.  On MI355X (256 compute units in 8 XCDs, an L2 per XCD) the pairs in flight interfere less when each has
 * compute units of its own: rife_hip_stream_create returns a hipStream_t restricted to the compute units i with i % nparts == part
 * (hipExtStreamCreateWithCUMask), and rife_hip_process_device on such a stream sizes its persistent kernels for that part.  Frames are the same
 * bytes on every stream.  nparts = 1: an ordinary stream.  Measured (1920x1080, resident frames): 4 parts x 1 caller each 1,690 frames/s against
 * 1,450 - 1,590 from 3 ordinary streams; 3840x2160: 2 parts x 2 callers each 473 - 479 against 465 - 469.  Destroy with rife_hip_stream_destroy (after the work on it has finished), or
 * let rife_hip_destroy do it.
 * Synchronisation semantics: hipExtStreamCreateWithCUMask takes no flags, so a stream with nparts > 1 is a BLOCKING stream - it synchronises implicitly
 * with the legacy NULL stream (work enqueued on stream 0, plain hipMemcpy / hipMemset), while nparts = 1 returns a hipStreamNonBlocking stream.  Keep
 * NULL-stream work out of the process while partition streams carry pairs, or the "independent" parts serialise behind it; the engine itself never
 * enqueues on the NULL stream. */
int rife_hip_stream_create(const rife_hip_t* r, int part, int nparts, void** hip_stream);
int rife_hip_stream_destroy(const rife_hip_t* r, void* hip_stream);

/* n resident pairs in one call (SURVEY.md §8f-2 "batch >= 2 pairs per launch for the coarse blocks"): the pairs run two by two in lockstep on
 * internal streams, the trunk layers of the coarse IFBlocks as ONE launch per layer for both pairs of a group (models/rife-v4.6/flownet.param:14-42,
 * 66-94), forked from and joined into `hip_stream` with events: like rife_hip_process_device the call returns without synchronising when a
 * stream is given, and work enqueued on `hip_stream` afterwards sees all n results.  NULL synchronises before returning.  Same bytes as n
 * rife_hip_process_device calls; model families without the lockstep schedule (and -x / -z) run the pairs one after the other. */
int rife_hip_process_device_batch(const rife_hip_t* r, int n, const void* const* d_in0_rgb, const void* const* d_in1_rgb, const float* timestep,
                                  void* const* d_out_rgb, int w, int h, void* hip_stream);

/* Stream mode (absent in the reference, whose tasks upload both frames every time, src/main.cpp:315-334,
 * src/rife.cpp:2490-2530): in a frame sequence every frame is the second frame of one pair and the first frame of the next,
 * and with -n > 2N it serves several timesteps, so a caller can upload a frame ONCE and interpolate between resident frames.
 * A frame belongs to the device of the engine that uploaded it and may be used by any thread and by several calls at once
 * (it is read-only); release it after the last call that uses it has returned.  Pixels are identical to rife_hip_process(). */
typedef struct rife_hip_frame rife_hip_frame_t;
int rife_hip_frame_upload(const rife_hip_t* r, const uint8_t* rgb, int w, int h, rife_hip_frame_t** frame);
int rife_hip_process_frames(const rife_hip_t* r, const rife_hip_frame_t* frame0, const rife_hip_frame_t* frame1, float timestep,
                            uint8_t* out_rgb);
void rife_hip_frame_release(rife_hip_frame_t* frame);

/* ---- deep colour: 10-bit RGB in and out (absent in the reference, whose frames are 8-bit, src/main.cpp:187) ------------------------------
 * The network's inputs are fp32 planes in [0, 1] (src/rife.cpp:4167), so nothing but the pre-processing, the frame taps and the quantising
 * epilogues knows the depth.  Resident frames stay one dword per pixel (10:10:10 instead of 8:8:8:x): a 10-bit pair moves the bytes an 8-bit pair moves.
 *   input plane  = code * (1 / 1023.f), zero-padded to 32n like the 8-bit plane;
 *   output code  = min(max((int)(v * 1023.f + 0.5f), 0), 1023), cropped with the padded pitch;
 *   timestep 0 / 1 return the first / second frame's codes (clamped to 1023, alpha bits 3).
 * Input and output of a call have the same format, and the two 10-bit formats give the same codes.  With RIFE_HIP_PIX_RGB8 every _px call IS the
 * call without the suffix (same code path, same bytes, every model family and mode).
 * Scope of the 10-bit formats: model family rife-v4.6, plain mode, every frame size the 8-bit path serves.  Any other family (rife-v4, v2.x, v3.x, v1) or mode
 * (TTA -x, temporal TTA -z, UHD -u) returns -RIFE_HIP_ENOSYS with a message that names it and leaves the output untouched; the opt-in graph replay
 * (RIFE_HIP_GRAPH=1) does not apply to 10-bit calls.  Out of scope: rife_hip_process_batch (the host batch with internal workers) at depth 10, 12- and
 * 16-bit samples (a second dword per pixel, i.e. different gather kernels), YUV. */
#define RIFE_HIP_PIX_RGB8         0   /* u8 HWC, 3 B / pixel: what rife_hip_process() takes */
#define RIFE_HIP_PIX_RGB10_U16    1   /* u16 HWC, native byte order, 6 B / pixel, codes 0..1023; a larger value is read as 1023 */
#define RIFE_HIP_PIX_A2B10G10R10  2   /* one little-endian dword / pixel: R bits 0-9, G 10-19, B 20-29; bits 30-31 ignored on input, written as 3 */
/* 3 is reserved (an unknown format today). */
#define RIFE_HIP_PIX_RGBA8        4   /* u8 HWC, 4 B / pixel, R G B A: alpha carried through, see below */
/* ---- alpha: RGBA frames in and out (absent in the reference, whose readers drop alpha) --------------------------------------------------------------
 * Served where the 10-bit formats are served, through the same _px calls: model family rife-v4.6, plain mode, every frame size the RGB8 path serves;
 * any other family or mode returns -RIFE_HIP_ENOSYS with a message that names it and leaves the output untouched; the opt-in graph replay does not apply.
 *   colour  the R, G, B bytes of an RGBA call are BYTE FOR BYTE those of the RGB8 call on the same R, G, B.  Alpha never reaches the network: flows
 *           and mask are estimated from the colour alone.
 *   alpha   a fourth plane through the tail of the graph and nothing else: A = code * (1 / 255.f);
 *           a = warp(A0, F.xy) * m + warp(A1, F.zw) * (1 - m), with the arithmetic of the colour channels (the reference's Warp, same operation order,
 *           no contraction) and the same m = sigmoid(M);  code = min(max((int)(a * 255.f + 0.5f), 0), 255).
 *           It is warped by the flow that was estimated from the colour it belongs to, so matte and colour cannot drift apart.
 *   padding colour is zero-padded to 32n as the reference pads it; alpha is padded by EDGE REPLICATION (a pad pixel holds the alpha of the nearest frame
 *           pixel): flows of a few pixels reach into the padding, and zero-padded alpha would turn an opaque frame transparent along its right and
 *           bottom edge.  Opaque in gives 255 everywhere, clear in gives 0 everywhere.
 *   timestep 0 / 1 return the first / second frame's four bytes unchanged.
 *   Straight or premultiplied alpha: the four planes are interpolated as given (premultiplied input avoids fringes of whatever colour hides under
 *   transparent pixels).
 * Out of scope: alpha at depth 10 (A2B10G10R10 has two alpha bits), other families and modes, rife_hip_process_batch (the host batch). */

/* ---- video: 4:2:0 Y'CbCr frames in and out (absent in the reference, whose frames are RGB stills) ---------------------------------------------------------
 * What decoders, `ffmpeg -f yuv4mpegpipe`, VapourSynth / AviSynth clips and hardware surfaces deliver: 1.5 bytes per pixel (3 at 10 bits) instead of 3 (6).
 * cw = (w + 1) / 2, ch = (h + 1) / 2; planes tightly packed, one after the other; odd sizes are served.
 * 5 .. 15 are reserved (unknown formats today, like 3): the 4:2:0 formats are 16 + 2 * (10 bits) + (planar). */
#define RIFE_HIP_PIX_NV12         16  /* u8: Y plane w*h, then one plane of interleaved Cb, Cr pairs, cw*ch*2 */
#define RIFE_HIP_PIX_I420         17  /* u8: planes Y w*h, Cb cw*ch, Cr cw*ch (what Y4M C420* holds) */
#define RIFE_HIP_PIX_P010         18  /* u16 little-endian, the code in the HIGH 10 bits, NV12 plane layout; low bits ignored on input, written as zero */
#define RIFE_HIP_PIX_I420P10      19  /* u16 little-endian, the code in the LOW 10 bits, I420 plane layout (what Y4M C420p10 holds); a larger value is read as 1023 */
/* 4:2:2 and 4:4:4 (mezzanine and camera material; screen capture, animation masters, chains that upsampled chroma): 16 * class + 2 * (10 bits) + (planar), class 1 =
 * 4:2:0 above, 2 = 4:2:2, 3 = 4:4:4.  Planar only: 32, 34, 48, 50 (the semi-planar slots NV16 / P210 / NV24 / P410) are unknown formats, as are 20 .. 31 and 52 .. 64 (class 4 is planar RGB, below).
 * Chroma planes have h rows (not ch); YV16 / YV24: swap plane[1] and plane[2] of an image. */
#define RIFE_HIP_PIX_I422         33  /* u8: planes Y w*h, Cb cw*h, Cr cw*h (what Y4M C422 holds) */
#define RIFE_HIP_PIX_I422P10      35  /* u16 little-endian, the code in the LOW 10 bits, I422 plane layout; a larger value is read as 1023 */
#define RIFE_HIP_PIX_I444         49  /* u8: planes Y, Cb, Cr, each w*h */
#define RIFE_HIP_PIX_I444P10      51  /* u16 little-endian, the code in the LOW 10 bits, I444 plane layout; a larger value is read as 1023 */
/* The colour description is OR-ed into pixfmt (YUV formats only; on an RGB format any of these bits is -RIFE_HIP_EINVAL):
 * bits 8-11 the matrix (an unknown one: -RIFE_HIP_EINVAL), bit 12 the range (limited is the default). */
#define RIFE_HIP_CSP_BT709        (0 << 8)   /* the default */
#define RIFE_HIP_CSP_BT601        (1 << 8)
#define RIFE_HIP_CSP_BT2020NCL    (2 << 8)
#define RIFE_HIP_CSP_FULL         (1 << 12)  /* full range ("JPEG" levels); 8-bit formats only: with a 10-bit format -RIFE_HIP_EINVAL (its round trip below is not exact) */
/* A YUV call is, byte for byte, the A2B10G10R10 call on the converted frames, converted back:
 *     out = rgb10_to_yuv(process_px(yuv_to_rgb10(in0), yuv_to_rgb10(in1), timestep, A2B10G10R10))
 * with INTEGER conversions (tests/yuv_ref.py and, for 4:2:2 / 4:4:4, tests/chroma_ref.py state them in numpy, csrc/yuv.h in HIP; they agree bit for bit):
 *   coefficients  the matrix's real coefficients times 1023 / range (in) or range / 1023 (out), rounded to Q16; range = 219 s luma, 224 s chroma (limited),
 *                 255 both (full); s = 1 at 8 bits, 4 at 10.  Products are summed in integers, + 0x8000, arithmetic shift right by 16.
 *   in            subtract the offsets (16 s and 128 s; full range 0 and 128 s), apply the matrix, clamp to 0..1023.  The chroma of a pixel is the sample of
 *                 its 2x2 block (replication).  The padding to 32n is zero RGB, as everywhere.
 *   out           Y per pixel; Cb, Cr from the SUM of the RGB codes of the block's pixels inside the frame (n = 4, 2 or 1), shifted by 16 + log2 n with the
 *                 rounding constant scaled alike; add the offsets, clamp to 0..255 / 0..1023.
 *   4:2:2, 4:4:4  coefficients, offsets, clamps and colour bits are the same; only the block changes.  4:2:2: the chroma of a pixel is the sample of its 2x1 block, and
 *                 Cb, Cr come from the sum over the block's pixels inside the frame (n = 2, or 1 in the last column of an odd width).  4:4:4: every pixel has its
 *                 own chroma and n = 1 everywhere.
 * YUV -> 10-bit RGB -> YUV is the identity on every sample whose RGB did not clamp, at both depths (half a code of RGB error weighs less than half a code of
 * any output), which is why 8- AND 10-bit video ride the engine's depth-10 path unchanged, and a difference of one RGB code moves no Y, Cb, Cr by more than
 * one code, which carries the engine's 1-code contract across.
 * Chroma siting: replication up and the box average down are each other's inverse on block-constant chroma and have no net shift whatever the stream's
 * siting is; chroma siting tags (Y4M C420jpeg / C420mpeg2 / C420paldv) are ignored.
 * timestep 0 / 1 return the first / second frame's samples (P010: low bits cleared; I420P10, I422P10, I444P10: clamped to 1023).  Input and output of a call share one format and
 * one colour description; rife_hip_process_frames refuses two frames that differ in either.
 * Scope: that of the 10-bit formats - model family rife-v4.6, plain mode, every frame size; any other family or mode returns -RIFE_HIP_ENOSYS with a message
 * that names it, before anything is written; the opt-in graph replay does not apply.  Out of scope: rife_hip_process_batch (the host batch), semi-planar
 * 4:2:2 / 4:4:4, 12-bit samples, alpha planes, interlaced chroma. */

/* ---- planar RGB: three planes R, G, B of w x h samples each (absent in the reference, whose frames are packed 8-bit RGB) ----------------------------------------------
 * What the RIFE filters of VapourSynth / AviSynth hold (RGB24, RGB30, RGBH, RGBS) and what ffmpeg calls gbrp / gbrp10le / gbrpf32le.  Class 4 of the numbering
 * 16 * class + 2 * k + (planar), k = 0 u8, 1 u16, 2 half, 3 float; 64, 66, 68, 70 (the packed slots) and 72 up are unknown formats.  A tight frame is the three planes
 * glued one after the other, R first; an image names them in plane[0..2] with a byte pitch each.  ffmpeg's G, B, R order needs no format of its own: the caller
 * permutes plane[] (the three planes are treated alike), as for YV12.  A colour description OR-ed onto these formats is -RIFE_HIP_EINVAL, as on every RGB format. */
#define RIFE_HIP_PIX_RGBP8        65  /* u8 */
#define RIFE_HIP_PIX_RGBP10       67  /* u16 little-endian, the code in the LOW ten bits; a larger value is read as 1023 (as I444P10) */
#define RIFE_HIP_PIX_RGBPH        69  /* IEEE binary16, nominal range [0, 1] */
#define RIFE_HIP_PIX_RGBPF        71  /* IEEE binary32, nominal range [0, 1] */
/* A planar RGB call is, byte for byte, the A2B10G10R10 call on the converted frames, converted back:
 *     out = from10(process_px(to10(in0), to10(in1), timestep, A2B10G10R10))
 * with the conversions fixed to the bit (tests/planar_ref.py states them in numpy, csrc/planar_rgb.h in HIP):
 *   to10    u8: (v << 2) | (v >> 6) (what `rife-hip -b 10` does to an 8-bit file);  u16: min(v, 1023);
 *           half and float, on the value x widened to fp32: (int)(fminf(fmaxf(x, 0.f), 1.f) * 1023.f + 0.5f), the product and the sum rounded separately (no fused
 *           multiply-add).  NaN and negative values read as 0, +inf and values above 1 as 1023.
 *   from10  u8: c >> 2;  u16: c;  float: (float)c / 1023.f, a correctly rounded division (not a product with a reciprocal: the two differ in 24 of the 1024 codes);
 *           half: that float rounded to nearest even.
 * to10(from10(c)) == c for every code in all four formats and u8 -> 10 -> u8 is the identity, so the engine's 1-code contract carries across unchanged (RGBP8: at
 * most one code at depth 8, since one 10-bit code moves c >> 2 by at most one); an 8-bit value carried as the float v / 255.f comes back as a float that rounds to v.
 * The padding to 32n (64n at flow scale 2) is zero RGB, as everywhere.  timestep 0 / 1 return the first / second frame's CANONICAL samples from10(to10(v)): a float
 * frame comes back quantised and NaN comes back as 0.
 * Depth limit: the resident frame holds ten bits per channel, and that is the precision of the half and float formats - a float frame is quantised to 1024 levels on
 * the way in and the result is one of 1024 values.  Storing the un-quantised blend for float output is out of scope.
 * Scope: that of the YUV formats - model family rife-v4.6, plain mode, both flow scales, every frame size, every _px call, rife_hip_process_frames and the image calls;
 * any other family or mode returns -RIFE_HIP_ENOSYS with a message that names it, before anything is written; the opt-in graph replay does not apply.  Out of scope:
 * rife_hip_process_batch (the host batch), packed float RGB, planar RGBA / alpha planes, 12- and 16-bit integer planes. */

size_t rife_hip_frame_bytes(int w, int h, int pixfmt);      /* 0 for an unknown format or w, h <= 0; YUV: (w*h + 2*cw*ch) samples (4:2:2: ch = h; 4:4:4: cw = w, ch = h); planar RGB: 3 * w * h samples; colour bits are ignored */
int rife_hip_process_px(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt);
int rife_hip_process_device_px(const rife_hip_t* r, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt,
                               void* hip_stream);
int rife_hip_process_device_batch_px(const rife_hip_t* r, int n, const void* const* d_in0, const void* const* d_in1, const float* timestep,
                                     void* const* d_out, int w, int h, int pixfmt, void* hip_stream);
/* A frame carries its format: rife_hip_process_frames writes the format its two frames were uploaded in (-RIFE_HIP_EINVAL if they differ), and its
 * out_rgb then points at rife_hip_frame_bytes() bytes. */
int rife_hip_frame_upload_px(const rife_hip_t* r, const void* pixels, int w, int h, int pixfmt, rife_hip_frame_t** frame);

/* ---- strides and planes: frames as video producers hand them over --------------------------------------------------------------------------------------
 * The _px calls take a tightly packed frame with its planes glued one after the other.  An AVFrame has data[] and linesize[], a VapourSynth / AviSynth frame one
 * allocation per plane with padded rows, a decoder surface is pitched NV12 / P010 in device memory, a crop or tile is a window with its parent's pitch: an image
 * descriptor names each plane and the BYTES from one of its rows to the next, and the image calls read and write those planes in place. */
typedef struct rife_hip_image {
    int w, h, pixfmt;        /* pixfmt as for the _px calls, colour bits included */
    void* plane[3];          /* RGB8 / RGB10_U16 / A2B10G10R10 / RGBA8: plane[0];  NV12 / P010: Y, CbCr;  I420 / I422 / I444 and their P10 forms: Y, Cb, Cr;  RGBP8 / RGBP10 / RGBPH / RGBPF: R, G, B */
    ptrdiff_t pitch[3];      /* BYTES from one row of the plane to the next */
} rife_hip_image_t;
/* Entries of plane[] and pitch[] that the format does not use are ignored.  YV12 and its 10-bit form need no format of their own: the caller swaps plane[1] and
 * plane[2] of an I420 / I420P10 image.
 * Rules (the check function below states them, and every image call repeats them before it touches anything; a violation is -RIFE_HIP_EINVAL with a message):
 *   w, h > 0 and pixfmt is one the _px calls accept; every plane the format has is non-NULL; each pitch is positive, at least the plane's row bytes, at most
 *   INT32_MAX and a multiple of the plane's element size (1 for the u8 formats, 2 for the u16 and half formats, 4 for A2B10G10R10 and float planes); each plane pointer is aligned to that
 *   element size.  A negative pitch (bottom-up rows) is refused.  The three images of one call agree in w, h and pixfmt.
 *   Output planes must not overlap each other or the inputs (documented, not checked).
 * Contract: an image call is, byte for byte, the _px call on the same samples repacked tight, with the result unpacked into `out`.  It writes only the first
 * row-bytes bytes of each of the h (4:2:0 chroma: ch) rows of each output plane; the gap between rows and everything around the window keep their bytes.  Timestep
 * 0 / 1 return the first / second frame's canonical samples (see the formats above) into the strided output.
 * Device planes are read and written by the pre- and post-processing kernels directly (no staging copy); host planes are copied row by row (2-D copies) into and
 * out of the staging buffers of the tight path, which then runs unchanged.
 * Scope: that of the _px formats - model family rife-v4.6, plain mode, every format and size served there; any other family or mode returns -RIFE_HIP_ENOSYS
 * with a message that names it, before anything is written.  Exception: an RGB8 image that is tight (pitch[0] == 3 * w) IS the call without the suffix and is
 * served wherever that is.  The opt-in graph replay does not apply.  Out of scope: a batch call on images, NV21, negative pitches. */
int rife_hip_image_check(const rife_hip_image_t* img);                   /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
size_t rife_hip_image_row_bytes(int w, int pixfmt, int plane);            /* host only: bytes of one row of that plane; 0 for a plane the format does not have */
/* planes in host memory */
int rife_hip_process_image(const rife_hip_t* r, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out);
/* planes in device memory; stream semantics as for the device _px call (NULL = the engine's own stream, synchronised before returning) */
int rife_hip_process_device_image(const rife_hip_t* r, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out,
                                  void* hip_stream);
/* stream mode: upload host planes once (the resident frame is tight, in the image's format), write a result into strided host planes */
int rife_hip_frame_upload_image(const rife_hip_t* r, const rife_hip_image_t* img, rife_hip_frame_t** frame);
int rife_hip_process_frames_image(const rife_hip_t* r, const rife_hip_frame_t* frame0, const rife_hip_frame_t* frame1, float timestep, const rife_hip_image_t* out);

/* ---- UHD / flow scale: flow estimation at half resolution (upstream RIFE's scale=0.5; absent in the reference, whose process_v4 ignores uhd_mode) ----------
 * Motion in 4K material is large in pixels; with every IFBlock at half its usual resolution the coarse pyramid reaches twice as far and the network does a quarter
 * of its arithmetic, while the frames are still warped and blended at full resolution.  divisor 1 (the default) is the reference's graph; divisor 2 is that graph
 * with the block scales 8, 4, 2, 1 doubled to 16, 8, 4, 2 (line numbers of models/rife-v4.6/flownet.param):
 *   blocks 0..2  every Interp factor below 1 is halved and every factor above 1 doubled; the scalar of the BinaryOp mul / div next to an Interp (:50, :53, :108)
 *                and the second coefficient of the two Eltwise sums (:102, :155) are doubled;
 *   block 3      gets the resize layers the other blocks have: Interp(0.5) on its 8-channel concat (:164), Interp(0.5) then / 2 on the flow concatenated to it
 *                (:165), Interp(2) on flow3, and F = F * 1 + u[0:4] * 2, M = M + u[4] in place of the plain adds (:204, :207); the rest of the tail is unchanged
 *                (sigmoid, two warps of the full-resolution frames, blend, quantise);
 *   padding      frames are zero-padded to a multiple of 64 (block 0's trunk runs at 1/64) and the output is cropped with the padded pitch; timestep 0 / 1
 *                return the input frames as at divisor 1.
 * tests/flowscale_ref.py states the rewrite on the .param text; a scale-2 frame is within one code per channel of the oracle running that graph.
 * Every entry point, _px format and image call that plain rife-v4.6 serves is served at divisor 2 with the same bytes as the single call; the batch calls run the
 * pair schedule once per pair (no lockstep groups), and the opt-in graph replay does not apply.  uhd_mode keeps doing nothing for rife-v4.x.
 * rife_hip_set_flow_scale returns 0 or, leaving the engine unchanged, with a last-error message:
 *   -RIFE_HIP_EINVAL  before rife_hip_load (the family is not known yet); divisor <= 0 or not a power of two; while a call on the engine is in flight;
 *   -RIFE_HIP_ENOSYS  divisor 2 on any family other than rife-v4.6 or on an engine created with tta_mode / tta_temporal_mode (the message names the family or
 *                     mode); divisor 4 and above (upstream's 0.25).
 * divisor 1 always succeeds after load.  Call it while no call on the engine is in flight: it drops the engine's workspaces.
 * Out of scope: divisor 4 (padding to 128), the other model families, -x / -z, lockstep groups and graph replay at divisor 2, any change to what uhd_mode does. */
int rife_hip_set_flow_scale(rife_hip_t* r, int divisor);
int rife_hip_flow_scale(const rife_hip_t* r);               /* the divisor in force (1 before load and for a null engine) */

/* ---- precision: one f16 product per weight tap in the residual trunks (the reference's Vulkan path runs fp16 storage and arithmetic; this engine's default is
 * fp32-equivalent) ----
 * The residual trunk layers x <- leaky(conv3x3(x) + b + x) run on tensors stored as a pair {hi = f16(x), lo = f16(x - hi)}.  RIFE_HIP_PRECISION_FULL (the default)
 * multiplies every weight with hi and with lo: two matrix instructions per tap, an fp32-equivalent result.  RIFE_HIP_PRECISION_FAST computes
 *     acc = sum over the 3 x 3 taps of W . hi(x)  +  I . (hi(x) + lo(x))        (fp32 accumulation)
 * i.e. the convolution sees its input rounded to f16 (round to nearest even), while the skip connection adds the unrounded input, so the residual stream stays
 * fp32-equivalent from layer to layer; then the unchanged epilogue: bias, LeakyReLU, and the split of the fp32 result into {hi, lo}, both stored as in full
 * precision.  Tensor layout, zero borders and kernel selection are those of full precision: the same kernel serves a layer in both modes.
 * Reach: all eight trunk layers of every IFBlock that runs on these tensors at the given frame size - at the usual sizes all four blocks.  A block that leaves that
 * path runs at full precision, unchanged: block 0 where its row-kernel grid exceeds 5/8 of a workgroup per compute unit (about 160 workgroups on an MI355X: 4K
 * frames), any trunk tensor of 4 GB and more, and (test build) RIFE_HIP_T64=0.  Stems, heads and everything outside the trunks are full precision always.
 * Within a mode the bytes are identical across entry points (host, device, stream mode, batch calls and their lockstep groups, CU-masked streams, every _px format
 * and image call, flow scale 2) and from run to run.  Accuracy of FAST against the reference's network is measured, not bounded by contract: see README
 * ("Precision"); FULL keeps its bound of one code per channel.
 * rife_hip_set_precision returns 0 or, leaving the engine unchanged, with a last-error message:
 *   -RIFE_HIP_EINVAL  before rife_hip_load (the family is not known yet); a value that is neither constant; while a call on the engine is in flight;
 *   -RIFE_HIP_ENOSYS  FAST on any family other than rife-v4.6 or on an engine created with tta_mode / tta_temporal_mode (the message names the family or mode).
 * FULL always succeeds after load.  Call it while no call on the engine is in flight: it drops the engine's workspaces and any captured graph.  It composes with
 * rife_hip_set_flow_scale in either order. */
enum { RIFE_HIP_PRECISION_FULL = 0, RIFE_HIP_PRECISION_FAST = 1 };
int rife_hip_set_precision(rife_hip_t* r, int precision);
int rife_hip_precision(const rife_hip_t* r);                /* FULL before load and for a null engine */

/* ---- motion export: the final flows and the blend mask, with the frame (absent in the reference, whose flow and mask blobs never leave the Extractor) ----------------
 * Every synthesised pixel has a displacement into frame 0, one into frame 1 and a blend weight; the kernels that finish the frame hold them in registers and a motion
 * call stores them next to the frame: an occlusion / confidence map, motion vectors for an encoder, a motion-blur pass or a temporal denoiser, cut detection without
 * a second optical-flow pass.  What to do with them is the caller's policy.
 *   flow   the graph's final flow tensor, the blob that feeds the last two rife.Warp layers (`327` of the stock models/rife-v4.6/flownet.param: F + flow3[0:4]): the
 *          output pixel (x, y) was sampled from frame 0 at (x + dx0, y + dy0) and from frame 1 at (x + dx1, y + dy1), in pixels of the full-resolution frame, as
 *          rife.Warp reads them (src/warp.cpp:96-168).  h rows of w pixels of 4 samples dx0, dy0, dx1, dy1.
 *   mask   the Sigmoid output (blob `332`): the weight of frame 0's warp; frame 1's is 1 - mask.  h rows of w samples.
 * Both are cropped to w x h and are THE values the frame of the same call was finished from, not a recomputation; at flow scale 2 they are the flow and sigmoid(mask
 * logit) after block 3's update at full resolution.  RIFE_HIP_MOTION_F16 is the F32 sample rounded to nearest even.  The frame of a motion call is byte for byte the
 * frame of the call without it (the same kernel code on the same grids, plus the stores), in every _px format: the motion does not depend on the frame format.
 * flow or mask may be NULL ("not wanted"); both NULL is -RIFE_HIP_EINVAL.  At timestep 0 / 1 the engine returns a copy of a frame without running the network; the
 * motion of such a call is defined as flow 0 and mask 1 - timestep.
 * Rules (rife_hip_motion_check states them, every motion call repeats them before it touches anything; a violation is -RIFE_HIP_EINVAL with the fault named in the
 * message): a known format; each pitch at least the row bytes; flow and its pitch aligned to the pixel (16 bytes for F32, 8 for F16), mask and its pitch to its element
 * (4 / 2); h * pitch < 2^32.  Rows may be padded: the bytes between the rows and around the buffers are not written.
 * Scope: model family rife-v4.6, plain mode, flow scale 1 and 2, precision full and fast, every _px format and frame size.  Any other family (rife-v4 4.0 included) or
 * mode (-x, -z, -u) returns -RIFE_HIP_ENOSYS with a message that names it and the words "motion export", and leaves every output untouched.  The opt-in graph replay
 * does not apply to motion calls.  Out of scope: the batch calls, image (strided-frame) calls with motion, lower-resolution or block motion, the command line (no file
 * format it writes holds this data). */
#define RIFE_HIP_MOTION_F32 0   /* IEEE binary32 samples */
#define RIFE_HIP_MOTION_F16 1   /* IEEE binary16: the F32 sample rounded to nearest-even */
typedef struct rife_hip_motion {
    void*  flow;  size_t flow_pitch;   /* h rows of w pixels x 4 samples: dx0, dy0, dx1, dy1; pitch in BYTES */
    void*  mask;  size_t mask_pitch;   /* h rows of w samples */
    int    format;
} rife_hip_motion_t;
int rife_hip_motion_check(const rife_hip_motion_t* m, int w, int h);          /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
/* host frames and host motion buffers: the motion is downloaded into the caller's pitched buffers from a tight device buffer the workspace allocates at its first
 * motion call (a process that never asks pays no memory) */
int rife_hip_process_motion(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt,
                            const rife_hip_motion_t* host_motion);
/* device frames and device motion buffers, written in place by the kernel that finishes the frame; stream semantics as for the device _px call (NULL = the engine's
 * own stream, synchronised before returning) */
int rife_hip_process_device_motion(const rife_hip_t* r, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt,
                                   const rife_hip_motion_t* device_motion, void* hip_stream);
/* stream mode: resident frames, the result and its motion into host memory */
int rife_hip_process_frames_motion(const rife_hip_t* r, const rife_hip_frame_t* frame0, const rife_hip_frame_t* frame1, float timestep, void* out,
                                   const rife_hip_motion_t* host_motion);

/* ---- apply motion: the exported motion applied to the caller's own planes - 16-bit, float, alpha, auxiliary data (absent in the reference) ----------------------------
 * rife-v4.6 has no refinement network: its frame IS warp(in0, flow[0:2]) * mask + warp(in1, flow[2:4]) * (1 - mask).  The network needs ten bits to ESTIMATE motion;
 * the BLEND of the caller's samples runs here at fp32 on planes of u8, u16, half or float samples: 12- and 16-bit and un-quantised float pictures, alpha at any depth,
 * mattes, depth, ids, a grain layer, the raw frame when motion was estimated on a denoised proxy - anything that must move with the picture without influencing the
 * flow.  The resident frame format and every existing call are untouched.
 * Inputs: two plane sets of w x h, n planes each (1..4), one sample type; a motion field of the same w x h (F32 or F16, flow AND mask); an extent wp >= w, hp >= h
 * (0, 0 = w, h); for integer samples a maxval (u8: 1..255, u16: 1..65535; float samples: 0).  Per output pixel (x, y) and plane k, all in fp32, in this order,
 * products and sums rounded separately (no fused multiply-add):
 *     S(p, xi, yi)  = (xi < w && yi < h) ? (float)p[yi][xi] : 0.f                  virtual zero padding up to the extent
 *     W(p, dx, dy):   sx = x + dx; sy = y + dy; x0 = floor(sx); y0 = floor(sy); x1 = x0 + 1; y1 = y0 + 1;
 *                     x0, x1 clamped to [0, wp-1];  y0, y1 clamped to [0, hp-1];  alpha = sx - x0; beta = sy - y0;      clamp, THEN alpha: src/warp.cpp:133-154
 *                     (S(x0,y0)*(1-alpha) + S(x1,y0)*alpha)*(1-beta) + (S(x0,y1)*(1-alpha) + S(x1,y1)*alpha)*beta
 *     v = W(p0[k], dx0, dy0) * m + W(p1[k], dx1, dy1) * (1 - m)
 *     integer out: min(max((int)(v + 0.5f), 0), maxval)      float out: v      half out: v rounded to nearest even
 * F16 motion samples are widened to fp32 first.  Integer inputs are read as stored; only the output is clamped to maxval.  A NaN or Inf sample may poison the pixels
 * whose footprint holds it, and nothing else.
 * The extent selects the border rule:
 *   frame semantics  extent = the engine's padded frame size (32n; 64n at flow scale 2: rife_hip_padded_size): the engine's COLOUR path - zero padding, coordinates
 *                    clamped at the padded edge.  On the R, G, B planes of an RGB8 pair with the motion of the same call this reproduces the call's frame up to
 *                    the rounding of the last code (the engine scales by 1 / 255 first).
 *   edge semantics   extent = w, h: ordinary edge clamping, and the engine's ALPHA path - with the edge value replicated into the padding both clamped taps read
 *                    the same value, so the extrapolating alpha cancels.
 * Rules (rife_hip_planes_check states them per plane set, every apply call repeats them before it touches anything; a violation is -RIFE_HIP_EINVAL with the fault
 * named in the message): w, h > 0; n in 1..4; a known sample type; maxval in range for integer samples and 0 for float samples; planes non-NULL; each pitch positive,
 * at least the row bytes and a multiple of the element size; each pointer element-aligned; h * pitch < 2^32.  The three plane sets of a call agree in w, h, n,
 * sample and maxval, and the motion passes rife_hip_motion_check for that w, h with both buffers present; the extent is 0, 0 or at least w, h with wp * hp <= 2^27.
 * Row padding and everything around the planes is never written.  The output planes must not overlap the inputs or the motion (documented, not checked).
 * Argument checks come before "no HIP device".
 * The two apply calls need an engine handle only for its device and stream: they work before rife_hip_load and on every model family and mode.
 * The two process_*_apply calls are rife_hip_process_motion / rife_hip_process_device_motion with F32 motion held in tight device buffers of the workspace, followed
 * by the apply launch on the same stream: the motion never leaves device memory.  in0 / in1 / out are tight frames of `pixfmt` (the proxy the motion is estimated
 * on), p0 / p1 / planes_out the planes it is applied to, all w x h.
 *   Contract    frame and planes are byte for byte those of rife_hip_process_motion (F32) followed by rife_hip_apply_motion on its output (device: likewise).
 *   Scope       that of motion export; the families and modes it refuses get -RIFE_HIP_ENOSYS with a message that names them and the words "apply motion",
 *               before anything is written.
 *   Timestep    0 / 1: no network pass and no arithmetic - the frame as for the _px call, the planes of frame 0 / frame 1 copied, integer samples clamped to maxval.
 * Out of scope: interleaved multi-channel samples (RGB48, RGBA64), the batch calls, image (strided-frame) calls with apply, other families for the combined calls,
 * the command line.  Planes at half or twice the motion's resolution: the next section. */
#define RIFE_HIP_SAMPLE_U8  0
#define RIFE_HIP_SAMPLE_U16 1   /* native byte order */
#define RIFE_HIP_SAMPLE_F16 2   /* IEEE binary16 */
#define RIFE_HIP_SAMPLE_F32 3   /* IEEE binary32 */
typedef struct rife_hip_planes {
    int w, h, n, sample, maxval;   /* n planes of w x h samples of type `sample`; maxval: integer samples only, else 0 */
    void* plane[4];
    ptrdiff_t pitch[4];            /* BYTES from one row of the plane to the next */
} rife_hip_planes_t;
int rife_hip_planes_check(const rife_hip_planes_t* p);                       /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
/* the padded frame size of the engine for frames of w x h at the flow scale in force: the extent of "frame semantics" */
int rife_hip_padded_size(const rife_hip_t* r, int w, int h, int* wp, int* hp);
/* planes and motion in device memory: one launch; stream semantics as for the device _px call (NULL = the engine's own stream, synchronised before returning) */
int rife_hip_apply_device_motion(const rife_hip_t* r, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* device_motion,
                                 int wp, int hp, const rife_hip_planes_t* out, void* hip_stream);
/* everything in host memory: upload, launch, download */
int rife_hip_apply_motion(const rife_hip_t* r, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* host_motion, int wp, int hp,
                          const rife_hip_planes_t* out);
/* estimate on in0 / in1, apply to p0 / p1 in the same pass; host memory; out may be NULL (the frame is not wanted) */
int rife_hip_process_apply(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt,
                           const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* planes_out);
/* the same in device memory (d_out is required); stream semantics as for the device _px call */
int rife_hip_process_device_apply(const rife_hip_t* r, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt,
                                  const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* planes_out, void* hip_stream);

/* ---- apply motion at another resolution: planes at half or twice the motion's size - 4:2:0 / 4:2:2 chroma, proxy upscaling (absent in the reference) ----------------
 * 12- and 16-bit Y'CbCr is 4:2:0 or 4:2:2 almost everywhere, and estimating on a half-size proxy costs a quarter of the arithmetic.  Both are the apply kernel with a
 * different motion fetch in front of it: the motion box-averaged over the chroma block, or interpolated up by two.  A SET is three plane descriptors p0, p1, out
 * (the rules of the apply section hold among them: they agree in w, h, n, sample and maxval), a pair of shifts and an extent; a call names a motion field of mw x mh
 * (F32 or F16, both buffers, the rules of rife_hip_motion_check for mw x mh) and 1..4 sets, which may differ in everything: sample type, maxval, n, shift, extent.
 * The admitted shift pairs and the plane size ws x hs each requires:
 *     (0, 0)     mw x mh                                          the apply calls above, byte for byte
 *     (-1, -1)   (mw + 1) / 2 x (mh + 1) / 2                      4:2:0 chroma
 *     (-1, 0)    (mw + 1) / 2 x mh                                4:2:2 chroma
 *     (+1, +1)   ws in {2 mw - 1, 2 mw}, hs in {2 mh - 1, 2 mh}   proxy upscaling
 * Any other pair, or a plane size that does not fit, is -RIFE_HIP_EINVAL with the fault named.  The shift is explicit on purpose: at mw = 1 a plane of width 1 fits
 * shift 0 and shift -1, and the two give different results.
 * The result of a set is the apply definition above, unchanged, in the planes' OWN coordinates (w, h = ws, hs; the extent in plane pixels) on a resampled motion
 * flow', mask' of ws x hs, computed in fp32 from the motion (F16 widened first, exactly), every product and sum rounded separately (no fused multiply-add), in
 * exactly this order; M stands for any of dx0, dy0, dx1, dy1, m:
 *   shift -1 on x   c0 = 2x, c1 = min(2x + 1, mw - 1);   shift -1 on y   r0 = 2y, r1 = min(2y + 1, mh - 1)      (an odd edge is the mean of the samples that exist)
 *   (-1, -1)   s = ((M[r0][c0] + M[r0][c1]) + (M[r1][c0] + M[r1][c1])) * 0.25f;     dx' = s.dx * 0.5f, dy' = s.dy * 0.5f, m' = s.m
 *   (-1, 0)    s = (M[y][c0] + M[y][c1]) * 0.5f;                                    dx' = s.dx * 0.5f, dy' = s.dy,        m' = s.m
 *   (+1, +1)   a x2 bilinear resize with half-pixel centres and edge clamping, x first, then y:
 *              j = x >> 1, jn = (x & 1) ? min(j + 1, mw - 1) : max(j - 1, 0);  i, in from y and mh likewise;  H(r) = M[r][j] * 0.75f + M[r][jn] * 0.25f;
 *              s = H(i) * 0.75f + H(in) * 0.25f;                                    dx' = s.dx * 2.f, dy' = s.dy * 2.f, m' = s.m
 *   (0, 0)     the motion itself
 * This is the engine's own chroma convention (replicated up and box-averaged down, no net shift, siting tags ignored).  Frame semantics on chroma is the extent
 * (wp / 2, hp / 2) of rife_hip_padded_size, which is always even; for shift +1 it is (2 wp, 2 hp) of the proxy's padded size; edge semantics is 0, 0.  A NaN or Inf
 * motion sample poisons the plane pixels whose fetch neighbourhood holds it, and nothing else.
 * Rules (rife_hip_apply_set_check states them for one set; every sets call repeats them per set, the message prefixed "set k:", before it touches anything; a
 * violation is -RIFE_HIP_EINVAL): nsets in 1..4; each descriptor passes rife_hip_planes_check; the three agree; the shift pair is admitted and the plane size fits
 * mw, mh; the extent is 0, 0 or at least the plane size with wp * hp <= 2^27.  Argument checks come before "no HIP device".
 * The two apply_*_sets calls need an engine only for its device and stream: they work before rife_hip_load and on every family and mode.  One launch per set, the
 * motion read once per set.
 * The two process_*_apply_sets calls have motion export's scope and refuse everything else with -RIFE_HIP_ENOSYS and the words "apply motion", before anything is
 * written.  They are byte for byte rife_hip_process_motion / rife_hip_process_device_motion (F32) followed by the _sets apply call: the motion, of the frame size
 * w x h, is held in the workspace's tight device buffers; one apply launch per set on the same stream.  out may be NULL in the host call only.  At timestep 0 / 1
 * there is no network pass and no arithmetic: every set is a copy of its frame-0 / frame-1 planes, integer samples clamped to maxval.
 * Out of scope: shifts beyond +-1, mixed shifts other than (-1, 0), exporting the resampled motion, semi-planar or interleaved chroma, the batch and
 * image calls, the command line, several sets in one launch.  Making the proxy: the next section ("high bit depth"). */
typedef struct rife_hip_apply_set {
    const rife_hip_planes_t* p0; const rife_hip_planes_t* p1; const rife_hip_planes_t* out;
    int shift_x, shift_y;   /* the planes relative to the motion, per axis: 0 same size, -1 half (rounded up), +1 double */
    int wp, hp;             /* extent in the planes' OWN pixels; 0, 0 = the plane size */
} rife_hip_apply_set_t;
int rife_hip_apply_set_check(const rife_hip_apply_set_t* s, int mw, int mh);   /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
/* planes and motion in device memory: one launch per set; stream semantics as for the device _px call */
int rife_hip_apply_device_motion_sets(const rife_hip_t* r, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* device_motion, int mw, int mh,
                                      void* hip_stream);
/* everything in host memory: upload, the launches, download */
int rife_hip_apply_motion_sets(const rife_hip_t* r, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* host_motion, int mw, int mh);
/* estimate on in0 / in1 (w x h = the motion size), apply to every set in the same pass; host memory; out may be NULL (the frame is not wanted) */
int rife_hip_process_apply_sets(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, int nsets,
                                const rife_hip_apply_set_t* sets);
/* the same in device memory (d_out is required); stream semantics as for the device _px call */
int rife_hip_process_device_apply_sets(const rife_hip_t* r, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt, int nsets,
                                       const rife_hip_apply_set_t* sets, void* hip_stream);

/* ---- high bit depth: 12- and 16-bit Y'CbCr and RGB planes in ONE call (absent in the reference) ------------------------------------------------------------------------
 * The resident frame holds ten bits per channel, and the sets calls above already blend the caller's own u16 samples at fp32 on motion estimated from a ten-bit proxy.
 * These calls make that proxy on the device: a caller holding yuv420p12, a 12-bit 4:2:2 mezzanine frame or gbrp16 planes hands them over as they are and gets
 * interpolated planes of the same depth back.  An hbd image is a rife_hip_image_t plus a depth:
 *   pixfmt   RIFE_HIP_PIX_I420P10, _I422P10, _I444P10 (with the usual colour bits) or RIFE_HIP_PIX_RGBP10 (none): the plane LAYOUT, and the ten-bit format the proxy
 *            is made in;
 *   depth    10..16: the samples are codes of `depth` bits in the LOW bits of native-endian u16.
 * Definition, operation by operation (tests/hbd_ref.py states it in numpy):
 *   proxy sample   every sample v of every plane is reduced to ten bits with integer arithmetic,
 *                      depth > 10:  c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023)        (round half up, saturate)
 *                      depth = 10:  c = min(v, 1023)
 *                  and the proxy is the TIGHT frame of the image's pixfmt that holds those codes.
 *   result         byte for byte the planes that rife_hip_process_apply_sets(r, proxy0, proxy1, w, h, timestep, NULL, pixfmt, nsets, sets) writes (device planes:
 *                  rife_hip_process_device_apply_sets), the sets made of the images' planes:
 *                      I444P10, RGBP10   one set:  the three planes, n = 3, shift (0, 0)
 *                      I420P10           set 0: the luma plane, n = 1, shift (0, 0);  set 1: Cb and Cr, n = 2, shift (-1, -1)
 *                      I422P10           set 0: the luma plane, n = 1, shift (0, 0);  set 1: Cb and Cr, n = 2, shift (-1, 0)
 *                  every set with sample RIFE_HIP_SAMPLE_U16, maxval (1 << depth) - 1 and extent 0, 0, i.e. EDGE semantics: zero padding is green in Y'CbCr, so the
 *                  plane's own edge is the border rule, and RGB planes follow the same rule so that there is one.
 *   timestep 0, 1  as in that call: the planes of frame 0 / frame 1 copied, clamped to maxval; no network pass.
 * No proxy frame is returned.  Input samples above maxval are read as stored by the blend and clamped only in the proxy (the rule of the apply calls).  The motion is
 * read once per set, and for I420P10 / I422P10 ONCE for both sets: where the luma stores (8 bytes) and the chroma stores (4 bytes) of the output planes are aligned
 * and w >= 4, one fused launch blends the luma plane and both chroma planes (the same bytes; everything else takes the two launches of the sets call).  The staged host planes
 * (2 bytes per sample, uploaded once, tight) feed the pre-processing and the blend.
 * Scope: that of the combined apply calls - model family rife-v4.6, plain mode, flow scale 1 and 2, precision full and fast.  Any other family or mode (-x, -z, -u)
 * returns -RIFE_HIP_ENOSYS with a message that names it and the words "high bit depth", before anything is written.
 * Rules (rife_hip_hbd_check states them for one image; both calls repeat them for their three images before they touch anything; a violation is -RIFE_HIP_EINVAL with
 * the fault named in the message): rife_hip_image_check passes (so full range is refused, as for every 10-bit format); pixfmt is one of the four layouts above (any
 * other format is named in the message); depth is in 10..16; w * h <= 2^27 and rows * pitch < 2^32 per plane (the rules of the sets calls on the same planes); the
 * three images of a call agree in w, h and pixfmt.  Argument checks come before "no HIP device".  Output planes must not overlap each other or the inputs (documented,
 * not checked); row padding and everything around the output planes is never written.
 * Out of scope: MSB-aligned planar and LSB-aligned semi-planar samples (P010 .. P216 as decoders hold them: "semi-planar high bit depth" below); alpha planes and float planes (the sets calls serve them); resident hbd frames (stream mode)
 * and the batch calls; the command line (its .y4m reader is untouched and keeps refusing C420p12 by name). */
int rife_hip_hbd_check(const rife_hip_image_t* img, int depth);               /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
/* planes in host memory */
int rife_hip_process_hbd(const rife_hip_t* r, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth);
/* planes in device memory; stream semantics as for the device _px call (NULL = the engine's own stream, synchronised before returning) */
int rife_hip_process_device_hbd(const rife_hip_t* r, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth,
                                void* hip_stream);

/* ---- 16-bit packed RGB and RGBA: interleaved 10..16-bit samples in ONE call - 16-bit PNG / PPM stills with or without a matte (absent in the reference) --------------
 * The hbd calls above take planes; a decoded 16-bit PNG is interleaved, R G B (A) per pixel.  These calls take such frames as they are: the same mechanism - motion
 * estimated on a ten-bit proxy made on the device, the caller's own samples blended at fp32 - with kernels that read and write packed pixels, so nobody de-interleaves.
 * The resident frame format, every trunk kernel and every existing call are untouched; there is no new pixfmt number.  A packed image is a descriptor of its own
 * (rife_hip_packed_t below): h rows of w pixels of `channels` interleaved native-endian u16 samples, codes of `depth` bits in the LOW bits.
 * Definition, operation by operation (tests/packed_ref.py states it in numpy); P_k(img) is the w x h plane of channel k of a packed image:
 *   proxy          the TIGHT RIFE_HIP_PIX_RGBP10 frame whose planes are reduce10(P_0), reduce10(P_1), reduce10(P_2), with the hbd section's reduction
 *                      depth > 10:  c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023)        depth = 10:  c = min(v, 1023)
 *                  Alpha never reaches the network.
 *   result         channel k of `out` is, byte for byte, plane k of rife_hip_process_apply_sets(r, proxy0, proxy1, w, h, timestep, NULL, RIFE_HIP_PIX_RGBP10, 1, set)
 *                  with the set of n = channels planes P_k(in0), P_k(in1), shift (0, 0), RIFE_HIP_SAMPLE_U16, maxval = (1 << depth) - 1, extent 0, 0 (edge
 *                  semantics).  For channels = 3 this is rife_hip_process_hbd with the RGBP10 layout on the de-interleaved planes.  The alpha channel is a fourth
 *                  plane of the same set: warped by the flow estimated from the colour it belongs to, blended by the same mask, with edge clamping - the engine's
 *                  alpha rule.  Opaque in (A = maxval everywhere) gives maxval everywhere.  Straight or premultiplied: the four channels are interpolated as given.
 *   timestep 0, 1  no network pass: the samples of frame 0 / frame 1 copied, each clamped to maxval.
 * Input samples above maxval are read as stored by the blend and clamped only in the proxy (the rule of the apply calls).  The host call stages both frames once
 * (2 bytes per sample, tight) and brings the result back with one 2-D copy; the device call reads and writes the caller's frames in place, stream semantics as for the
 * device _px call.
 * Scope: that of the hbd calls - model family rife-v4.6, plain mode, flow scale 1 and 2, precision full and fast.  Any other family or mode (-x, -z, -u) returns
 * -RIFE_HIP_ENOSYS with a message that names it and the words "high bit depth", before anything is written.
 * Rules (rife_hip_packed_check states them for one image; both calls repeat them for their three images before they touch anything; a violation is -RIFE_HIP_EINVAL with
 * the fault named and the prefix "high bit depth: image 0: " / "image 1: " / "image out: "): w, h > 0; channels is 3 or 4; depth is in 10..16; data is non-NULL and
 * aligned to 2; pitch is positive, at least w * channels * 2, a multiple of 2 and at most INT32_MAX; w * h <= 2^27; h * pitch < 2^32; the three images of a call agree
 * in w, h, channels and depth.  Argument checks come before "no HIP device".  Row padding and everything around `out` is never written.  The output must not overlap the
 * inputs (documented, not checked).
 * Out of scope: a public apply-only call on packed frames; packed float or u8 frames; BGR(A) channel order; resident packed frames (stream mode) and the batch calls;
 * MSB-aligned samples. */
typedef struct rife_hip_packed {
    int w, h;
    int channels;      /* 3: R G B;  4: R G B A */
    int depth;         /* 10..16: codes of `depth` bits in the LOW bits of native-endian u16 */
    void* data;        /* h rows of w pixels of `channels` interleaved u16 samples */
    ptrdiff_t pitch;   /* BYTES from one row to the next */
} rife_hip_packed_t;
int rife_hip_packed_check(const rife_hip_packed_t* img);                     /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
/* frames in host memory */
int rife_hip_process_hbd_packed(const rife_hip_t* r, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out);
/* frames in device memory; stream semantics as for the device _px call (NULL = the engine's own stream, synchronised before returning) */
int rife_hip_process_device_hbd_packed(const rife_hip_t* r, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out,
                                       void* hip_stream);

/* ---- semi-planar high bit depth: decoder surfaces - P010 / P012 / P016 and P210 / P212 / P216 - in ONE call (absent in the reference) ---------------------------------
 * The hbd calls above take three planes with the code in the LOW bits.  A hardware decoder surface, and every ffmpeg hw-frame format above 8 bits, is a Y plane plus ONE
 * plane of interleaved Cb, Cr pairs with the code in the HIGH bits of each u16.  These calls take such surfaces as they are: the same mechanism - motion estimated on a
 * ten-bit proxy made on the device, the caller's own samples blended at fp32 - with kernels that read and write interleaved chroma and shift on the way, so nobody
 * de-interleaves or shifts.  The resident frame format, every trunk kernel and every existing call are untouched; there is no new pixfmt number (rife_hip_hbd_check keeps
 * refusing RIFE_HIP_PIX_P010, which stays the ten-bit 4:2:0 format of the _px and image calls).  A semi-planar image is a descriptor of its own (rife_hip_semiplanar_t
 * below).
 * Definition, operation by operation (tests/semiplanar_ref.py states it in numpy); s = 16 - depth:
 *   split(img)     the three planes Y >> s (h x w), Cb >> s and Cr >> s (each ch x cw, cw = (w + 1) / 2, ch = (h + 1) / 2 for chroma 1 and h for chroma 2): sample 2 i of
 *                  a cbcr row is Cb of chroma pixel i, sample 2 i + 1 its Cr.  The low s bits of an input sample are ignored.
 *   join(planes)   the inverse on codes: Y << s, and Cb << s, Cr << s interleaved; the low s bits are zero.
 *   result         byte for byte join(planes << s) of the planes rife_hip_process_hbd(r, split(in0), split(in1), timestep, planes, depth) writes (device surfaces:
 *                  rife_hip_process_device_hbd), the planar images of pixfmt RIFE_HIP_PIX_I420P10 | csp (chroma 1) or RIFE_HIP_PIX_I422P10 | csp (chroma 2).
 *                  Everything of the hbd definition carries over unchanged: the proxy sample c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023) (depth 10:
 *                  c = min(v, 1023)) of every code v, the luma set at shift (0, 0) and the chroma set at (-1, -1) or (-1, 0), edge semantics, u16 samples,
 *                  maxval = (1 << depth) - 1.
 *   timestep 0, 1  no network pass: (v >> s) << s of every sample of frame 0 / frame 1.
 * The host call stages both images once (2 bytes per sample, tight) and brings the result back with two 2-D copies; the device call reads and writes the caller's
 * surfaces in place, stream semantics as for the device _px call.  ONE launch blends the luma plane and the interleaved chroma plane; a chroma tap row is one load of
 * the four samples Cb, Cr, Cb, Cr of two neighbouring chroma pixels.
 * Scope: that of the hbd calls - model family rife-v4.6, plain mode, flow scale 1 and 2, precision full and fast.  Any other family or mode (-x, -z, -u) returns
 * -RIFE_HIP_ENOSYS with a message that names it and the words "high bit depth", before anything is written.
 * Rules (rife_hip_semiplanar_check states them for one image; both calls repeat them for their three images before they touch anything; a violation is
 * -RIFE_HIP_EINVAL with the fault named and the prefix "high bit depth: image 0: " / "image 1: " / "image out: "): w, h > 0; chroma is 1 or 2 (3 is refused with a
 * message that says 4:4:4 semi-planar is not served); csp is one of the three matrices (RIFE_HIP_CSP_FULL is refused by name, as for every 10-bit format); depth is in
 * 10..16; y and cbcr are non-NULL and aligned to 2; both pitches are positive, multiples of 2 and at most INT32_MAX; pitch_y >= 2 w; pitch_c >= 4 ((w + 1) / 2);
 * w * h <= 2^27; rows * pitch < 2^32 for each plane; the three images of a call agree in w, h, chroma, csp and depth.  Argument checks come before "no HIP device".
 * Row padding and everything around the output planes is never written.  The output must not overlap the inputs (documented, not checked).
 * Out of scope: 4:4:4 semi-planar (P410 / P416); Cr, Cb order (NV21-like); LSB-aligned semi-planar and MSB-aligned planar samples; 8-bit NV12 / NV16 through this
 * path; a public apply-only call on semi-planar surfaces; resident semi-planar frames (stream mode) and the batch calls; the command line (no container it reads holds
 * these layouts). */
typedef struct rife_hip_semiplanar {
    int w, h;            /* luma size; chroma is (w + 1) / 2 pairs wide, (h + 1) / 2 rows (chroma 1) or h rows (chroma 2) */
    int chroma;          /* 1: 4:2:0 (P010 / P012 / P016)   2: 4:2:2 (P210 / P212 / P216) */
    int csp;             /* RIFE_HIP_CSP_BT709 / _BT601 / _BT2020NCL; RIFE_HIP_CSP_FULL is refused, as for every 10-bit format */
    int depth;           /* 10..16: codes of `depth` bits in the HIGH bits of little-endian u16; low bits ignored on input, written as zero */
    void* y;    ptrdiff_t pitch_y;   /* BYTES per row */
    void* cbcr; ptrdiff_t pitch_c;   /* rows of interleaved Cb, Cr pairs */
} rife_hip_semiplanar_t;
int rife_hip_semiplanar_check(const rife_hip_semiplanar_t* img);             /* host only, no device needed: 0, or -RIFE_HIP_EINVAL with the fault in the last-error message */
/* surfaces in host memory */
int rife_hip_process_hbd_semiplanar(const rife_hip_t* r, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep,
                                    const rife_hip_semiplanar_t* out);
/* surfaces in device memory; stream semantics as for the device _px call (NULL = the engine's own stream, synchronised before returning) */
int rife_hip_process_device_hbd_semiplanar(const rife_hip_t* r, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep,
                                           const rife_hip_semiplanar_t* out, void* hip_stream);

const char* rife_hip_last_error(void);

/* ---- measurement hooks (bench.py / profiles) ---------------------------------------------------------------
 * When enabled, every launch of the engine's kernels is bracketed by HIP events on the launch stream; read-out
 * synchronises and returns per-kernel-class totals.  `names` receives '\n'-separated class names. */
int rife_hip_profile_enable(rife_hip_t* r, int on);
int rife_hip_profile_read(rife_hip_t* r, char* names, size_t names_cap, double* total_ms, long long* launches,
                          double* flops, int max_classes);   /* returns number of classes */

/* Dry run of the generic graph executor's loader on one ncnn .param file (no GPU needed): 0 if every layer of the graph has a
 * kernel, RIFE_HIP_EMODEL with the offending layer in rife_hip_last_error() otherwise.  The v1 family (models/rife, rife-HD,
 * rife-UHD, rife-anime) is executed from its .param layer by layer, like ncnn::Net does for every model (src/rife.cpp:112-121). */
int rife_hip_graph_check(const char* param_path_without_extension);
/* Structural hash of the sub-graph that produces blob `blob` of an ncnn .param file (layer types, parameters, topology; no names,
 * no weights) - what rife_hip_load() compares with the compiled-in constants of csrc/model_hashes.h to prove that a model directory
 * holds the graph a fused schedule was written for (the reference's models/rife-v4.6/flownet.param etc.).  CPU only. */
int rife_hip_param_hash(const char* param_path, const char* blob, uint64_t* hash_out);

/* ---- page-locked host frames (optional) -------------------------------------------------------------------------------
 * rife_hip_process() takes any host pointer, like RIFE::process() takes any ncnn::Mat (src/main.cpp:187, 332).  Copies from / to
 * pageable memory are staged by the HIP runtime and hold the calling thread for their whole duration; from page-locked memory they
 * are asynchronous DMA at PCIe rate, so that with two caller threads (the reference's default -j 1:2:2) one pair's copies run
 * under the other pair's kernels.  A caller without HIP headers can get such memory here: allocate frames with
 * rife_hip_host_alloc() (returns NULL on failure), or page-lock buffers it already owns for as long as it keeps them
 * (rife_hip_host_register / rife_hip_host_unregister; the range must stay mapped in between).  Pixels are identical either way. */
void* rife_hip_host_alloc(size_t bytes);
void rife_hip_host_free(void* p);
int rife_hip_host_register(void* p, size_t bytes);
int rife_hip_host_unregister(void* p);

#ifdef __cplusplus
}
#endif
#endif /* RIFE_HIP_H */
