// RIFE — same class name, constructor and member signatures as the reference (src/rife.h:11-52), implemented on
// librife_hip.so (include/rife_hip.h) instead of ncnn + Vulkan.  `src/main.cpp` of the reference compiles against
// this header unchanged apart from the include path of the Mat type.
#ifndef RIFE_H
#define RIFE_H

#include <string>

#include "ncnn_mat.h"
#include "../../include/rife_hip.h"      // rife_hip_image_t for the image calls below

struct rife_hip;
struct rife_hip_frame;

class RIFE
{
public:
    RIFE(int gpuid, bool tta_mode = false, bool tta_temporal_mode = false, bool uhd_mode = false, int num_threads = 1, bool rife_v2 = false, bool rife_v4 = false);
    ~RIFE();

    int load(const std::string& modeldir);

    int process(const ncnn::Mat& in0image, const ncnn::Mat& in1image, float timestep, ncnn::Mat& outimage) const;

    // Extension, not in the reference (include/rife_hip.h "UHD / flow scale"): estimate flow at 1 / divisor of the usual resolution - 1 = the reference's graph,
    // 2 = every IFBlock at half its resolution (upstream RIFE's scale=0.5, for UHD material; rife-v4.6, plain mode).  After load(), with no call in flight.
    // Returns the C-ABI's code; the message of a refusal is rife_hip_last_error().
    int set_flow_scale(int divisor);

    // Extension, not in the reference (include/rife_hip.h "precision"): RIFE_HIP_PRECISION_FULL (the default) or RIFE_HIP_PRECISION_FAST - one f16 product per
    // weight tap of the residual trunk convolutions, the skip connection at full precision (rife-v4.6, plain mode).  After load(), with no call in flight.
    // Returns the C-ABI's code; the message of a refusal is rife_hip_last_error().
    int set_precision(int precision);
    int precision() const;

    // The reference exposes its four back-ends publicly (src/rife.h:25-29).  Here the HIP engine is the only one:
    // process_v4 == process for rife_v4 objects; the *_cpu entry points report an error (no CPU path in this build).
    int process_cpu(const ncnn::Mat& in0image, const ncnn::Mat& in1image, float timestep, ncnn::Mat& outimage) const;
    int process_v4(const ncnn::Mat& in0image, const ncnn::Mat& in1image, float timestep, ncnn::Mat& outimage) const;
    int process_v4_cpu(const ncnn::Mat& in0image, const ncnn::Mat& in1image, float timestep, ncnn::Mat& outimage) const;

    // Extension, not in the reference (include/rife_hip.h "stream mode"): a frame uploaded once and used by several process()
    // calls - consecutive pairs share a frame, and every timestep of a pair shares both.  Same pixels as the host-buffer call.
    rife_hip_frame* upload(const ncnn::Mat& image) const;
    int process(const rife_hip_frame* frame0, const rife_hip_frame* frame1, float timestep, ncnn::Mat& outimage) const;
    static void release(rife_hip_frame* frame);

    // Extension, not in the reference (include/rife_hip.h "video"): planar Y'CbCr frames (4:2:0, 4:2:2, 4:4:4).  An ncnn::Mat has no natural shape for them, so these take plain pointers
    // to tightly packed frames of `pixfmt` (RIFE_HIP_PIX_NV12 .. I420P10, I422, I422P10, I444, I444P10 | RIFE_HIP_CSP_*), rife_hip_frame_bytes(w, h, pixfmt) bytes each.  rife-v4.6, plain mode.
    // A frame of upload_yuv() goes through process(frame0, frame1, timestep, outimage) above, whose outimage.data then points at a frame of that size.
    // Both forward `pixfmt` unfiltered, so they serve every planar format of the _px calls: the planar RGB formats too (include/rife_hip.h "planar RGB":
    // RIFE_HIP_PIX_RGBP8 / RGBP10 / RGBPH / RGBPF, three planes R, G, B glued one after the other, no colour bits).
    int process_yuv(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt) const;
    rife_hip_frame* upload_yuv(const void* frame, int w, int h, int pixfmt) const;

    // Extension, not in the reference (include/rife_hip.h "motion export"): the frame AND the motion it was made from - the final flows (h rows of w pixels of dx0, dy0,
    // dx1, dy1) and the blend mask (the weight of frame 0's warp), into the host buffers `motion` names with their pitches in bytes (either may be null).  Plain pointers
    // to tightly packed frames of any _px format, as for process_yuv; the frame is byte for byte the one of the call without motion.  rife-v4.6, plain mode.
    int process_motion(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, const rife_hip_motion_t& motion) const;
    int process_frames_motion(const rife_hip_frame* frame0, const rife_hip_frame* frame1, float timestep, void* out, const rife_hip_motion_t& motion) const;

    // Extension, not in the reference (include/rife_hip.h "apply motion"): a motion field applied to the caller's own planes - n <= 4 planes of u8 / u16 / half / float
    // samples, a pointer and a pitch in bytes each - at fp32: 16-bit and float pictures, alpha, mattes, depth, the raw frame behind a denoised proxy.  Host memory.
    // apply_motion needs no loaded model; process_apply estimates on the tight frames in0 / in1 of `pixfmt` (out may be null: the frame is not wanted) and applies in
    // the same pass, the motion staying in device memory.  wp, hp: the extent (0, 0 = edge clamping; rife_hip_padded_size = the engine's frame semantics).
    int apply_motion(const rife_hip_planes_t& p0, const rife_hip_planes_t& p1, const rife_hip_motion_t& motion, int wp, int hp, const rife_hip_planes_t& out) const;
    int process_apply(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, const rife_hip_planes_t& p0, const rife_hip_planes_t& p1,
                      int wp, int hp, const rife_hip_planes_t& planes_out) const;
    // The same for planes at half or twice the motion's resolution (include/rife_hip.h "apply motion at another resolution"): 1..4 sets of three plane descriptors
    // with a shift pair each - (0, 0), (-1, -1) 4:2:0 chroma, (-1, 0) 4:2:2 chroma, (1, 1) proxy upscaling - on a motion of mw x mh (process_apply_sets: w x h).
    int apply_motion_sets(int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t& motion, int mw, int mh) const;
    int process_apply_sets(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, int nsets, const rife_hip_apply_set_t* sets) const;
    // High-bit-depth planes in one call (include/rife_hip.h "high bit depth"): host planes of `depth`-bit samples (10..16) in u16, laid out as RIFE_HIP_PIX_I420P10 /
    // _I422P10 / _I444P10 / _RGBP10 images; the ten-bit proxy the motion is estimated on is made on the device, the blend runs on the planes themselves.
    int process_hbd(const rife_hip_image_t& in0, const rife_hip_image_t& in1, float timestep, const rife_hip_image_t& out, int depth) const;
    // Packed 16-bit RGB / RGBA frames in one call (include/rife_hip.h "16-bit packed RGB and RGBA"): host frames of 3 or 4 interleaved u16 samples per pixel as
    // descriptors (an ncnn::Mat with elemsize 6, elempack 3 already means RGB10_U16 and is not overloaded); alpha is warped and blended with the colour.
    int process_hbd_packed(const rife_hip_packed_t& in0, const rife_hip_packed_t& in1, float timestep, const rife_hip_packed_t& out) const;
    // Decoder surfaces in one call (include/rife_hip.h "semi-planar high bit depth"): host surfaces of a Y plane and one plane of interleaved Cb, Cr pairs, codes of
    // 10..16 bits in the HIGH bits of u16 (P010 / P012 / P016, P210 / P212 / P216), as descriptors; nothing is de-interleaved or shifted on the host.
    int process_hbd_semiplanar(const rife_hip_semiplanar_t& in0, const rife_hip_semiplanar_t& in1, float timestep, const rife_hip_semiplanar_t& out) const;

    // Extension, not in the reference (include/rife_hip.h "strides and planes"): frames as an AVFrame or a VapourSynth frame holds them - a pointer and a
    // pitch in BYTES per plane, any of the _px formats (planar RGB: R, G, B in plane[0..2]; ffmpeg's gbrp: permute them).  Host planes; plain pass-throughs to rife_hip_process_image / rife_hip_frame_upload_image (inline: a
    // program that never calls them links against an engine without those two symbols as before; the message of a failure is rife_hip_last_error()).
    int process_image(const rife_hip_image_t& in0, const rife_hip_image_t& in1, float timestep, const rife_hip_image_t& out) const
    {
        return engine ? rife_hip_process_image(engine, &in0, &in1, timestep, &out) : -RIFE_HIP_ENODEV;
    }
    rife_hip_frame* upload_image(const rife_hip_image_t& image) const
    {
        rife_hip_frame* f = 0;
        if (engine) rife_hip_frame_upload_image(engine, &image, &f);
        return f;
    }

private:
    RIFE(const RIFE&);
    RIFE& operator=(const RIFE&);
    rife_hip* engine;
    int gpuid;
    bool rife_v4;
};

#endif // RIFE_H
