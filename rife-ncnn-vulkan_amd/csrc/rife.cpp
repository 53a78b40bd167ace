// RIFE class shim over the C-ABI (see rife.h).  Behaviour kept from the reference:
//   * constructor never fails; an unusable device surfaces at load()/process() (reference: vkdev lookup, rife.cpp:27-47)
//   * process() with timestep 0 / 1 rebinds outimage to an input Mat, sharing its buffer (rife.cpp:395-405, 2470-2480)
//   * return value 0 = ok (rife.cpp:1211, 3201); errors are printed to stderr like ncnn does and returned negative
#include "rife.h"

#include <cstdio>

#include "../../include/rife_hip.h"

// the pixel format of a Mat at this boundary: elemsize 6, elempack 3 = three u16 codes 0..1023 per pixel (RIFE_HIP_PIX_RGB10_U16); elemsize 4, elempack 4 =
// u8 RGBA (RIFE_HIP_PIX_RGBA8); every other Mat is the
// 8-bit RGB Mat the reference builds (src/main.cpp:187, 332)
static int mat_pixfmt(const ncnn::Mat& m)
{
    if (m.elemsize == 4 && m.elempack == 4) return RIFE_HIP_PIX_RGBA8;      // four u8 per pixel, R G B A: alpha is carried through
    return (m.elemsize == 6 && m.elempack == 3) ? RIFE_HIP_PIX_RGB10_U16 : RIFE_HIP_PIX_RGB8;
}

RIFE::RIFE(int gpuid_, bool tta_mode, bool tta_temporal_mode, bool uhd_mode, int num_threads, bool rife_v2, bool rife_v4_)
    : engine(0), gpuid(gpuid_), rife_v4(rife_v4_)
{
    if (gpuid >= 0)
        engine = rife_hip_create(gpuid, tta_mode, tta_temporal_mode, uhd_mode, num_threads, rife_v2, rife_v4);
    if (!engine)
        fprintf(stderr, "RIFE: %s\n", gpuid < 0 ? "gpuid -1 (CPU device) is not served by the HIP engine" : rife_hip_last_error());
}

RIFE::~RIFE()
{
    if (engine) rife_hip_destroy(engine);
}

int RIFE::load(const std::string& modeldir)
{
    if (!engine) return -RIFE_HIP_ENODEV;
    int ret = rife_hip_load(engine, modeldir.c_str());
    if (ret) fprintf(stderr, "RIFE::load: %s\n", rife_hip_last_error());
    return ret;
}

// A weak reference: a host program linked against an engine stand-in that predates the call (tests/test_cli_yuv.py links main.cpp and this file against two stub
// files) still links; the call then reports -RIFE_HIP_ENOSYS.  librife_hip.so always defines it.
extern "C" int rife_hip_set_flow_scale(rife_hip_t* r, int divisor) __attribute__((weak));

int RIFE::set_flow_scale(int divisor)
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_set_flow_scale)
    {
        fprintf(stderr, "RIFE::set_flow_scale: this engine has no flow scale\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_set_flow_scale(engine, divisor);
    if (ret) fprintf(stderr, "RIFE::set_flow_scale: %s\n", rife_hip_last_error());
    return ret;
}

// weak for the same reason: an engine stand-in without the two precision calls still links
extern "C" int rife_hip_set_precision(rife_hip_t* r, int precision) __attribute__((weak));
extern "C" int rife_hip_precision(const rife_hip_t* r) __attribute__((weak));

int RIFE::set_precision(int precision)
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_set_precision)
    {
        fprintf(stderr, "RIFE::set_precision: this engine has one precision\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_set_precision(engine, precision);
    if (ret) fprintf(stderr, "RIFE::set_precision: %s\n", rife_hip_last_error());
    return ret;
}

int RIFE::precision() const
{
    return engine && rife_hip_precision ? rife_hip_precision(engine) : RIFE_HIP_PRECISION_FULL;
}

int RIFE::process(const ncnn::Mat& in0image, const ncnn::Mat& in1image, float timestep, ncnn::Mat& outimage) const
{
    const int pixfmt = mat_pixfmt(in0image);
    if (pixfmt != mat_pixfmt(in1image) || (outimage.data && mat_pixfmt(outimage) != pixfmt))
    {
        fprintf(stderr, "RIFE::process: the three images differ in pixel format (8-bit RGB, RGBA and 10-bit Mats mixed)\n");
        return -RIFE_HIP_EINVAL;
    }

    if (timestep == 0.f)
    {
        outimage = in0image;
        return 0;
    }

    if (timestep == 1.f)
    {
        outimage = in1image;
        return 0;
    }

    if (!engine) return -RIFE_HIP_ENODEV;
    if (in0image.w != in1image.w || in0image.h != in1image.h || outimage.w != in0image.w || outimage.h != in0image.h || !outimage.data)
    {
        fprintf(stderr, "RIFE::process: frame size mismatch\n");
        return -RIFE_HIP_EINVAL;
    }

    int ret = pixfmt == RIFE_HIP_PIX_RGB8
                  ? rife_hip_process(engine, (const unsigned char*)in0image.data, (const unsigned char*)in1image.data, in0image.w, in0image.h, timestep, (unsigned char*)outimage.data)
                  : rife_hip_process_px(engine, in0image.data, in1image.data, in0image.w, in0image.h, timestep, outimage.data, pixfmt);
    if (ret) fprintf(stderr, "RIFE::process: %s\n", rife_hip_last_error());
    return ret;
}

rife_hip_frame* RIFE::upload(const ncnn::Mat& image) const
{
    if (!engine || !image.data) return 0;
    rife_hip_frame* f = 0;
    const int pixfmt = mat_pixfmt(image);
    if (pixfmt == RIFE_HIP_PIX_RGB8 ? rife_hip_frame_upload(engine, (const unsigned char*)image.data, image.w, image.h, &f)
                                    : rife_hip_frame_upload_px(engine, image.data, image.w, image.h, pixfmt, &f))
        fprintf(stderr, "RIFE::upload: %s\n", rife_hip_last_error());
    return f;
}

int RIFE::process(const rife_hip_frame* frame0, const rife_hip_frame* frame1, float timestep, ncnn::Mat& outimage) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!outimage.data) return -RIFE_HIP_EINVAL;
    // the engine checks the two frames against each other; outimage must be the caller's w x h x 3 buffer as in main.cpp:332
    int ret = rife_hip_process_frames(engine, frame0, frame1, timestep, (unsigned char*)outimage.data);
    if (ret) fprintf(stderr, "RIFE::process: %s\n", rife_hip_last_error());
    return ret;
}

int RIFE::process_yuv(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    int ret = rife_hip_process_px(engine, in0, in1, w, h, timestep, out, pixfmt);
    if (ret) fprintf(stderr, "RIFE::process_yuv: %s\n", rife_hip_last_error());
    return ret;
}

// weak like the precision calls: an engine stand-in without the motion calls still links, and the call then reports -RIFE_HIP_ENOSYS
extern "C" int rife_hip_process_motion(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt,
                                       const rife_hip_motion_t* host_motion) __attribute__((weak));
extern "C" int rife_hip_process_frames_motion(const rife_hip_t* r, const rife_hip_frame_t* frame0, const rife_hip_frame_t* frame1, float timestep, void* out,
                                              const rife_hip_motion_t* host_motion) __attribute__((weak));

int RIFE::process_motion(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, const rife_hip_motion_t& motion) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_motion)
    {
        fprintf(stderr, "RIFE::process_motion: this engine has no motion export\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_motion(engine, in0, in1, w, h, timestep, out, pixfmt, &motion);
    if (ret) fprintf(stderr, "RIFE::process_motion: %s\n", rife_hip_last_error());
    return ret;
}

int RIFE::process_frames_motion(const rife_hip_frame* frame0, const rife_hip_frame* frame1, float timestep, void* out, const rife_hip_motion_t& motion) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_frames_motion)
    {
        fprintf(stderr, "RIFE::process_frames_motion: this engine has no motion export\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_frames_motion(engine, frame0, frame1, timestep, out, &motion);
    if (ret) fprintf(stderr, "RIFE::process_frames_motion: %s\n", rife_hip_last_error());
    return ret;
}

// weak like the motion calls: an engine stand-in without the apply calls still links, and the call then reports -RIFE_HIP_ENOSYS
extern "C" int rife_hip_apply_motion(const rife_hip_t* r, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* host_motion, int wp, int hp,
                                     const rife_hip_planes_t* out) __attribute__((weak));
extern "C" int rife_hip_process_apply(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt,
                                      const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* planes_out) __attribute__((weak));

int RIFE::apply_motion(const rife_hip_planes_t& p0, const rife_hip_planes_t& p1, const rife_hip_motion_t& motion, int wp, int hp, const rife_hip_planes_t& out) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_apply_motion)
    {
        fprintf(stderr, "RIFE::apply_motion: this engine has no apply motion\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_apply_motion(engine, &p0, &p1, &motion, wp, hp, &out);
    if (ret) fprintf(stderr, "RIFE::apply_motion: %s\n", rife_hip_last_error());
    return ret;
}

int RIFE::process_apply(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, const rife_hip_planes_t& p0, const rife_hip_planes_t& p1,
                        int wp, int hp, const rife_hip_planes_t& planes_out) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_apply)
    {
        fprintf(stderr, "RIFE::process_apply: this engine has no apply motion\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_apply(engine, in0, in1, w, h, timestep, out, pixfmt, &p0, &p1, wp, hp, &planes_out);
    if (ret) fprintf(stderr, "RIFE::process_apply: %s\n", rife_hip_last_error());
    return ret;
}

// weak like the apply calls
extern "C" int rife_hip_apply_motion_sets(const rife_hip_t* r, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* host_motion, int mw, int mh)
    __attribute__((weak));
extern "C" int rife_hip_process_apply_sets(const rife_hip_t* r, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, int nsets,
                                           const rife_hip_apply_set_t* sets) __attribute__((weak));

int RIFE::apply_motion_sets(int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t& motion, int mw, int mh) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_apply_motion_sets)
    {
        fprintf(stderr, "RIFE::apply_motion_sets: this engine has no apply motion at another resolution\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_apply_motion_sets(engine, nsets, sets, &motion, mw, mh);
    if (ret) fprintf(stderr, "RIFE::apply_motion_sets: %s\n", rife_hip_last_error());
    return ret;
}

int RIFE::process_apply_sets(const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, int nsets, const rife_hip_apply_set_t* sets) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_apply_sets)
    {
        fprintf(stderr, "RIFE::process_apply_sets: this engine has no apply motion at another resolution\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_apply_sets(engine, in0, in1, w, h, timestep, out, pixfmt, nsets, sets);
    if (ret) fprintf(stderr, "RIFE::process_apply_sets: %s\n", rife_hip_last_error());
    return ret;
}

// weak like the apply calls
extern "C" int rife_hip_process_hbd(const rife_hip_t* r, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth)
    __attribute__((weak));

int RIFE::process_hbd(const rife_hip_image_t& in0, const rife_hip_image_t& in1, float timestep, const rife_hip_image_t& out, int depth) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_hbd)
    {
        fprintf(stderr, "RIFE::process_hbd: this engine has no high bit depth call\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_hbd(engine, &in0, &in1, timestep, &out, depth);
    if (ret) fprintf(stderr, "RIFE::process_hbd: %s\n", rife_hip_last_error());
    return ret;
}

// weak like the hbd call
extern "C" int rife_hip_process_hbd_packed(const rife_hip_t* r, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out)
    __attribute__((weak));

int RIFE::process_hbd_packed(const rife_hip_packed_t& in0, const rife_hip_packed_t& in1, float timestep, const rife_hip_packed_t& out) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_hbd_packed)
    {
        fprintf(stderr, "RIFE::process_hbd_packed: this engine has no packed high bit depth call\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_hbd_packed(engine, &in0, &in1, timestep, &out);
    if (ret) fprintf(stderr, "RIFE::process_hbd_packed: %s\n", rife_hip_last_error());
    return ret;
}

// weak like the hbd call
extern "C" int rife_hip_process_hbd_semiplanar(const rife_hip_t* r, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep,
                                               const rife_hip_semiplanar_t* out) __attribute__((weak));

int RIFE::process_hbd_semiplanar(const rife_hip_semiplanar_t& in0, const rife_hip_semiplanar_t& in1, float timestep, const rife_hip_semiplanar_t& out) const
{
    if (!engine) return -RIFE_HIP_ENODEV;
    if (!rife_hip_process_hbd_semiplanar)
    {
        fprintf(stderr, "RIFE::process_hbd_semiplanar: this engine has no semi-planar high bit depth call\n");
        return -RIFE_HIP_ENOSYS;
    }
    int ret = rife_hip_process_hbd_semiplanar(engine, &in0, &in1, timestep, &out);
    if (ret) fprintf(stderr, "RIFE::process_hbd_semiplanar: %s\n", rife_hip_last_error());
    return ret;
}

rife_hip_frame* RIFE::upload_yuv(const void* frame, int w, int h, int pixfmt) const
{
    if (!engine || !frame) return 0;
    rife_hip_frame* f = 0;
    if (rife_hip_frame_upload_px(engine, frame, w, h, pixfmt, &f))
        fprintf(stderr, "RIFE::upload_yuv: %s\n", rife_hip_last_error());
    return f;
}

void RIFE::release(rife_hip_frame* frame)
{
    rife_hip_frame_release(frame);
}

int RIFE::process_v4(const ncnn::Mat& in0image, const ncnn::Mat& in1image, float timestep, ncnn::Mat& outimage) const
{
    return process(in0image, in1image, timestep, outimage);
}

int RIFE::process_cpu(const ncnn::Mat&, const ncnn::Mat&, float, ncnn::Mat&) const
{
    fprintf(stderr, "RIFE::process_cpu: this build has no CPU path\n");
    return -RIFE_HIP_ENOSYS;
}

int RIFE::process_v4_cpu(const ncnn::Mat&, const ncnn::Mat&, float, ncnn::Mat&) const
{
    fprintf(stderr, "RIFE::process_v4_cpu: this build has no CPU path\n");
    return -RIFE_HIP_ENOSYS;
}
