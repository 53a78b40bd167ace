// engine_image.h: the image entry points of include/rife_hip.h (rife_hip_image_t: strided frames, separate planes) on top of engine_abi.h
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
//   device planes: run_v4 with the three plane sets - the pitched kernels of planes.h read and write the caller's planes in place; the RGB formats' quantising kernels
//                  write the workspace's tight frame (Ctx::d_out) and k_store_rows moves it into the caller's pitch on the same stream
//   host planes:   2-D copies per plane between the caller's planes and the tight staging buffers, then the path of the _px calls (same upload token)
// An image whose planes are all tight IS the _px call and goes there.
// The skeleton around them is engine_abi.h's: StreamWorkspace, with_leased_ctx, upload_with_token, CopyStreamLease, guarded.

// 0, or -RIFE_HIP_EINVAL: the rules of rife_hip_image_check on every image of a call, and that they agree
static int image_precheck(std::initializer_list<const rife_hip_image_t*> imgs) {
    std::string err;
    const rife_hip_image_t* first = nullptr;
    for (const rife_hip_image_t* im : imgs) {
        if (rife_img::check(im, err)) return fail(RIFE_HIP_EINVAL, "image: " + err);
        if (first && rife_img::check_same(first, im, err)) return fail(RIFE_HIP_EINVAL, err);
        if (!first) first = im;
    }
    return no_hip_device();
}
// strided images are served by the plain rife-v4.6 schedule only (RGB8 included: the other families' pre-processing reads tight frames)
static int image_supported(const rife_hip* E) { return plain_v46_only(E, "strided and planar images are"); }
// byte offset of plane p in the tight frame of the _px calls
static size_t image_tight_offset(int w, int h, int pixfmt, int p) {
    size_t off = 0;
    for (int q = 0; q < p; q++) off += rife_img::row_bytes(w, pixfmt, q) * (size_t)rife_img::plane_rows(h, pixfmt, q);
    return off;
}
// 2-D copies per plane between an image and a tight frame (either side host or device, `kind` says which)
static hipError_t image_copy_to_tight(void* tight, const rife_hip_image_t& im, hipMemcpyKind kind, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (int p = 0; p < rife_img::planes(im.pixfmt) && e == hipSuccess; p++) {
        const size_t rb = rife_img::row_bytes(im.w, im.pixfmt, p);
        e = hipMemcpy2DAsync(static_cast<uint8_t*>(tight) + image_tight_offset(im.w, im.h, im.pixfmt, p), rb, im.plane[p], (size_t)im.pitch[p], rb, (size_t)rife_img::plane_rows(im.h, im.pixfmt, p), kind, st);
    }
    return e;
}
static hipError_t image_copy_from_tight(const rife_hip_image_t& im, const void* tight, hipMemcpyKind kind, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (int p = 0; p < rife_img::planes(im.pixfmt) && e == hipSuccess; p++) {
        const size_t rb = rife_img::row_bytes(im.w, im.pixfmt, p);
        e = hipMemcpy2DAsync(im.plane[p], (size_t)im.pitch[p], static_cast<const uint8_t*>(tight) + image_tight_offset(im.w, im.h, im.pixfmt, p), rb, rb, (size_t)rife_img::plane_rows(im.h, im.pixfmt, p), kind, st);
    }
    return e;
}
// canonical samples (timestep 0 / 1; canon10_host states the same for tight frames), row by row; the modes are planes.h CanonMode
static void image_canon_host(const rife_hip_image_t& out, const rife_hip_image_t& in) {
    const CanonMode mode = canon_mode(in.pixfmt);
    for (int p = 0; p < rife_img::planes(in.pixfmt); p++) {
        const size_t rb = rife_img::row_bytes(in.w, in.pixfmt, p);
        for (int y = 0; y < rife_img::plane_rows(in.h, in.pixfmt, p); y++) {
            const uint8_t* s = static_cast<const uint8_t*>(in.plane[p]) + (size_t)y * in.pitch[p];
            uint8_t* d = static_cast<uint8_t*>(out.plane[p]) + (size_t)y * out.pitch[p];
            canon_row_host(mode, s, d, rb);
        }
    }
}
// the same on device planes: strided forms of the canonical copies; 2-D copies where the bytes pass unchanged
static int image_canon_device(hipStream_t st, const rife_hip_image_t& in, const rife_hip_image_t& out) {
    const CanonMode mode = canon_mode(in.pixfmt);
    for (int p = 0; p < rife_img::planes(in.pixfmt); p++) {
        const size_t rb = rife_img::row_bytes(in.w, in.pixfmt, p);
        const int rows = rife_img::plane_rows(in.h, in.pixfmt, p);
        const uint8_t* s = static_cast<const uint8_t*>(in.plane[p]); uint8_t* d = static_cast<uint8_t*>(out.plane[p]);
        const size_t sp = (size_t)in.pitch[p], dp = (size_t)out.pitch[p];
        if (mode == CANON_BYTES) { HIPCHK(hipMemcpy2DAsync(d, dp, s, sp, rb, (size_t)rows, hipMemcpyDeviceToDevice, st)); continue; }
        launch_canon_rows(st, mode, s, sp, d, dp, rb, rows);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static int rife_hip_process_image_impl(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out) {
    int rc;
    if ((rc = image_precheck({in0, in1, out}))) return rc;
    const int w = in0->w, h = in0->h, pixfmt = in0->pixfmt;
    if (rife_img::is_tight(in0) && rife_img::is_tight(in1) && rife_img::is_tight(out))      // the _px call itself (RGB8: every family and mode)
        return rife_hip_process_impl(E, static_cast<const uint8_t*>(in0->plane[0]), static_cast<const uint8_t*>(in1->plane[0]), w, h, timestep, static_cast<uint8_t*>(out->plane[0]), pixfmt);
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = image_supported(E))) return rc;
    if (timestep == 0.f || timestep == 1.f) { image_canon_host(*out, timestep == 0.f ? *in0 : *in1); return 0; }
    if ((rc = check_device(E->gpuid))) return rc;
    return with_leased_ctx(E, w, h, pixfmt, [&](Ctx& c) {
        int rc = upload_with_token(E, c.stream, [&] {
            const hipError_t e = image_copy_to_tight(c.d_in0, *in0, hipMemcpyHostToDevice, c.stream);
            return e != hipSuccess ? e : image_copy_to_tight(c.d_in1, *in1, hipMemcpyHostToDevice, c.stream);
        });
        if (!rc) rc = run_v4_replay(*E, c, c.d_in0, c.d_in1, timestep, c.d_out);
        hipError_t e;
        if (!rc && (e = image_copy_from_tight(*out, c.d_out, hipMemcpyDeviceToHost, c.stream)) != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
        return rc;
    });
}

static int rife_hip_frame_upload_image_impl(const rife_hip_t* E, const rife_hip_image_t* img, rife_hip_frame_t** frame) {
    if (frame) *frame = nullptr;
    if (!frame) return fail(RIFE_HIP_EINVAL, "null argument");
    int rc;
    if ((rc = image_precheck({img}))) return rc;
    if (rife_img::is_tight(img)) return rife_hip_frame_upload_impl(E, static_cast<const uint8_t*>(img->plane[0]), img->w, img->h, frame, img->pixfmt);
    if (!E) return fail(RIFE_HIP_EINVAL, "null argument");
    if ((rc = image_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    std::unique_ptr<rife_hip_frame> f(new rife_hip_frame);
    f->w = img->w; f->h = img->h; f->gpuid = E->gpuid; f->pixfmt = img->pixfmt;
    const size_t nbytes = frame_bytes(img->w, img->h, img->pixfmt);
    f->nbytes = nbytes; f->pool = E->frame_pool;
    if (!(f->d = f->pool->take(nbytes))) return fail(RIFE_HIP_EHIP, "hipMalloc of a resident frame failed");
    // a copy on its own stream, drained here (rife_hip_frame_upload_impl)
    const hipError_t e = CopyStreamLease(E).run([&](hipStream_t st) { return image_copy_to_tight(f->d, *img, hipMemcpyHostToDevice, st); });
    if (e != hipSuccess) { f->pool->give(f->d, nbytes); return fail(RIFE_HIP_EHIP, std::string("frame upload: ") + hipGetErrorString(e)); }
    *frame = f.release();
    return 0;
}

static int rife_hip_process_frames_image_impl(const rife_hip_t* E, const rife_hip_frame_t* f0, const rife_hip_frame_t* f1, float timestep, const rife_hip_image_t* out) {
    int rc;
    if ((rc = image_precheck({out}))) return rc;
    if (!f0 || !f1) return fail(RIFE_HIP_EINVAL, "null frame pointer");
    if (f0->w != f1->w || f0->h != f1->h) return fail(RIFE_HIP_EINVAL, "the two frames differ in size");
    if (f0->pixfmt != f1->pixfmt) return fail(RIFE_HIP_EINVAL, "the two frames differ in pixel format or colour description");
    if (out->w != f0->w || out->h != f0->h) return fail(RIFE_HIP_EINVAL, "the output image and the frames differ in size");
    if (out->pixfmt != f0->pixfmt) return fail(RIFE_HIP_EINVAL, "the output image and the frames differ in pixel format or colour description");
    if (rife_img::is_tight(out)) return rife_hip_process_frames_impl(E, f0, f1, timestep, static_cast<uint8_t*>(out->plane[0]));
    const int w = f0->w, h = f0->h, pixfmt = f0->pixfmt;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (f0->gpuid != E->gpuid || f1->gpuid != E->gpuid) return fail(RIFE_HIP_EINVAL, "frame was uploaded to another device");
    if ((rc = image_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    if (timestep == 0.f || timestep == 1.f) {      // a copy stream of the pool, never the legacy stream; canonical form on the host, in place
        const hipError_t e = CopyStreamLease(E).run([&](hipStream_t st) { return image_copy_from_tight(*out, timestep == 0.f ? f0->d : f1->d, hipMemcpyDeviceToHost, st); });
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("frame download: ") + hipGetErrorString(e));
        image_canon_host(*out, *out);
        return 0;
    }
    return with_leased_ctx(E, w, h, pixfmt, [&](Ctx& c) {
        int rc = run_v4_replay(*E, c, f0->d, f1->d, timestep, c.d_out);
        if (!rc && image_copy_from_tight(*out, c.d_out, hipMemcpyDeviceToHost, c.stream) != hipSuccess) rc = fail(RIFE_HIP_EHIP, "D2H failed");
        return rc;
    });
}

static int rife_hip_process_device_image_impl(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, void* hip_stream) {
    int rc;
    if ((rc = image_precheck({in0, in1, out}))) return rc;
    const int w = in0->w, h = in0->h, pixfmt = in0->pixfmt;
    if (rife_img::is_tight(in0) && rife_img::is_tight(in1) && rife_img::is_tight(out))      // the _px call itself (RGB8: every family and mode)
        return rife_hip_process_device_impl(E, in0->plane[0], in1->plane[0], w, h, timestep, out->plane[0], hip_stream, pixfmt);
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = image_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    StreamWorkspace ws(E, hip_stream);
    if (ws.rc) return ws.rc;
    Ctx* const c = ws.c;
    if (timestep == 0.f || timestep == 1.f) {
        if ((rc = image_canon_device(c->stream, timestep == 0.f ? *in0 : *in1, *out))) return rc;
    } else {
        if ((rc = ensure_ctx(*c, w, h, pixfmt, E->pad()))) return rc;
        const PlaneIO pio{plane_set(*in0), plane_set(*in1), plane_set(*out)};
        rc = run_v4(*E, *c, nullptr, nullptr, timestep, c->d_out, nullptr, &pio);      // YUV and planar RGB: the pitched post-processing kernel writes the caller's planes; packed RGB formats: the tight frame c->d_out
        if (rc) return rc;
        if (!pix_conv(pixfmt)) {
            Timed t(E->prof, "store_rows", 0, c->stream);
            launch_store_rows(c->stream, c->d_out, rife_img::row_bytes(w, pixfmt, 0), h, static_cast<uint8_t*>(out->plane[0]), (size_t)out->pitch[0], rife_img::elem_size(pixfmt));
            HIPCHK(hipGetLastError());
        }
    }
    if (!hip_stream) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int rife_hip_image_check(const rife_hip_image_t* img) {
    std::string err;
    return rife_img::check(img, err) ? fail(RIFE_HIP_EINVAL, "image: " + err) : 0;
}
size_t rife_hip_image_row_bytes(int w, int pixfmt, int plane) { return rife_img::row_bytes(w, pixfmt, plane); }

int rife_hip_process_image(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out) {
    return guarded("rife_hip_process_image", [&] { return rife_hip_process_image_impl(E, in0, in1, timestep, out); });
}
int rife_hip_process_device_image(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, void* hip_stream) {
    return guarded("rife_hip_process_device_image", [&] { return rife_hip_process_device_image_impl(E, in0, in1, timestep, out, hip_stream); });
}
int rife_hip_frame_upload_image(const rife_hip_t* E, const rife_hip_image_t* img, rife_hip_frame_t** frame) {
    return guarded("rife_hip_frame_upload_image", [&] { return rife_hip_frame_upload_image_impl(E, img, frame); });
}
int rife_hip_process_frames_image(const rife_hip_t* E, const rife_hip_frame_t* f0, const rife_hip_frame_t* f1, float timestep, const rife_hip_image_t* out) {
    return guarded("rife_hip_process_frames_image", [&] { return rife_hip_process_frames_image_impl(E, f0, f1, timestep, out); });
}

#ifdef RIFE_HIP_TEST_BUILD
// ---- the pitched kernels alone (include/rife_hip_test.h) ----
// every plane's span (first byte of its first row .. last byte of its last row, gaps included) in ONE device allocation, at the host pointer's alignment modulo 16
struct ImageMirror {
    uint8_t* d = nullptr;
    size_t off[3] = {0, 0, 0}, span[3] = {0, 0, 0};
    std::vector<uint8_t> sent[3];
    rife_hip_image_t dev;
    ~ImageMirror() { if (d) (void)hipFree(d); }
    hipError_t upload(const rife_hip_image_t& im) {
        size_t cur = 0;
        const int np = rife_img::planes(im.pixfmt);
        for (int p = 0; p < np; p++) {
            span[p] = (size_t)(rife_img::plane_rows(im.h, im.pixfmt, p) - 1) * (size_t)im.pitch[p] + rife_img::row_bytes(im.w, im.pixfmt, p);
            off[p] = align_up(cur, 16) + (reinterpret_cast<uintptr_t>(im.plane[p]) & 15);
            cur = off[p] + span[p];
        }
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), cur + 16);
        dev = im;
        for (int p = 0; p < np && e == hipSuccess; p++) {
            sent[p].assign(static_cast<const uint8_t*>(im.plane[p]), static_cast<const uint8_t*>(im.plane[p]) + span[p]);
            dev.plane[p] = d + off[p];
            e = hipMemcpy(d + off[p], sent[p].data(), span[p], hipMemcpyHostToDevice);
        }
        return e;
    }
    // rows come back as they are; a gap byte comes back only if the device changed it (two planes of the caller may share rows of one buffer)
    hipError_t download(const rife_hip_image_t& im) {
        hipError_t e = hipSuccess;
        for (int p = 0; p < rife_img::planes(im.pixfmt) && e == hipSuccess; p++) {
            std::vector<uint8_t> got(span[p]);
            if ((e = hipMemcpy(got.data(), d + off[p], span[p], hipMemcpyDeviceToHost)) != hipSuccess) break;
            const size_t rb = rife_img::row_bytes(im.w, im.pixfmt, p), pitch = (size_t)im.pitch[p];
            uint8_t* host = static_cast<uint8_t*>(im.plane[p]);
            for (size_t i = 0; i < span[p]; i++) if (i % pitch < rb || got[i] != sent[p][i]) host[i] = got[i];
        }
        return e;
    }
};
int rife_hip_op_image_to_resident(int gpuid, const rife_hip_image_t* img, int force_scalar, uint32_t* out_padded) {
    int rc;
    if ((rc = rife_hip_image_check(img))) return rc;
    if (!out_padded || force_scalar < 0 || force_scalar > 2) return fail(RIFE_HIP_EINVAL, "op_image_to_resident: an output array and force_scalar 0, 1 or 2");
    if (force_scalar == 2 && !rife_img::is_tight(img)) return fail(RIFE_HIP_EINVAL, "op_image_to_resident: the tight kernels take a tight image");
    if ((rc = check_device(gpuid))) return rc;
    const int w = img->w, h = img->h;
    ImageMirror m;
    uint8_t* d_t = nullptr;                                                  // force_scalar == 2: the tight frame in ONE piece (the tight kernels find the chroma planes by arithmetic), at the host pointer's alignment modulo 16
    const size_t ntight = frame_bytes(w, h, img->pixfmt), toff = reinterpret_cast<uintptr_t>(img->plane[0]) & 15;
    hipError_t e = force_scalar == 2 ? hipMalloc(reinterpret_cast<void**>(&d_t), ntight + 16) : m.upload(*img);
    if (e == hipSuccess && force_scalar == 2) e = hipMemcpy(d_t + toff, img->plane[0], ntight, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = op_padded_rgb10(w, h, out_padded, [&](uint32_t* d_o, int wp, int hp) {
        if (force_scalar == 2) launch_preproc(0, d_t + toff, w, h, d_o, wp, hp, img->pixfmt);
        else launch_preproc_planes(0, plane_set(m.dev), w, h, d_o, wp, hp, img->pixfmt, force_scalar == 1);
    });
    (void)hipFree(d_t);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_image_to_resident: ") + hipGetErrorString(e));
    return 0;
}
int rife_hip_op_resident_to_image(int gpuid, const uint32_t* tight_frame, const rife_hip_image_t* img, int force_scalar) {
    int rc;
    if ((rc = rife_hip_image_check(img))) return rc;
    if (!tight_frame || force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_resident_to_image: a tight frame and force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    const int w = img->w, h = img->h;
    const bool yuv = pix_conv(img->pixfmt);      // YUV and planar RGB: converted from an A2B10G10R10 frame
    const size_t nin = yuv ? (size_t)w * h * 4 : frame_bytes(w, h, img->pixfmt);
    ImageMirror m;
    void* d_i = nullptr;
    hipError_t e = m.upload(*img);
    if (e == hipSuccess) e = hipMalloc(&d_i, nin);
    if (e == hipSuccess) e = hipMemcpy(d_i, tight_frame, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (yuv) launch_postproc_yuv_planes(0, static_cast<const uint32_t*>(d_i), w, h, plane_set(m.dev), img->pixfmt, force_scalar == 1);
        else launch_store_rows(0, static_cast<const uint8_t*>(d_i), rife_img::row_bytes(w, img->pixfmt, 0), h, static_cast<uint8_t*>(m.dev.plane[0]), (size_t)img->pitch[0],
                               rife_img::elem_size(img->pixfmt), force_scalar == 1);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = m.download(*img);
    }
    (void)hipFree(d_i);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_resident_to_image: ") + hipGetErrorString(e));
    return 0;
}
#endif  // RIFE_HIP_TEST_BUILD

}  // extern "C"
