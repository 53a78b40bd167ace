// engine_hbd_packed.h: the packed 16-bit entry points of include/rife_hip.h ("16-bit packed RGB and RGBA": rife_hip_packed_t) on top of engine_hbd.h
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
// A packed call IS the combined sets call on the RGBP10 proxy of the colour channels with ONE set of `channels` planes at shift (0, 0), edge semantics - except that
// neither the proxy nor the planes exist: k_preproc_packed (hbd_packed.h) reduces the caller's interleaved samples on their way into the resident frames, the pass
// leaves its motion in the workspace, and ONE launch of k_apply_packed blends all channels of the packed frames.
//   process_device_hbd_packed   the stream's workspace (StreamWorkspace); pre-processing, pass and blend on the caller's device frames, in place
//   process_hbd_packed          a pool workspace (with_leased_ctx); host frames staged ONCE, 2 bytes per sample, tight, in its apply staging (apply_staging); the result comes back with one
//                               2-D copy
// The rules and their words: csrc/packed_check.h.

// 0, or -RIFE_HIP_EINVAL; then "no HIP device at all" (-RIFE_HIP_ENODEV) before anything looks at the engine
static int packed_precheck(const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, const rife_hip_packed_t* out) {
    std::string err;
    if (rife_packed::check_call(in0, in1, out, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    return no_hip_device();
}
static int packed_supported(const rife_hip* E) { return plain_v46_only(E, "high bit depth packed frames are"); }
// what k_apply_packed gets, for frames and motion in DEVICE memory: plane 0 of ApplyArgs holds the packed frames, the extent is the frame (edge semantics)
static ApplyArgs packed_args(const rife_hip_packed_t& p0, const rife_hip_packed_t& p1, const rife_hip_packed_t& out, const uint8_t* flow, size_t flow_pitch,
                             const uint8_t* mask, size_t mask_pitch, int format) {
    ApplyArgs a{};
    a.p0[0] = static_cast<const uint8_t*>(p0.data); a.p1[0] = static_cast<const uint8_t*>(p1.data); a.out[0] = static_cast<uint8_t*>(out.data);
    a.pitch0[0] = (unsigned)p0.pitch; a.pitch1[0] = (unsigned)p1.pitch; a.pitcho[0] = (unsigned)out.pitch;
    a.flow = flow; a.mask = mask; a.flow_pitch = (unsigned)flow_pitch; a.mask_pitch = (unsigned)mask_pitch; a.format = format;
    a.w = p0.w; a.h = p0.h; a.wp = p0.w; a.hp = p0.h; a.n = p0.channels; a.maxval = (1 << p0.depth) - 1;
    return a;
}
// `prof`: null in the single-kernel test call; *vec tells that call which form ran
static int packed_apply_launch(Profiler* prof, hipStream_t st, const ApplyArgs& a, int channels, bool force_scalar = false, bool* vec = nullptr) {
    {
        std::optional<Timed> t;
        if (prof) t.emplace(*prof, "apply_packed", 0, st);
        const bool v = launch_apply_packed(st, a, channels, force_scalar);
        if (vec) *vec = v;
    }
    HIPCHK(hipGetLastError());
    return 0;
}
static HbdIO packed_io(const rife_hip_packed_t& in0, const rife_hip_packed_t& in1) {
    HbdIO io{};
    io.in0.p[0] = static_cast<uint8_t*>(in0.data); io.in0.pitch[0] = (size_t)in0.pitch;
    io.in1.p[0] = static_cast<uint8_t*>(in1.data); io.in1.pitch[0] = (size_t)in1.pitch;
    io.depth = in0.depth; io.packed = in0.channels;
    return io;
}

static int rife_hip_process_hbd_packed_impl(const rife_hip_t* E, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out) {
    int rc;
    const int w = in0->w, h = in0->h;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = packed_supported(E))) return rc;
    if (timestep == 0.f || timestep == 1.f) {                             // no pass, no arithmetic: the samples of frame 0 / frame 1, clamped to maxval
        apply_copy_host(rife_packed::as_plane(timestep == 0.f ? *in0 : *in1), rife_packed::as_plane(*out));
        return 0;
    }
    if ((rc = check_device(E->gpuid))) return rc;
    return with_leased_ctx(E, w, h, RIFE_HIP_PIX_RGBP10, [&](Ctx& C) {
        MotionArgs mo;
        int rc = apply_motion_stage(C, mo);
        const size_t rb = (size_t)w * in0->channels * 2, frame = align_up((size_t)h * rb, 16);
        if (!rc) rc = apply_staging(C, 3 * frame);
        if (rc) return rc;
        rife_hip_packed_t d0 = *in0, d1 = *in1, dout = *out;              // the tight device copies
        d0.data = C.ap_planes; d1.data = C.ap_planes + frame; dout.data = C.ap_planes + 2 * frame;
        d0.pitch = d1.pitch = dout.pitch = (ptrdiff_t)rb;
        rc = upload_with_token(E, C.stream, [&] {
            const hipError_t e = hipMemcpy2DAsync(d0.data, rb, in0->data, (size_t)in0->pitch, rb, (size_t)h, hipMemcpyHostToDevice, C.stream);
            return e != hipSuccess ? e : hipMemcpy2DAsync(d1.data, rb, in1->data, (size_t)in1->pitch, rb, (size_t)h, hipMemcpyHostToDevice, C.stream);
        });
        const HbdIO io = packed_io(d0, d1);
        if (!rc) rc = run_v4(*E, C, nullptr, nullptr, timestep, nullptr, nullptr, nullptr, &mo, &io);
        if (!rc) rc = packed_apply_launch(&E->prof, C.stream, packed_args(d0, d1, dout, mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32), in0->channels);
        hipError_t e;
        if (!rc && (e = hipMemcpy2DAsync(out->data, (size_t)out->pitch, dout.data, rb, rb, (size_t)h, hipMemcpyDeviceToHost, C.stream)) != hipSuccess)
            rc = fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
        return rc;
    });
}

static int rife_hip_process_device_hbd_packed_impl(const rife_hip_t* E, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out,
                                                   void* hip_stream) {
    int rc;
    const int w = in0->w, h = in0->h;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = packed_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    StreamWorkspace ws(E, hip_stream);
    if (ws.rc) return ws.rc;
    Ctx* const c = ws.c;
    if (timestep == 0.f || timestep == 1.f) {
        if ((rc = apply_copy_device(c->stream, rife_packed::as_plane(timestep == 0.f ? *in0 : *in1), rife_packed::as_plane(*out)))) return rc;
    } else {
        MotionArgs mo;
        if ((rc = ensure_ctx(*c, w, h, RIFE_HIP_PIX_RGBP10, E->pad()))) return rc;
        if ((rc = apply_motion_stage(*c, mo))) return rc;
        const HbdIO io = packed_io(*in0, *in1);
        if ((rc = run_v4(*E, *c, nullptr, nullptr, timestep, nullptr, nullptr, nullptr, &mo, &io))) return rc;
        if ((rc = packed_apply_launch(&E->prof, c->stream, packed_args(*in0, *in1, *out, mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32), in0->channels))) return rc;
    }
    if (!hip_stream) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int rife_hip_packed_check(const rife_hip_packed_t* img) {
    std::string err;
    return rife_packed::check(img, err) ? fail(RIFE_HIP_EINVAL, "high bit depth: " + err) : 0;
}
int rife_hip_process_hbd_packed(const rife_hip_t* E, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out) {
    int rc;
    if ((rc = packed_precheck(in0, in1, out))) return rc;
    return guarded("rife_hip_process_hbd_packed", [&] { return rife_hip_process_hbd_packed_impl(E, in0, in1, timestep, out); });
}
int rife_hip_process_device_hbd_packed(const rife_hip_t* E, const rife_hip_packed_t* in0, const rife_hip_packed_t* in1, float timestep, const rife_hip_packed_t* out,
                                       void* hip_stream) {
    int rc;
    if ((rc = packed_precheck(in0, in1, out))) return rc;
    return guarded("rife_hip_process_device_hbd_packed", [&] { return rife_hip_process_device_hbd_packed_impl(E, in0, in1, timestep, out, hip_stream); });
}

#ifdef RIFE_HIP_TEST_BUILD
// ---- the packed pre-processing kernel alone (include/rife_hip_test.h): uploaded as rife_hip_op_apply uploads (ApplyMirror: pitch and pointer alignment kept) ----
int rife_hip_op_packed_to_rgb10(int gpuid, const rife_hip_packed_t* img, uint32_t* out_padded, int force_scalar) {
    int rc;
    if ((rc = rife_hip_packed_check(img))) return rc;
    if (!out_padded || force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_packed_to_rgb10: an output array and force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_packed_to_rgb10", [&] {
        const int w = img->w, h = img->h;
        ApplyMirror m;
        bool vec = false;
        hipError_t e = m.upload(img->data, (size_t)img->pitch, (size_t)w * img->channels * 2, h);
        if (e == hipSuccess) e = op_padded_rgb10(w, h, out_padded, [&](uint32_t* d_o, int wp, int hp) {
            vec = launch_preproc_packed(0, m.dev, (size_t)img->pitch, img->channels, w, h, d_o, wp, hp, img->depth, force_scalar == 1);
        });
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_packed_to_rgb10: ") + hipGetErrorString(e));
        return vec ? 1 : 0;
    });
}
// ---- the packed blend alone (include/rife_hip_test.h): uploaded as rife_hip_op_apply uploads ----
int rife_hip_op_apply_packed(int gpuid, const rife_hip_packed_t* p0, const rife_hip_packed_t* p1, const rife_hip_packed_t* out, const rife_hip_motion_t* hm, int force_scalar) {
    int rc;
    std::string err;
    if (rife_packed::check_call(p0, p1, out, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    if (rife_apply::check_sets_motion(hm, p0->w, p0->h, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    if (force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_apply_packed: force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_apply_packed", [&] {
        const int w = p0->w, h = p0->h;
        const size_t rb = (size_t)w * p0->channels * 2;
        ApplyMirror m0, m1, mo;
        MotionMirror mm;
        rife_hip_packed_t d0 = *p0, d1 = *p1, dout = *out;
        hipError_t e = m0.upload(p0->data, (size_t)p0->pitch, rb, h); d0.data = m0.dev;
        if (e == hipSuccess) { e = m1.upload(p1->data, (size_t)p1->pitch, rb, h); d1.data = m1.dev; }
        if (e == hipSuccess) { e = mo.upload(out->data, (size_t)out->pitch, rb, h); dout.data = mo.dev; }
        if (e == hipSuccess) e = mm.upload(*hm, w, h);
        int lrc = 0;
        bool vec = false;
        if (e == hipSuccess) e = op_on_own_stream(lrc, [&](hipStream_t st) {
            return packed_apply_launch(nullptr, st, packed_args(d0, d1, dout, mm.flow.dev, hm->flow_pitch, mm.mask.dev, hm->mask_pitch, hm->format), p0->channels, force_scalar == 1, &vec);
        });
        if (lrc) return lrc;
        if (e == hipSuccess) e = mo.download(out->data, (size_t)out->pitch, rb);
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_apply_packed: ") + hipGetErrorString(e));
        return vec ? 1 : 0;
    });
}
#endif  // RIFE_HIP_TEST_BUILD

}  // extern "C"
