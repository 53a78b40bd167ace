// engine_hbd_semiplanar.h: the semi-planar entry points of include/rife_hip.h ("semi-planar high bit depth": rife_hip_semiplanar_t) on top of engine_hbd.h
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
// A semi-planar call IS the hbd call on split(img) - the planes Y >> s, Cb >> s, Cr >> s of layout I420P10 | csp / I422P10 | csp - joined back and shifted left,
// except that the planes never exist: k_preproc_sp (hbd_semiplanar.h) shifts and reduces the caller's samples on their way into the resident frames, the pass leaves its
// motion in the workspace, and ONE launch of k_apply_sp blends the luma plane and the interleaved chroma plane.
//   process_device_hbd_semiplanar   the stream's workspace (StreamWorkspace); pre-processing, pass and blend on the caller's device planes, in place
//   process_hbd_semiplanar          a pool workspace (with_leased_ctx); host planes staged ONCE, 2 bytes per sample, tight, in its apply staging (apply_staging); the result comes back with
//                                   two 2-D copies
// The rules and their words: csrc/semiplanar_check.h.

// 0, or -RIFE_HIP_EINVAL; then "no HIP device at all" (-RIFE_HIP_ENODEV) before anything looks at the engine
static int sp_precheck(const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, const rife_hip_semiplanar_t* out) {
    std::string err;
    if (rife_sp::check_call(in0, in1, out, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    return no_hip_device();
}
static int sp_supported(const rife_hip* E) { return plain_v46_only(E, "high bit depth semi-planar surfaces are"); }
// what k_apply_sp gets, for surfaces and motion in DEVICE memory: the luma set and the chroma set of the hbd call (edge semantics: extent = the plane) on one motion
static ApplySpArgs sp_args(const rife_hip_semiplanar_t& p0, const rife_hip_semiplanar_t& p1, const rife_hip_semiplanar_t& out, const uint8_t* flow, size_t flow_pitch,
                           const uint8_t* mask, size_t mask_pitch, int format) {
    ApplySpArgs s{};
    ApplyArgs* const two[2] = {&s.y, &s.c.a};
    for (int i = 0; i < 2; i++) {
        ApplyArgs& a = *two[i];
        a.p0[0] = static_cast<const uint8_t*>(i ? p0.cbcr : p0.y); a.p1[0] = static_cast<const uint8_t*>(i ? p1.cbcr : p1.y); a.out[0] = static_cast<uint8_t*>(i ? out.cbcr : out.y);
        a.pitch0[0] = (unsigned)(i ? p0.pitch_c : p0.pitch_y); a.pitch1[0] = (unsigned)(i ? p1.pitch_c : p1.pitch_y); a.pitcho[0] = (unsigned)(i ? out.pitch_c : out.pitch_y);
        a.flow = flow; a.mask = mask; a.flow_pitch = (unsigned)flow_pitch; a.mask_pitch = (unsigned)mask_pitch; a.format = format;
        a.w = i ? rife_sp::chroma_w(p0.w) : p0.w; a.h = i ? rife_sp::chroma_h(p0.h, p0.chroma) : p0.h; a.wp = a.w; a.hp = a.h;
        a.n = i ? 2 : 1; a.maxval = (1 << p0.depth) - 1;
    }
    s.c.mw = p0.w; s.c.mh = p0.h;
    s.sh = 16 - p0.depth;
    return s;
}
// `prof`: null in the single-kernel test call; *vec tells that call which form ran
static int sp_apply_launch(Profiler* prof, hipStream_t st, const ApplySpArgs& s, int chroma, bool force_scalar = false, bool* vec = nullptr) {
    {
        std::optional<Timed> t;
        if (prof) t.emplace(*prof, "apply_sp", 0, st);
        const bool v = launch_apply_sp(st, s, chroma == 1, force_scalar);
        if (vec) *vec = v;
    }
    HIPCHK(hipGetLastError());
    return 0;
}
static HbdIO sp_io(const rife_hip_semiplanar_t& in0, const rife_hip_semiplanar_t& in1) {
    HbdIO io{};
    io.in0.p[0] = static_cast<uint8_t*>(in0.y); io.in0.pitch[0] = (size_t)in0.pitch_y; io.in0.p[1] = static_cast<uint8_t*>(in0.cbcr); io.in0.pitch[1] = (size_t)in0.pitch_c;
    io.in1.p[0] = static_cast<uint8_t*>(in1.y); io.in1.pitch[0] = (size_t)in1.pitch_y; io.in1.p[1] = static_cast<uint8_t*>(in1.cbcr); io.in1.pitch[1] = (size_t)in1.pitch_c;
    io.depth = in0.depth; io.semiplanar = 1;
    return io;
}
// timestep 0 / 1: (v >> s) << s of every sample of both planes
static void sp_copy_host(const rife_hip_semiplanar_t& src, const rife_hip_semiplanar_t& out) {
    const int sh = 16 - src.depth, n[2] = {src.w, 2 * rife_sp::chroma_w(src.w)}, rows[2] = {src.h, rife_sp::chroma_h(src.h, src.chroma)};
    for (int p = 0; p < 2; p++)
        for (int y = 0; y < rows[p]; y++) {
            const uint16_t* s = reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(p ? src.cbcr : src.y) + (size_t)y * (p ? src.pitch_c : src.pitch_y));
            uint16_t* d = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(p ? out.cbcr : out.y) + (size_t)y * (p ? out.pitch_c : out.pitch_y));
            for (int x = 0; x < n[p]; x++) d[x] = (uint16_t)((s[x] >> sh) << sh);
        }
}
static int sp_copy_device(hipStream_t st, const rife_hip_semiplanar_t& src, const rife_hip_semiplanar_t& out) {
    launch_copy_sp(st, static_cast<const uint8_t*>(src.y), (size_t)src.pitch_y, static_cast<uint8_t*>(out.y), (size_t)out.pitch_y, src.w, src.h, src.depth);
    launch_copy_sp(st, static_cast<const uint8_t*>(src.cbcr), (size_t)src.pitch_c, static_cast<uint8_t*>(out.cbcr), (size_t)out.pitch_c, 2 * rife_sp::chroma_w(src.w),
                   rife_sp::chroma_h(src.h, src.chroma), src.depth);
    HIPCHK(hipGetLastError());
    return 0;
}

static int rife_hip_process_hbd_semiplanar_impl(const rife_hip_t* E, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep,
                                                const rife_hip_semiplanar_t* out) {
    int rc;
    const int w = in0->w, h = in0->h;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = sp_supported(E))) return rc;
    if (timestep == 0.f || timestep == 1.f) {                             // no pass, no arithmetic but the shifts
        sp_copy_host(timestep == 0.f ? *in0 : *in1, *out);
        return 0;
    }
    if ((rc = check_device(E->gpuid))) return rc;
    return with_leased_ctx(E, w, h, rife_sp::planar_pixfmt(in0->chroma, in0->csp), [&](Ctx& C) {
        MotionArgs mo;
        int rc = apply_motion_stage(C, mo);
        const int ch = rife_sp::chroma_h(h, in0->chroma);
        const size_t rby = (size_t)w * 2, rbc = (size_t)rife_sp::chroma_w(w) * 4;
        const size_t ly = align_up((size_t)h * rby, 16), lc = align_up((size_t)ch * rbc, 16);
        if (!rc) rc = apply_staging(C, 3 * (ly + lc));
        if (rc) return rc;
        rife_hip_semiplanar_t d[3] = {*in0, *in1, *out};                  // the tight device copies
        for (int i = 0; i < 3; i++) { d[i].y = C.ap_planes + i * (ly + lc); d[i].cbcr = C.ap_planes + i * (ly + lc) + ly; d[i].pitch_y = (ptrdiff_t)rby; d[i].pitch_c = (ptrdiff_t)rbc; }
        rc = upload_with_token(E, C.stream, [&] {
            const rife_hip_semiplanar_t* src[2] = {in0, in1};
            hipError_t e = hipSuccess;
            for (int i = 0; i < 2 && e == hipSuccess; i++) {
                e = hipMemcpy2DAsync(d[i].y, rby, src[i]->y, (size_t)src[i]->pitch_y, rby, (size_t)h, hipMemcpyHostToDevice, C.stream);
                if (e == hipSuccess) e = hipMemcpy2DAsync(d[i].cbcr, rbc, src[i]->cbcr, (size_t)src[i]->pitch_c, rbc, (size_t)ch, hipMemcpyHostToDevice, C.stream);
            }
            return e;
        });
        const HbdIO io = sp_io(d[0], d[1]);
        if (!rc) rc = run_v4(*E, C, nullptr, nullptr, timestep, nullptr, nullptr, nullptr, &mo, &io);
        if (!rc) rc = sp_apply_launch(&E->prof, C.stream, sp_args(d[0], d[1], d[2], mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32), in0->chroma);
        if (!rc) {
            hipError_t e = hipMemcpy2DAsync(out->y, (size_t)out->pitch_y, d[2].y, rby, rby, (size_t)h, hipMemcpyDeviceToHost, C.stream);
            if (e == hipSuccess) e = hipMemcpy2DAsync(out->cbcr, (size_t)out->pitch_c, d[2].cbcr, rbc, rbc, (size_t)ch, hipMemcpyDeviceToHost, C.stream);
            if (e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
        }
        return rc;
    });
}

static int rife_hip_process_device_hbd_semiplanar_impl(const rife_hip_t* E, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep,
                                                       const rife_hip_semiplanar_t* out, void* hip_stream) {
    int rc;
    const int w = in0->w, h = in0->h;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = sp_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    StreamWorkspace ws(E, hip_stream);
    if (ws.rc) return ws.rc;
    Ctx* const c = ws.c;
    if (timestep == 0.f || timestep == 1.f) {
        if ((rc = sp_copy_device(c->stream, timestep == 0.f ? *in0 : *in1, *out))) return rc;
    } else {
        MotionArgs mo;
        if ((rc = ensure_ctx(*c, w, h, rife_sp::planar_pixfmt(in0->chroma, in0->csp), E->pad()))) return rc;
        if ((rc = apply_motion_stage(*c, mo))) return rc;
        const HbdIO io = sp_io(*in0, *in1);
        if ((rc = run_v4(*E, *c, nullptr, nullptr, timestep, nullptr, nullptr, nullptr, &mo, &io))) return rc;
        if ((rc = sp_apply_launch(&E->prof, c->stream, sp_args(*in0, *in1, *out, mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32), in0->chroma))) return rc;
    }
    if (!hip_stream) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int rife_hip_semiplanar_check(const rife_hip_semiplanar_t* img) {
    std::string err;
    return rife_sp::check(img, err) ? fail(RIFE_HIP_EINVAL, "high bit depth: " + err) : 0;
}
int rife_hip_process_hbd_semiplanar(const rife_hip_t* E, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep, const rife_hip_semiplanar_t* out) {
    int rc;
    if ((rc = sp_precheck(in0, in1, out))) return rc;
    return guarded("rife_hip_process_hbd_semiplanar", [&] { return rife_hip_process_hbd_semiplanar_impl(E, in0, in1, timestep, out); });
}
int rife_hip_process_device_hbd_semiplanar(const rife_hip_t* E, const rife_hip_semiplanar_t* in0, const rife_hip_semiplanar_t* in1, float timestep,
                                           const rife_hip_semiplanar_t* out, void* hip_stream) {
    int rc;
    if ((rc = sp_precheck(in0, in1, out))) return rc;
    return guarded("rife_hip_process_device_hbd_semiplanar", [&] { return rife_hip_process_device_hbd_semiplanar_impl(E, in0, in1, timestep, out, hip_stream); });
}

#ifdef RIFE_HIP_TEST_BUILD
// ---- the semi-planar pre-processing kernel alone (include/rife_hip_test.h): both planes uploaded as rife_hip_op_apply uploads (ApplyMirror: pitch and pointer alignment kept) ----
int rife_hip_op_sp_to_rgb10(int gpuid, const rife_hip_semiplanar_t* img, uint32_t* out_padded, int force_scalar) {
    int rc;
    if ((rc = rife_hip_semiplanar_check(img))) return rc;
    if (!out_padded || force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_sp_to_rgb10: an output array and force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_sp_to_rgb10", [&] {
        const int w = img->w, h = img->h;
        ApplyMirror my, mc;
        bool vec = false;
        hipError_t e = my.upload(img->y, (size_t)img->pitch_y, (size_t)w * 2, h);
        if (e == hipSuccess) e = mc.upload(img->cbcr, (size_t)img->pitch_c, (size_t)rife_sp::chroma_w(w) * 4, rife_sp::chroma_h(h, img->chroma));
        if (e == hipSuccess) e = op_padded_rgb10(w, h, out_padded, [&](uint32_t* d_o, int wp, int hp) {
            vec = launch_preproc_sp(0, SpPlanes{my.dev, mc.dev, (unsigned)img->pitch_y, (unsigned)img->pitch_c}, w, h, d_o, wp, hp, rife_sp::planar_pixfmt(img->chroma, img->csp),
                                    img->depth, force_scalar == 1);
        });
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_sp_to_rgb10: ") + hipGetErrorString(e));
        return vec ? 1 : 0;
    });
}
// ---- the semi-planar blend alone (include/rife_hip_test.h): uploaded as rife_hip_op_apply uploads ----
int rife_hip_op_apply_sp(int gpuid, const rife_hip_semiplanar_t* p0, const rife_hip_semiplanar_t* p1, const rife_hip_semiplanar_t* out, const rife_hip_motion_t* hm, int mw, int mh,
                         int force_scalar) {
    int rc;
    std::string err;
    if (rife_sp::check_call(p0, p1, out, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    if (mw != p0->w || mh != p0->h) return fail(RIFE_HIP_EINVAL, "op_apply_sp: the motion has the luma size");
    if (rife_apply::check_sets_motion(hm, mw, mh, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    if (force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_apply_sp: force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_apply_sp", [&] {
        const int w = p0->w, h = p0->h, ch = rife_sp::chroma_h(h, p0->chroma);
        const size_t rby = (size_t)w * 2, rbc = (size_t)rife_sp::chroma_w(w) * 4;
        ApplyMirror my[3], mc[3];
        MotionMirror mm;
        const rife_hip_semiplanar_t* src[3] = {p0, p1, out};
        rife_hip_semiplanar_t d[3] = {*p0, *p1, *out};
        hipError_t e = hipSuccess;
        for (int i = 0; i < 3 && e == hipSuccess; i++) {
            e = my[i].upload(src[i]->y, (size_t)src[i]->pitch_y, rby, h); d[i].y = my[i].dev;
            if (e == hipSuccess) { e = mc[i].upload(src[i]->cbcr, (size_t)src[i]->pitch_c, rbc, ch); d[i].cbcr = mc[i].dev; }
        }
        if (e == hipSuccess) e = mm.upload(*hm, mw, mh);
        int lrc = 0;
        bool vec = false;
        if (e == hipSuccess) e = op_on_own_stream(lrc, [&](hipStream_t st) {
            return sp_apply_launch(nullptr, st, sp_args(d[0], d[1], d[2], mm.flow.dev, hm->flow_pitch, mm.mask.dev, hm->mask_pitch, hm->format), p0->chroma, force_scalar == 1, &vec);
        });
        if (lrc) return lrc;
        if (e == hipSuccess) e = my[2].download(out->y, (size_t)out->pitch_y, rby);
        if (e == hipSuccess) e = mc[2].download(out->cbcr, (size_t)out->pitch_c, rbc);
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_apply_sp: ") + hipGetErrorString(e));
        return vec ? 1 : 0;
    });
}
#endif  // RIFE_HIP_TEST_BUILD

#ifdef RIFE_HIP_BENCH_BUILD
// ---- bench build only (tools/bench_semiplanar.py; nothing in the headers declares it): the blend ALONE on a motion the caller supplies, everything in DEVICE memory -
// variant 0: k_apply_sp on the surfaces p0, p1 -> out; variant 1: k_apply_yuv on the planar hbd images q0, q1 -> qout of the same size and depth.  Three untimed launches,
// then `iters` launches between two events on a stream of its own; *ms_out = milliseconds per launch.  A planar image the fused launch does not take is refused.
int rife_hip_bench_apply_sp(int gpuid, const rife_hip_semiplanar_t* p0, const rife_hip_semiplanar_t* p1, const rife_hip_semiplanar_t* out, const rife_hip_image_t* q0,
                            const rife_hip_image_t* q1, const rife_hip_image_t* qout, const rife_hip_motion_t* dm, int variant, int iters, float* ms_out) {
    int rc;
    std::string err;
    if (rife_sp::check_call(p0, p1, out, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    if (rife_hbd::check_call(q0, q1, qout, p0->depth, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    if (q0->w != p0->w || q0->h != p0->h || q0->pixfmt != rife_sp::planar_pixfmt(p0->chroma, p0->csp)) return fail(RIFE_HIP_EINVAL, "bench_apply_sp: the planar images are split(surface)");
    if (rife_apply::check_sets_motion(dm, p0->w, p0->h, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    if (!ms_out || iters < 1 || variant < 0 || variant > 1) return fail(RIFE_HIP_EINVAL, "bench_apply_sp: variant 0 or 1, iters >= 1 and a result pointer");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_bench_apply_sp", [&] {
        rife_hbd::Sets S;
        rife_hbd::make_sets(S, *q0, *q1, *qout, p0->depth);
        const HbdDev dv[2] = {{S.sets[0].p0, S.sets[0].p1, S.sets[0].out}, {S.sets[1].p0, S.sets[1].p1, S.sets[1].out}};
        const uint8_t* flow = static_cast<const uint8_t*>(dm->flow);
        const uint8_t* mask = static_cast<const uint8_t*>(dm->mask);
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        int lrc = 0;
        bool fused = true;
        for (int i = -3; i < iters && !lrc; i++) {
            if (i == 0) HIPCHK(hipEventRecord(e0, st));
            if (variant) lrc = hbd_apply_launch(nullptr, st, S.n, S.sets, dv, flow, dm->flow_pitch, mask, dm->mask_pitch, dm->format, p0->w, p0->h, true, &fused);
            else lrc = sp_apply_launch(nullptr, st, sp_args(*p0, *p1, *out, flow, dm->flow_pitch, mask, dm->mask_pitch, dm->format), p0->chroma);
            if (!lrc && !fused) lrc = fail(RIFE_HIP_EINVAL, "bench_apply_sp: the planar image does not take the fused launch");
        }
        if (!lrc) {
            HIPCHK(hipEventRecord(e1, st));
            HIPCHK(hipStreamSynchronize(st));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            *ms_out = ms / (float)iters;
        } else (void)hipStreamSynchronize(st);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
        return lrc;
    });
}
#endif  // RIFE_HIP_BENCH_BUILD

}  // extern "C"
