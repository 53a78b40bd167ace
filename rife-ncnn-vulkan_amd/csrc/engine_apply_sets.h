// engine_apply_sets.h: the sets entry points of include/rife_hip.h ("apply motion at another resolution": rife_hip_apply_set_t) on top of engine_apply.h
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
//   apply_device_motion_sets   one launch per set on the caller's planes and motion, on the caller's stream: k_apply_motion (shift 0, 0: the launch of
//                              rife_hip_apply_device_motion) or k_apply_motion_scaled (apply_scaled.h)
//   apply_motion_sets          host planes and motion: tight device copies for the call's life, the launches, the planes back; needs no model and no workspace
//   process_device_apply_sets  the motion pass with F32 motion into the workspace's tight motion buffers (motion_stage), then the launches on the same stream
//   process_apply_sets         the same from host memory: frames and planes staged through workspace buffers (Ctx::ap_planes, allocated at the first such call)
// The two combined calls of engine_apply.h (rife_hip_process_apply, rife_hip_process_device_apply) are these two with one set of shift 0, 0: there is ONE copy of the
// staging and the timestep 0 / 1 branch.  The workspace lookup, the lease, the upload token and the staging buffer are engine_abi.h's and engine_ctx.h's (StreamWorkspace,
// with_leased_ctx, upload_with_token, apply_staging).
// The rules and their words: csrc/apply_set_check.h.

// 0, or -RIFE_HIP_EINVAL; then "no HIP device at all" (-RIFE_HIP_ENODEV) before anything looks at the engine
static int sets_precheck(int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* m, bool with_motion, int mw, int mh) {
    std::string err;
    if (mw <= 0 || mh <= 0) return fail(RIFE_HIP_EINVAL, "apply motion: bad motion size");
    if (rife_apply::check_sets(nsets, sets, mw, mh, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    if (with_motion && rife_apply::check_sets_motion(m, mw, mh, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    return no_hip_device();
}
// one set with planes and motion in DEVICE memory; `prof`: null in the single-kernel test call
static int apply_set_launch(Profiler* prof, hipStream_t st, const rife_hip_planes_t& p0, const rife_hip_planes_t& p1, const rife_hip_planes_t& out, const rife_hip_apply_set_t& s,
                            const uint8_t* flow, size_t flow_pitch, const uint8_t* mask, size_t mask_pitch, int format, int mw, int mh, bool force_scalar = false) {
    const ApplyArgs a = apply_args(p0, p1, out, flow, flow_pitch, mask, mask_pitch, format, s.wp, s.hp);
    {
        std::optional<Timed> t;
        if (prof) t.emplace(*prof, s.shift_x == 0 ? "apply_motion" : s.shift_x < 0 ? "apply_motion_down" : "apply_motion_up", 0, st);
        if (s.shift_x == 0) launch_apply(st, a, p0.sample, force_scalar);
        else {
            ApplyScaledArgs sa{};
            sa.a = a; sa.mw = mw; sa.mh = mh;
            launch_apply_scaled(st, sa, s.shift_x, s.shift_y, p0.sample, force_scalar);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int rife_hip_apply_device_motion_sets_impl(const rife_hip_t* E, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* dm, int mw, int mh, void* hip_stream) {
    int rc;
    if ((rc = sets_precheck(nsets, sets, dm, true, mw, mh))) return rc;
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if ((rc = check_device(E->gpuid))) return rc;
    auto run = [&](hipStream_t st) {
        for (int k = 0; k < nsets; k++) {
            const rife_hip_apply_set_t& s = sets[k];
            const int r = apply_set_launch(&E->prof, st, *s.p0, *s.p1, *s.out, s, static_cast<const uint8_t*>(dm->flow), dm->flow_pitch, static_cast<const uint8_t*>(dm->mask),
                                           dm->mask_pitch, dm->format, mw, mh);
            if (r) return r;
        }
        return 0;
    };
    if (hip_stream) return run((hipStream_t)hip_stream);
    CopyStreamLease own(E);                                              // NULL: a stream of the engine's, drained before returning (never the legacy stream)
    if (own.err != hipSuccess) return fail(RIFE_HIP_EHIP, "hipStreamCreate failed");
    if ((rc = run(own.st))) return rc;
    HIPCHK(hipStreamSynchronize(own.st));
    return 0;
}

// the tight device copies of every set of a host call, one after the other from `base`
static size_t sets_stage_bytes(int nsets, const rife_hip_apply_set_t* sets) {
    size_t n = 0;
    for (int k = 0; k < nsets; k++) n += apply_stage_bytes(*sets[k].p0);
    return n;
}
static void sets_stage(uint8_t* base, int nsets, const rife_hip_apply_set_t* sets, ApplyStage* st) {
    for (int k = 0; k < nsets; k++) { st[k] = apply_stage(base, *sets[k].p0); base += apply_stage_bytes(*sets[k].p0); }
}
static hipError_t sets_upload(int nsets, const rife_hip_apply_set_t* sets, const ApplyStage* sg, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < nsets && e == hipSuccess; k++) {
        e = apply_planes_copy(sg[k].d0, *sets[k].p0, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = apply_planes_copy(sg[k].d1, *sets[k].p1, hipMemcpyHostToDevice, st);
    }
    return e;
}
static int sets_launch_staged(const rife_hip* E, hipStream_t st, int nsets, const rife_hip_apply_set_t* sets, const ApplyStage* sg, const uint8_t* flow, size_t flow_pitch,
                              const uint8_t* mask, size_t mask_pitch, int format, int mw, int mh) {
    for (int k = 0; k < nsets; k++) {
        const int rc = apply_set_launch(&E->prof, st, sg[k].d0, sg[k].d1, sg[k].dout, sets[k], flow, flow_pitch, mask, mask_pitch, format, mw, mh);
        if (rc) return rc;
    }
    return 0;
}
static hipError_t sets_download(int nsets, const rife_hip_apply_set_t* sets, const ApplyStage* sg, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < nsets && e == hipSuccess; k++) e = apply_planes_copy(*sets[k].out, sg[k].dout, hipMemcpyDeviceToHost, st);
    return e;
}

static int rife_hip_apply_motion_sets_impl(const rife_hip_t* E, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* hm, int mw, int mh) {
    int rc;
    if ((rc = sets_precheck(nsets, sets, hm, true, mw, mh))) return rc;
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if ((rc = check_device(E->gpuid))) return rc;
    const size_t frow = rife_motion::flow_row_bytes(mw, hm->format), mrow = rife_motion::mask_row_bytes(mw, hm->format);
    const size_t nplanes = sets_stage_bytes(nsets, sets), nflow = align_up((size_t)mh * frow, 16), nmask = (size_t)mh * mrow;
    uint8_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), nplanes + nflow + nmask) != hipSuccess) return fail(RIFE_HIP_EHIP, "apply motion: hipMalloc of the staging buffer failed");
    ApplyStage sg[4];
    sets_stage(d, nsets, sets, sg);
    uint8_t *d_flow = d + nplanes, *d_mask = d_flow + nflow;
    hipError_t e;
    {
        CopyStreamLease own(E);
        hipStream_t st = own.st;
        e = own.err;
        if (e == hipSuccess) e = sets_upload(nsets, sets, sg, st);
        if (e == hipSuccess) e = hipMemcpy2DAsync(d_flow, frow, hm->flow, hm->flow_pitch, frow, (size_t)mh, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpy2DAsync(d_mask, mrow, hm->mask, hm->mask_pitch, mrow, (size_t)mh, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            rc = sets_launch_staged(E, st, nsets, sets, sg, d_flow, frow, d_mask, mrow, hm->format, mw, mh);
            if (!rc) e = sets_download(nsets, sets, sg, st);
        }
        const hipError_t es = st ? hipStreamSynchronize(st) : hipSuccess;      // drained on every path: the buffer is freed next
        if (e == hipSuccess) e = es;
    }
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("apply motion: ") + hipGetErrorString(e));
    return 0;
}

// the argument checks of the two combined calls that need no engine; the motion is the frame's: mw, mh = w, h
static int process_apply_sets_precheck(int pixfmt, bool ptrs_ok, int w, int h, int nsets, const rife_hip_apply_set_t* sets) {
    int rc;
    if ((rc = pixfmt_check(pixfmt))) return rc;
    if (!ptrs_ok) return fail(RIFE_HIP_EINVAL, "null pointer argument");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "bad frame size");
    std::string err;
    if (rife_apply::check_sets(nsets, sets, w, h, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    return px_precheck(pixfmt, true, w, h);
}

static int rife_hip_process_apply_sets_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out, int pixfmt, int nsets,
                                            const rife_hip_apply_set_t* sets) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if ((rc = apply_supported(E))) return rc;
    const size_t nbytes = frame_bytes(w, h, pixfmt);
    if (timestep == 0.f || timestep == 1.f) {                             // no pass, no arithmetic: the frame as rife_hip_process_px returns it, every set's planes of that frame
        const uint8_t* src = timestep == 0.f ? in0 : in1;
        if (out) { if (pix_deep(pixfmt)) canon10_host(out, src, w, h, pixfmt); else std::memmove(out, src, nbytes); }
        for (int k = 0; k < nsets; k++) apply_copy_host(timestep == 0.f ? *sets[k].p0 : *sets[k].p1, *sets[k].out);
        return 0;
    }
    if ((rc = check_device(E->gpuid))) return rc;
    return with_leased_ctx(E, w, h, pixfmt, [&](Ctx& C) {
        MotionArgs mo;
        int rc = apply_motion_stage(C, mo);
        if (!rc) rc = apply_staging(C, sets_stage_bytes(nsets, sets));
        if (rc) return rc;
        ApplyStage sg[4];
        sets_stage(C.ap_planes, nsets, sets, sg);
        rc = upload_with_token(E, C.stream, [&] {
            const hipError_t e = host_pair_upload(C, in0, in1, nbytes);
            return e != hipSuccess ? e : sets_upload(nsets, sets, sg, C.stream);
        });
        if (!rc) rc = run_pass(E, C, C.d_in0, C.d_in1, w, h, timestep, C.d_out, &mo);
        if (!rc) rc = sets_launch_staged(E, C.stream, nsets, sets, sg, mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32, w, h);
        hipError_t e;
        if (!rc && out && (e = hipMemcpyAsync(out, C.d_out, nbytes, hipMemcpyDeviceToHost, C.stream)) != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
        if (!rc && (e = sets_download(nsets, sets, sg, C.stream)) != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
        return rc;
    });
}

static int rife_hip_process_device_apply_sets_impl(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt, int nsets,
                                                   const rife_hip_apply_set_t* sets, void* hip_stream) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if ((rc = apply_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    StreamWorkspace ws(E, hip_stream);
    if (ws.rc) return ws.rc;
    Ctx* const c = ws.c;
    if (timestep == 0.f || timestep == 1.f) {
        if ((rc = copy_frame_device(c->stream, timestep == 0.f ? d_in0 : d_in1, d_out, w, h, pixfmt))) return rc;
        for (int k = 0; k < nsets; k++)
            if ((rc = apply_copy_device(c->stream, timestep == 0.f ? *sets[k].p0 : *sets[k].p1, *sets[k].out))) return rc;
    } else {
        MotionArgs mo;
        if ((rc = ensure_ctx(*c, w, h, pixfmt, E->pad()))) return rc;
        if ((rc = apply_motion_stage(*c, mo))) return rc;
        if ((rc = run_pass(E, *c, static_cast<const uint8_t*>(d_in0), static_cast<const uint8_t*>(d_in1), w, h, timestep, static_cast<uint8_t*>(d_out), &mo))) return rc;
        for (int k = 0; k < nsets; k++)
            if ((rc = apply_set_launch(&E->prof, c->stream, *sets[k].p0, *sets[k].p1, *sets[k].out, sets[k], mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32, w, h)))
                return rc;
    }
    if (!hip_stream) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int rife_hip_apply_set_check(const rife_hip_apply_set_t* s, int mw, int mh) {
    std::string err;
    return rife_apply::check_set(s, mw, mh, err) ? fail(RIFE_HIP_EINVAL, "apply set: " + err) : 0;
}
int rife_hip_apply_device_motion_sets(const rife_hip_t* E, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* device_motion, int mw, int mh, void* hip_stream) {
    return guarded("rife_hip_apply_device_motion_sets", [&] { return rife_hip_apply_device_motion_sets_impl(E, nsets, sets, device_motion, mw, mh, hip_stream); });
}
int rife_hip_apply_motion_sets(const rife_hip_t* E, int nsets, const rife_hip_apply_set_t* sets, const rife_hip_motion_t* host_motion, int mw, int mh) {
    return guarded("rife_hip_apply_motion_sets", [&] { return rife_hip_apply_motion_sets_impl(E, nsets, sets, host_motion, mw, mh); });
}
int rife_hip_process_apply_sets(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, int nsets,
                                const rife_hip_apply_set_t* sets) {
    int rc;
    if ((rc = process_apply_sets_precheck(pixfmt, in0 && in1, w, h, nsets, sets))) return rc;      // out may be NULL: the frame is not wanted
    return guarded("rife_hip_process_apply_sets", [&] {
        return rife_hip_process_apply_sets_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, static_cast<uint8_t*>(out), pixfmt, nsets, sets);
    });
}
int rife_hip_process_device_apply_sets(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt, int nsets,
                                       const rife_hip_apply_set_t* sets, void* hip_stream) {
    int rc;
    if ((rc = process_apply_sets_precheck(pixfmt, d_in0 && d_in1 && d_out, w, h, nsets, sets))) return rc;
    return guarded("rife_hip_process_device_apply_sets", [&] {
        return rife_hip_process_device_apply_sets_impl(E, d_in0, d_in1, w, h, timestep, d_out, pixfmt, nsets, sets, hip_stream);
    });
}

#ifdef RIFE_HIP_TEST_BUILD
// ---- the scaled apply kernel alone (include/rife_hip_test.h) ----
int rife_hip_op_apply_scaled(int gpuid, const rife_hip_apply_set_t* set, const rife_hip_motion_t* hm, int mw, int mh, int force_scalar) {
    int rc;
    if ((rc = sets_precheck(1, set, hm, true, mw, mh))) return rc;
    if (force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_apply_scaled: force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_apply_scaled", [&] {
        ApplySetMirror m;
        MotionMirror mm;
        hipError_t e = m.upload(*set->p0, *set->p1, *set->out);
        if (e == hipSuccess) e = mm.upload(*hm, mw, mh);
        int lrc = 0;
        if (e == hipSuccess) e = op_on_own_stream(lrc, [&](hipStream_t st) {
            return apply_set_launch(nullptr, st, m.d0, m.d1, m.dout, *set, mm.flow.dev, hm->flow_pitch, mm.mask.dev, hm->mask_pitch, hm->format, mw, mh, force_scalar == 1);
        });
        if (lrc) return lrc;
        if (e == hipSuccess) e = m.download(*set->out);
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_apply_scaled: ") + hipGetErrorString(e));
        return 0;
    });
}
#endif  // RIFE_HIP_TEST_BUILD

}  // extern "C"
