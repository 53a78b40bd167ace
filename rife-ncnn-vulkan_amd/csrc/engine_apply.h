// engine_apply.h: the apply entry points of include/rife_hip.h ("apply motion": rife_hip_planes_t) on top of engine_abi.h
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
//   apply_device_motion   one launch of k_apply_motion (apply_motion.h) on the caller's planes and motion, on the caller's stream
//   apply_motion          host planes and motion: tight device copies for the call's life, the launch, the planes back; needs no model and no workspace
//   process_device_apply  the motion pass with F32 motion into the workspace's tight motion buffers (motion_stage), then the launch on the same stream
//   process_apply         the same from host memory: frames and planes staged through workspace buffers (Ctx::ap_planes, allocated at the first such call)
//                         (both: engine_apply_sets.h's combined calls with one set of shift 0, 0)
// The rules and their words: csrc/apply_check.h.

// 0, or -RIFE_HIP_EINVAL; then "no HIP device at all" (-RIFE_HIP_ENODEV) before anything looks at the engine
static int apply_precheck(const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_planes_t* out, const rife_hip_motion_t* m, bool with_motion, int wp, int hp) {
    std::string err;
    if (rife_apply::check_call(p0, p1, out, m, with_motion, wp, hp, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    return no_hip_device();
}
// the combined calls are served where motion export is
static int apply_supported(const rife_hip* E) { return plain_v46_only(E, "process with apply motion is"); }
// what the kernel gets, for planes and motion in DEVICE memory
static ApplyArgs apply_args(const rife_hip_planes_t& p0, const rife_hip_planes_t& p1, const rife_hip_planes_t& out, const uint8_t* flow, size_t flow_pitch,
                            const uint8_t* mask, size_t mask_pitch, int format, int wp, int hp) {
    ApplyArgs a{};
    for (int k = 0; k < p0.n; k++) {
        a.p0[k] = static_cast<const uint8_t*>(p0.plane[k]); a.p1[k] = static_cast<const uint8_t*>(p1.plane[k]); a.out[k] = static_cast<uint8_t*>(out.plane[k]);
        a.pitch0[k] = (unsigned)p0.pitch[k]; a.pitch1[k] = (unsigned)p1.pitch[k]; a.pitcho[k] = (unsigned)out.pitch[k];
    }
    a.flow = flow; a.mask = mask; a.flow_pitch = (unsigned)flow_pitch; a.mask_pitch = (unsigned)mask_pitch; a.format = format;
    a.w = p0.w; a.h = p0.h; a.wp = wp ? wp : p0.w; a.hp = hp ? hp : p0.h; a.n = p0.n; a.maxval = p0.maxval;
    return a;
}
static int apply_launch(const rife_hip* E, hipStream_t st, const ApplyArgs& a, int sample, bool force_scalar = false) {
    Timed t(E->prof, "apply_motion", 0, st);
    launch_apply(st, a, sample, force_scalar);
    HIPCHK(hipGetLastError());
    return 0;
}
// timestep 0 / 1 of the combined calls: the planes of one frame, integer samples clamped to maxval
static int apply_copy_device(hipStream_t st, const rife_hip_planes_t& src, const rife_hip_planes_t& out) {
    const ApplyArgs a = apply_args(src, src, out, nullptr, 0, nullptr, 0, 0, 0, 0);
    launch_apply_copy(st, a, src.sample);
    HIPCHK(hipGetLastError());
    return 0;
}
static void apply_copy_host(const rife_hip_planes_t& src, const rife_hip_planes_t& out) {
    const size_t rb = rife_apply::row_bytes(src.w, src.sample);
    for (int k = 0; k < src.n; k++)
        for (int y = 0; y < src.h; y++) {
            const uint8_t* s = static_cast<const uint8_t*>(src.plane[k]) + (size_t)y * src.pitch[k];
            uint8_t* d = static_cast<uint8_t*>(out.plane[k]) + (size_t)y * out.pitch[k];
            if (src.sample == RIFE_HIP_SAMPLE_U8) for (int x = 0; x < src.w; x++) d[x] = (uint8_t)std::min<int>(s[x], src.maxval);
            else if (src.sample == RIFE_HIP_SAMPLE_U16) for (int x = 0; x < src.w; x++) reinterpret_cast<uint16_t*>(d)[x] = (uint16_t)std::min<int>(reinterpret_cast<const uint16_t*>(s)[x], src.maxval);
            else std::memmove(d, s, rb);
        }
}
// tight device copies of the three plane sets of a host call in ONE buffer `base` (3 n planes of h rows of w samples): the descriptors, and the copies in and out
struct ApplyStage { rife_hip_planes_t d0, d1, dout; };
static size_t apply_stage_bytes(const rife_hip_planes_t& p) { return 3 * (size_t)p.n * align_up((size_t)p.h * rife_apply::row_bytes(p.w, p.sample), 16); }
static ApplyStage apply_stage(uint8_t* base, const rife_hip_planes_t& p) {
    ApplyStage s{p, p, p};
    const size_t rb = rife_apply::row_bytes(p.w, p.sample), plane = align_up((size_t)p.h * rb, 16);
    rife_hip_planes_t* d[3] = {&s.d0, &s.d1, &s.dout};
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 4; k++) { d[i]->plane[k] = k < p.n ? base + ((size_t)i * p.n + k) * plane : nullptr; d[i]->pitch[k] = k < p.n ? (ptrdiff_t)rb : 0; }
    return s;
}
static hipError_t apply_planes_copy(const rife_hip_planes_t& dst, const rife_hip_planes_t& src, hipMemcpyKind kind, hipStream_t st) {
    hipError_t e = hipSuccess;
    const size_t rb = rife_apply::row_bytes(src.w, src.sample);
    for (int k = 0; k < src.n && e == hipSuccess; k++) e = hipMemcpy2DAsync(dst.plane[k], (size_t)dst.pitch[k], src.plane[k], (size_t)src.pitch[k], rb, (size_t)src.h, kind, st);
    return e;
}

static int rife_hip_apply_device_motion_impl(const rife_hip_t* E, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* dm, int wp, int hp,
                                             const rife_hip_planes_t* out, void* hip_stream) {
    int rc;
    if ((rc = apply_precheck(p0, p1, out, dm, true, wp, hp))) return rc;
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if ((rc = check_device(E->gpuid))) return rc;
    const ApplyArgs a = apply_args(*p0, *p1, *out, static_cast<const uint8_t*>(dm->flow), dm->flow_pitch, static_cast<const uint8_t*>(dm->mask), dm->mask_pitch, dm->format, wp, hp);
    if (hip_stream) return apply_launch(E, (hipStream_t)hip_stream, a, p0->sample);
    CopyStreamLease own(E);                                              // NULL: a stream of the engine's, drained before returning (never the legacy stream)
    if (own.err != hipSuccess) return fail(RIFE_HIP_EHIP, "hipStreamCreate failed");
    if ((rc = apply_launch(E, own.st, a, p0->sample))) return rc;
    HIPCHK(hipStreamSynchronize(own.st));
    return 0;
}

// host planes and host motion through tight device copies that live for the call; force_scalar: the test hook of rife_hip_op_apply never reaches here (its planes keep their pitch)
static int rife_hip_apply_motion_impl(const rife_hip_t* E, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* hm, int wp, int hp,
                                      const rife_hip_planes_t* out) {
    int rc;
    if ((rc = apply_precheck(p0, p1, out, hm, true, wp, hp))) return rc;
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if ((rc = check_device(E->gpuid))) return rc;
    const int w = p0->w, h = p0->h;
    const size_t frow = rife_motion::flow_row_bytes(w, hm->format), mrow = rife_motion::mask_row_bytes(w, hm->format);
    const size_t nplanes = apply_stage_bytes(*p0), nflow = align_up((size_t)h * frow, 16), nmask = (size_t)h * mrow;
    uint8_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), nplanes + nflow + nmask) != hipSuccess) return fail(RIFE_HIP_EHIP, "apply motion: hipMalloc of the staging buffer failed");
    const ApplyStage s = apply_stage(d, *p0);
    uint8_t *d_flow = d + nplanes, *d_mask = d_flow + nflow;
    hipError_t e;
    {
        CopyStreamLease own(E);
        hipStream_t st = own.st;
        e = own.err;
        if (e == hipSuccess) e = apply_planes_copy(s.d0, *p0, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = apply_planes_copy(s.d1, *p1, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpy2DAsync(d_flow, frow, hm->flow, hm->flow_pitch, frow, (size_t)h, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpy2DAsync(d_mask, mrow, hm->mask, hm->mask_pitch, mrow, (size_t)h, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            rc = apply_launch(E, st, apply_args(s.d0, s.d1, s.dout, d_flow, frow, d_mask, mrow, hm->format, wp, hp), p0->sample);
            if (!rc) e = apply_planes_copy(*out, s.dout, hipMemcpyDeviceToHost, st);
        }
        const hipError_t es = st ? hipStreamSynchronize(st) : hipSuccess;      // drained on every path: the buffer is freed next
        if (e == hipSuccess) e = es;
    }
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("apply motion: ") + hipGetErrorString(e));
    return 0;
}

// the argument checks of the two combined calls that need no engine
static int process_apply_precheck(int pixfmt, bool ptrs_ok, int w, int h, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* pout) {
    int rc;
    if ((rc = pixfmt_check(pixfmt))) return rc;
    if (!ptrs_ok) return fail(RIFE_HIP_EINVAL, "null pointer argument");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "bad frame size");
    std::string err;
    if (rife_apply::check_call(p0, p1, pout, nullptr, false, wp, hp, err)) return fail(RIFE_HIP_EINVAL, "apply motion: " + err);
    if (p0->w != w || p0->h != h) return fail(RIFE_HIP_EINVAL, "apply motion: the planes and the frames differ in size");
    return px_precheck(pixfmt, true, w, h);
}
// the workspace's tight F32 motion buffers (motion_stage) for a pass whose motion stays in device memory
static int apply_motion_stage(Ctx& c, MotionArgs& mo) {
    rife_hip_motion_t want{};
    want.flow = &want; want.mask = &want; want.format = RIFE_HIP_MOTION_F32;      // "both wanted": motion_stage reads nothing else of the pointers
    return motion_stage(c, want, mo);
}

// the two combined calls are the sets calls of engine_apply_sets.h with ONE set of shift 0, 0 (the same staging, the same launch of k_apply_motion, the same copies)
static int rife_hip_process_apply_sets_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out, int pixfmt, int nsets,
                                            const rife_hip_apply_set_t* sets);
static int rife_hip_process_device_apply_sets_impl(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt, int nsets,
                                                   const rife_hip_apply_set_t* sets, void* hip_stream);
static rife_hip_apply_set_t apply_one_set(const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_planes_t* pout, int wp, int hp) {
    rife_hip_apply_set_t s{};
    s.p0 = p0; s.p1 = p1; s.out = pout; s.wp = wp; s.hp = hp;
    return s;
}
static int rife_hip_process_apply_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out, int pixfmt,
                                       const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* pout) {
    const rife_hip_apply_set_t s = apply_one_set(p0, p1, pout, wp, hp);
    return rife_hip_process_apply_sets_impl(E, in0, in1, w, h, timestep, out, pixfmt, 1, &s);
}
static int rife_hip_process_device_apply_impl(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt,
                                              const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* pout, void* hip_stream) {
    const rife_hip_apply_set_t s = apply_one_set(p0, p1, pout, wp, hp);
    return rife_hip_process_device_apply_sets_impl(E, d_in0, d_in1, w, h, timestep, d_out, pixfmt, 1, &s, hip_stream);
}

extern "C" {

int rife_hip_planes_check(const rife_hip_planes_t* p) {
    std::string err;
    return rife_apply::check(p, err) ? fail(RIFE_HIP_EINVAL, "planes: " + err) : 0;
}
int rife_hip_padded_size(const rife_hip_t* E, int w, int h, int* wp, int* hp) {
    if (!E || !wp || !hp) return fail(RIFE_HIP_EINVAL, "null argument");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "bad frame size");
    const int pad = E->pad();                                             // 32n; flow scale 2: 64n (process_common)
    *wp = (w + pad - 1) / pad * pad; *hp = (h + pad - 1) / pad * pad;
    return 0;
}
int rife_hip_apply_device_motion(const rife_hip_t* E, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* device_motion, int wp, int hp,
                                 const rife_hip_planes_t* out, void* hip_stream) {
    return guarded("rife_hip_apply_device_motion", [&] { return rife_hip_apply_device_motion_impl(E, p0, p1, device_motion, wp, hp, out, hip_stream); });
}
int rife_hip_apply_motion(const rife_hip_t* E, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* host_motion, int wp, int hp,
                          const rife_hip_planes_t* out) {
    return guarded("rife_hip_apply_motion", [&] { return rife_hip_apply_motion_impl(E, p0, p1, host_motion, wp, hp, out); });
}
int rife_hip_process_apply(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt,
                           const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* planes_out) {
    int rc;
    if ((rc = process_apply_precheck(pixfmt, in0 && in1, w, h, p0, p1, wp, hp, planes_out))) return rc;      // out may be NULL: the frame is not wanted
    return guarded("rife_hip_process_apply", [&] {
        return rife_hip_process_apply_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, static_cast<uint8_t*>(out), pixfmt, p0, p1, wp, hp, planes_out);
    });
}
int rife_hip_process_device_apply(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt,
                                  const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, int wp, int hp, const rife_hip_planes_t* planes_out, void* hip_stream) {
    int rc;
    if ((rc = process_apply_precheck(pixfmt, d_in0 && d_in1 && d_out, w, h, p0, p1, wp, hp, planes_out))) return rc;
    return guarded("rife_hip_process_device_apply", [&] {
        return rife_hip_process_device_apply_impl(E, d_in0, d_in1, w, h, timestep, d_out, pixfmt, p0, p1, wp, hp, planes_out, hip_stream);
    });
}

#ifdef RIFE_HIP_TEST_BUILD
// ---- the apply kernel alone (include/rife_hip_test.h) ----
// one buffer's span (first byte of its first row .. last byte of its last row, gaps included) in a device allocation of its own, at the host pointer's alignment modulo 16
struct ApplyMirror {
    uint8_t* d = nullptr;
    uint8_t* dev = nullptr;
    size_t span = 0;
    std::vector<uint8_t> sent;
    ~ApplyMirror() { if (d) (void)hipFree(d); }
    hipError_t upload(const void* host, size_t pitch, size_t row, int h) {
        span = (size_t)(h - 1) * pitch + row;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), span + 32);
        if (e != hipSuccess) return e;
        dev = d + (reinterpret_cast<uintptr_t>(host) & 15);      // hipMalloc returns at least 16-byte alignment
        sent.assign(static_cast<const uint8_t*>(host), static_cast<const uint8_t*>(host) + span);
        return hipMemcpy(dev, sent.data(), span, hipMemcpyHostToDevice);
    }
    // rows come back as they are; a gap byte comes back only if the device changed it
    hipError_t download(void* host, size_t pitch, size_t row) {
        std::vector<uint8_t> got(span);
        const hipError_t e = hipMemcpy(got.data(), dev, span, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        uint8_t* hb = static_cast<uint8_t*>(host);
        for (size_t i = 0; i < span; i++) if (i % pitch < row || got[i] != sent[i]) hb[i] = got[i];
        return hipSuccess;
    }
};
// the three plane sets of one apply set and a host motion in device memory, every buffer an ApplyMirror of its own (pitches and pointer alignment kept): what the blend
// ops of this and the following sections launch on, and the output planes back
namespace {
struct ApplySetMirror {
    ApplyMirror m0[4], m1[4], mo[4];
    rife_hip_planes_t d0, d1, dout;
    hipError_t upload(const rife_hip_planes_t& p0, const rife_hip_planes_t& p1, const rife_hip_planes_t& out) {
        const size_t rb = rife_apply::row_bytes(p0.w, p0.sample);
        d0 = p0; d1 = p1; dout = out;
        hipError_t e = hipSuccess;
        for (int k = 0; k < p0.n && e == hipSuccess; k++) {
            e = m0[k].upload(p0.plane[k], (size_t)p0.pitch[k], rb, p0.h); d0.plane[k] = m0[k].dev;
            if (e == hipSuccess) { e = m1[k].upload(p1.plane[k], (size_t)p1.pitch[k], rb, p0.h); d1.plane[k] = m1[k].dev; }
            if (e == hipSuccess) { e = mo[k].upload(out.plane[k], (size_t)out.pitch[k], rb, p0.h); dout.plane[k] = mo[k].dev; }
        }
        return e;
    }
    hipError_t download(const rife_hip_planes_t& out) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < out.n && e == hipSuccess; k++) e = mo[k].download(out.plane[k], (size_t)out.pitch[k], rife_apply::row_bytes(out.w, out.sample));
        return e;
    }
};
struct MotionMirror {
    ApplyMirror flow, mask;
    hipError_t upload(const rife_hip_motion_t& hm, int mw, int mh) {
        const hipError_t e = flow.upload(hm.flow, hm.flow_pitch, rife_motion::flow_row_bytes(mw, hm.format), mh);
        return e != hipSuccess ? e : mask.upload(hm.mask, hm.mask_pitch, rife_motion::mask_row_bytes(mw, hm.format), mh);
    }
};
}  // namespace
int rife_hip_op_apply(int gpuid, const rife_hip_planes_t* p0, const rife_hip_planes_t* p1, const rife_hip_motion_t* hm, int wp, int hp, const rife_hip_planes_t* out, int force_scalar) {
    int rc;
    if ((rc = apply_precheck(p0, p1, out, hm, true, wp, hp))) return rc;
    if (force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_apply: force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_apply", [&] {
        ApplySetMirror m;
        MotionMirror mm;
        hipError_t e = m.upload(*p0, *p1, *out);
        if (e == hipSuccess) e = mm.upload(*hm, p0->w, p0->h);
        int lrc = 0;
        if (e == hipSuccess) e = op_on_own_stream(lrc, [&](hipStream_t st) {      // a launch error goes before what the drain says, in the op's own words
            launch_apply(st, apply_args(m.d0, m.d1, m.dout, mm.flow.dev, hm->flow_pitch, mm.mask.dev, hm->mask_pitch, hm->format, wp, hp), p0->sample, force_scalar == 1);
            const hipError_t le = hipGetLastError();
            return le == hipSuccess ? 0 : fail(RIFE_HIP_EHIP, std::string("op_apply: ") + hipGetErrorString(le));
        });
        if (lrc) return lrc;
        if (e == hipSuccess) e = m.download(*out);
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_apply: ") + hipGetErrorString(e));
        return 0;
    });
}
#endif  // RIFE_HIP_TEST_BUILD

}  // extern "C"
