// engine_hbd.h: the high-bit-depth entry points of include/rife_hip.h ("high bit depth": a rife_hip_image_t of u16 planes plus a depth of 10..16) on top of
// engine_apply_sets.h
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
// An hbd call IS the combined sets call on a ten-bit proxy of the planes (one set for I444P10 / RGBP10, luma + chroma sets for I420P10 / I422P10: hbd_check.h
// make_sets), except that the proxy never exists: the pre-processing kernels of hbd.h reduce the caller's samples on their way into the resident frames, the pass
// leaves its ten-bit frame in the workspace, and the apply launches of engine_apply_sets.h blend the same planes - for a subsampled image ONE launch of k_apply_yuv
// (apply_yuv.h) where its stores are aligned, with the same bytes (hbd_apply_launch).
//   process_device_hbd   the stream's workspace (StreamWorkspace); pre-processing, pass and apply launches on the caller's device planes, in place
//   process_hbd          a pool workspace (with_leased_ctx); host planes staged ONCE, 2 bytes per sample, in its apply staging (Ctx::ap_planes, apply_staging): the staged planes feed the pre-processing and
//                        the blend; the output planes come back with 2-D copies
// The rules and their words: csrc/hbd_check.h.

// 0, or -RIFE_HIP_EINVAL; then "no HIP device at all" (-RIFE_HIP_ENODEV) before anything looks at the engine
static int hbd_precheck(const rife_hip_image_t* in0, const rife_hip_image_t* in1, const rife_hip_image_t* out, int depth) {
    std::string err;
    if (rife_hbd::check_call(in0, in1, out, depth, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    return no_hip_device();
}
// served where the combined apply calls are
static int hbd_supported(const rife_hip* E) { return plain_v46_only(E, "high bit depth planes are"); }
// the sets of the definition, checked by the rules of the sets calls (nothing hbd_check let through fails them; a fault here is reported, not assumed away)
static int hbd_sets(rife_hbd::Sets& S, const rife_hip_image_t& in0, const rife_hip_image_t& in1, const rife_hip_image_t& out, int depth) {
    rife_hbd::make_sets(S, in0, in1, out, depth);
    std::string err;
    if (rife_apply::check_sets(S.n, S.sets, in0.w, in0.h, err)) return fail(RIFE_HIP_EINVAL, "high bit depth: " + err);
    return 0;
}
// Y, Cb, Cr (R, G, B) of input `which` (0, 1) as the pre-processing kernels take them, from the sets' descriptors: set 0 holds all three planes or the luma plane alone
static PlaneSet hbd_plane_set(int nsets, const rife_hip_planes_t& first, const rife_hip_planes_t* chroma) {
    PlaneSet s;
    for (int p = 0; p < 3; p++) {
        const rife_hip_planes_t& d = (nsets == 2 && p > 0) ? *chroma : first;
        const int k = (nsets == 2 && p > 0) ? p - 1 : p;
        s.p[p] = static_cast<uint8_t*>(d.plane[k]); s.pitch[p] = (size_t)d.pitch[k];
    }
    return s;
}

// the apply launches of an hbd call, on descriptors of DEVICE planes (d[k]: the planes of set k): a subsampled image - a luma set and a chroma set - is ONE launch of
// k_apply_yuv (apply_yuv.h) where its stores are aligned (apply_yuv_ok) and `fuse` (RIFE_HIP_APPLY_YUV, read per call) allows it; everything else is one launch per
// set, as in engine_apply_sets.h.  `prof`: null in the single-kernel test call; *fused tells that call which it was
struct HbdDev { const rife_hip_planes_t *p0, *p1, *out; };
static int hbd_apply_launch(Profiler* prof, hipStream_t st, int nsets, const rife_hip_apply_set_t* sets, const HbdDev* d, const uint8_t* flow, size_t flow_pitch,
                            const uint8_t* mask, size_t mask_pitch, int format, int mw, int mh, bool fuse, bool* fused = nullptr) {
    if (fused) *fused = false;
    if (nsets == 2 && fuse && sets[0].shift_x == 0 && sets[0].shift_y == 0 && sets[1].shift_x == -1 && d[0].p0->sample == d[1].p0->sample) {
        ApplyYuvArgs s{};
        s.y = apply_args(*d[0].p0, *d[0].p1, *d[0].out, flow, flow_pitch, mask, mask_pitch, format, sets[0].wp, sets[0].hp);
        s.c.a = apply_args(*d[1].p0, *d[1].p1, *d[1].out, flow, flow_pitch, mask, mask_pitch, format, sets[1].wp, sets[1].hp);
        s.c.mw = mw; s.c.mh = mh;
        if (apply_yuv_ok(s.y, s.c.a, d[0].p0->sample)) {
            {
                std::optional<Timed> t;
                if (prof) t.emplace(*prof, "apply_yuv", 0, st);
                launch_apply_yuv(st, s, sets[1].shift_y);
            }
            HIPCHK(hipGetLastError());
            if (fused) *fused = true;
            return 0;
        }
    }
    for (int k = 0; k < nsets; k++)
        if (int rc = apply_set_launch(prof, st, *d[k].p0, *d[k].p1, *d[k].out, sets[k], flow, flow_pitch, mask, mask_pitch, format, mw, mh)) return rc;
    return 0;
}

static int rife_hip_process_hbd_impl(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth) {
    int rc;
    const int w = in0->w, h = in0->h, pixfmt = in0->pixfmt;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = hbd_supported(E))) return rc;
    rife_hbd::Sets S;
    if ((rc = hbd_sets(S, *in0, *in1, *out, depth))) return rc;
    if (timestep == 0.f || timestep == 1.f) {                             // no pass, no arithmetic: the planes of frame 0 / frame 1, clamped to maxval
        for (int k = 0; k < S.n; k++) apply_copy_host(timestep == 0.f ? *S.sets[k].p0 : *S.sets[k].p1, *S.sets[k].out);
        return 0;
    }
    if ((rc = check_device(E->gpuid))) return rc;
    return with_leased_ctx(E, w, h, pixfmt, [&](Ctx& C) {
        MotionArgs mo;
        int rc = apply_motion_stage(C, mo);
        if (!rc) rc = apply_staging(C, sets_stage_bytes(S.n, S.sets));
        if (rc) return rc;
        ApplyStage sg[2] = {};
        sets_stage(C.ap_planes, S.n, S.sets, sg);
        rc = upload_with_token(E, C.stream, [&] { return sets_upload(S.n, S.sets, sg, C.stream); });
        const HbdIO io{hbd_plane_set(S.n, sg[0].d0, S.n == 2 ? &sg[1].d0 : nullptr), hbd_plane_set(S.n, sg[0].d1, S.n == 2 ? &sg[1].d1 : nullptr), depth};
        if (!rc) rc = run_v4(*E, C, nullptr, nullptr, timestep, nullptr, nullptr, nullptr, &mo, &io);
        const HbdDev dv[2] = {{&sg[0].d0, &sg[0].d1, &sg[0].dout}, {&sg[1].d0, &sg[1].d1, &sg[1].dout}};      // [1]: addresses only, read when S.n == 2
        if (!rc) rc = hbd_apply_launch(&E->prof, C.stream, S.n, S.sets, dv, mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32, w, h, read_switches().apply_yuv);
        hipError_t e;
        if (!rc && (e = sets_download(S.n, S.sets, sg, C.stream)) != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
        return rc;
    });
}

static int rife_hip_process_device_hbd_impl(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth,
                                            void* hip_stream) {
    int rc;
    const int w = in0->w, h = in0->h, pixfmt = in0->pixfmt;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if ((rc = hbd_supported(E))) return rc;
    rife_hbd::Sets S;
    if ((rc = hbd_sets(S, *in0, *in1, *out, depth))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    StreamWorkspace ws(E, hip_stream);
    if (ws.rc) return ws.rc;
    Ctx* const c = ws.c;
    if (timestep == 0.f || timestep == 1.f) {
        for (int k = 0; k < S.n; k++)
            if ((rc = apply_copy_device(c->stream, timestep == 0.f ? *S.sets[k].p0 : *S.sets[k].p1, *S.sets[k].out))) return rc;
    } else {
        MotionArgs mo;
        if ((rc = ensure_ctx(*c, w, h, pixfmt, E->pad()))) return rc;
        if ((rc = apply_motion_stage(*c, mo))) return rc;
        const HbdIO io{hbd_plane_set(S.n, S.d[0][0], S.n == 2 ? &S.d[1][0] : nullptr), hbd_plane_set(S.n, S.d[0][1], S.n == 2 ? &S.d[1][1] : nullptr), depth};
        if ((rc = run_v4(*E, *c, nullptr, nullptr, timestep, nullptr, nullptr, nullptr, &mo, &io))) return rc;
        const HbdDev dv[2] = {{S.sets[0].p0, S.sets[0].p1, S.sets[0].out}, {S.sets[1].p0, S.sets[1].p1, S.sets[1].out}};
        if ((rc = hbd_apply_launch(&E->prof, c->stream, S.n, S.sets, dv, mo.flow, mo.flow_pitch, mo.mask, mo.mask_pitch, RIFE_HIP_MOTION_F32, w, h, read_switches().apply_yuv))) return rc;
    }
    if (!hip_stream) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int rife_hip_hbd_check(const rife_hip_image_t* img, int depth) {
    std::string err;
    return rife_hbd::check(img, depth, err) ? fail(RIFE_HIP_EINVAL, "high bit depth: " + err) : 0;
}
int rife_hip_process_hbd(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth) {
    int rc;
    if ((rc = hbd_precheck(in0, in1, out, depth))) return rc;
    return guarded("rife_hip_process_hbd", [&] { return rife_hip_process_hbd_impl(E, in0, in1, timestep, out, depth); });
}
int rife_hip_process_device_hbd(const rife_hip_t* E, const rife_hip_image_t* in0, const rife_hip_image_t* in1, float timestep, const rife_hip_image_t* out, int depth,
                                void* hip_stream) {
    int rc;
    if ((rc = hbd_precheck(in0, in1, out, depth))) return rc;
    return guarded("rife_hip_process_device_hbd", [&] { return rife_hip_process_device_hbd_impl(E, in0, in1, timestep, out, depth, hip_stream); });
}

#ifdef RIFE_HIP_TEST_BUILD
// ---- the hbd pre-processing kernel alone (include/rife_hip_test.h): uploaded as rife_hip_op_image_to_resident uploads (ImageMirror: pitches and pointer alignment kept) ----
int rife_hip_op_hbd_to_rgb10(int gpuid, const rife_hip_image_t* img, int depth, uint32_t* out_padded, int force_scalar) {
    int rc;
    if ((rc = rife_hip_hbd_check(img, depth))) return rc;
    if (!out_padded || force_scalar < 0 || force_scalar > 1) return fail(RIFE_HIP_EINVAL, "op_hbd_to_rgb10: an output array and force_scalar 0 or 1");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_hbd_to_rgb10", [&] {
        ImageMirror m;
        hipError_t e = m.upload(*img);
        if (e == hipSuccess) e = op_padded_rgb10(img->w, img->h, out_padded, [&](uint32_t* d_o, int wp, int hp) {
            launch_preproc_hbd(0, plane_set(m.dev), img->w, img->h, d_o, wp, hp, img->pixfmt, depth, force_scalar == 1);
        });
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_hbd_to_rgb10: ") + hipGetErrorString(e));
        return 0;
    });
}
// ---- the apply launches of a subsampled hbd image alone (include/rife_hip_test.h): uploaded as rife_hip_op_apply_scaled uploads ----
int rife_hip_op_apply_yuv(int gpuid, const rife_hip_apply_set_t* luma_set, const rife_hip_apply_set_t* chroma_set, const rife_hip_motion_t* hm, int mw, int mh) {
    int rc;
    if (!luma_set || !chroma_set) return fail(RIFE_HIP_EINVAL, "op_apply_yuv: null set");
    const rife_hip_apply_set_t two[2] = {*luma_set, *chroma_set};
    if ((rc = sets_precheck(2, two, hm, true, mw, mh))) return rc;
    if (two[0].shift_x != 0 || two[0].shift_y != 0 || two[1].shift_x != -1)
        return fail(RIFE_HIP_EINVAL, "op_apply_yuv: a luma set of shift (0, 0) and a chroma set of shift (-1, -1) or (-1, 0)");
    if ((rc = check_device(gpuid))) return rc;
    return guarded("rife_hip_op_apply_yuv", [&] {
        ApplySetMirror m[2];
        MotionMirror mm;
        hipError_t e = hipSuccess;
        for (int s = 0; s < 2 && e == hipSuccess; s++) e = m[s].upload(*two[s].p0, *two[s].p1, *two[s].out);
        if (e == hipSuccess) e = mm.upload(*hm, mw, mh);
        int lrc = 0;
        bool fused = false;
        if (e == hipSuccess) e = op_on_own_stream(lrc, [&](hipStream_t st) {
            const HbdDev dv[2] = {{&m[0].d0, &m[0].d1, &m[0].dout}, {&m[1].d0, &m[1].d1, &m[1].dout}};
            return hbd_apply_launch(nullptr, st, 2, two, dv, mm.flow.dev, hm->flow_pitch, mm.mask.dev, hm->mask_pitch, hm->format, mw, mh, read_switches().apply_yuv, &fused);
        });
        if (lrc) return lrc;
        for (int s = 0; s < 2 && e == hipSuccess; s++) e = m[s].download(*two[s].out);
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_apply_yuv: ") + hipGetErrorString(e));
        return fused ? 1 : 0;
    });
}
#endif  // RIFE_HIP_TEST_BUILD

}  // extern "C"
