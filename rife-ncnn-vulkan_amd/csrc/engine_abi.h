// engine_abi.h: the C-ABI of include/rife_hip.h (+ include/rife_hip_test.h in the test build, bench_hooks.h in the bench build)
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.

// ================================================================================================
// C-ABI
// ================================================================================================
namespace rife {
// the exception guard of the extern "C" entry points: nothing may throw across the C boundary (malformed model files, std::bad_alloc)
template <typename F>
static int guarded(const char* entry, F&& f) {
    try { return f(); }
    catch (const std::exception& e) { return fail(RIFE_HIP_EIO, std::string(entry) + ": " + e.what()); }
    catch (...) { return fail(RIFE_HIP_EIO, std::string(entry) + ": unknown exception"); }
}
}  // namespace rife

extern "C" {

const char* rife_hip_last_error(void) { return g_err.c_str(); }

int rife_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

rife_hip_t* rife_hip_create(int gpuid, int tta_mode, int tta_temporal_mode, int uhd_mode, int num_threads, int rife_v2, int rife_v4) {
    if (check_device(gpuid)) return nullptr;
    rife_hip* E = new rife_hip;
    E->gpuid = gpuid; E->tta = tta_mode; E->tta_temporal = tta_temporal_mode; E->uhd = uhd_mode;
    E->num_threads = num_threads; E->v2 = rife_v2; E->v4 = rife_v4;
    E->frame_pool = std::make_shared<FramePool>();
    E->frame_pool->gpuid = gpuid;
    const Switches sw = read_switches();                                 // engine scope: the kernel-selection switches of the test build (product: the defaults)
    E->t64 = sw.t64; E->rs = sw.rs; E->rs2 = sw.rs2; E->stem_rs = sw.stem_rs; E->tta_consensus = sw.tta_consensus;
    E->tail_rs = sw.tail_rs; E->tail_rs_always = sw.tail_rs_always; E->fuse_flow = sw.fuse_flow;
    if (sw.ks_mask >= 0) E->ks_mask = sw.ks_mask;
    if (E->fuse_flow) g_fuse_flow_buffers = true;
    return E;
}

void rife_hip_destroy(rife_hip_t* r) { delete r; }

static int rife_hip_load_impl(rife_hip_t* E, const char* modeldir) {
    if (!E || !modeldir) return fail(RIFE_HIP_EINVAL, "null argument");
    int rc;
    if ((rc = check_device(E->gpuid))) return rc;
    if (E->v2 && !E->v4) {
        if ((rc = load_v2(E, modeldir))) return rc;
        E->loaded = true;
        return 0;
    }
    if (!E->v4) {
        if ((rc = load_v1(E, modeldir))) return rc;
        E->loaded = true;
        return 0;
    }
    NcnnModel m;
    const std::string base = std::string(modeldir) + "/flownet";
    if (!m.load_param(base + ".param")) return fail(RIFE_HIP_EIO, m.error);
    const uint64_t gh = m.structural_hash("out0");
    if (gh != V46_HASH_OUT0 && gh != RIFE_V40_HASH_OUT0)
        return fail(RIFE_HIP_EMODEL, base + ".param is neither the rife-v4.6 nor the rife-v4 IFNet graph this engine schedules");
    if (!m.load_bin(base + ".bin")) return fail(RIFE_HIP_EIO, m.error);
    std::vector<const NcnnLayer*> wl = m.weighted();
    E->v40 = gh == RIFE_V40_HASH_OUT0;
    if (E->v40) {
        // rife-v4 (4.0): every conv is followed by its PReLU in the weight stream; the 5-channel head is padded to 8 output channels
        // (zero weights / bias) so that flow{b} keeps the [.][.][8] = {x, y, z, w, mask, 0, 0, 0} layout of the v4.6 schedule
        static const int C[4] = {192, 128, 96, 64}, SC[4] = {8, 4, 2, 1};
        size_t k = 0;
        for (int b = 0; b < 4; b++) {
            rife_hip::Block& B = E->blk[b];
            B.c = C[b]; B.scale = SC[b];
            static const char* const SN0[4] = {"stem0_b0", "stem0_b1", "stem0_b2", "stem0_b3"};
            static const char* const SN1[4] = {"stem1_b0", "stem1_b1", "stem1_b2", "stem1_b3"};
            static const char* const TN[4] = {"trunk_b0", "trunk_b1", "trunk_b2", "trunk_b3"};
            static const char* const HN[4] = {"head_b0", "head_b1", "head_b2", "head_b3"};
            auto take = [&](ConvLayer& L, int cin, int cout, int stride, bool deconv, const char* cls) -> int {
                if (k >= wl.size()) return fail(RIFE_HIP_EMODEL, "weight stream ended early");
                const NcnnLayer* nl = wl[k++];
                const int kk = deconv ? 16 : 9;
                if (nl->type != (deconv ? "Deconvolution" : "Convolution") || nl->geti(0, 0) != cout || (int)nl->weight.size() != cin * cout * kk ||
                    nl->geti(3, 1) != stride)
                    return fail(RIFE_HIP_EMODEL, "weighted layer " + nl->name + " does not match the rife-v4 schedule");
                free_layer(L);
                L.cin = cin; L.stride = deconv ? 1 : stride; L.deconv = deconv; L.epi = deconv ? EPI_DECONV : EPI_STORE; L.cls = cls; L.tag = 0; L.skip = false;
                if (deconv) {
                    L.cout = 8;
                    std::vector<float> w((size_t)8 * cin * 16, 0.f), bias(8, 0.f);
                    std::copy(nl->weight.begin(), nl->weight.end(), w.begin());              // ncnn deconv weights are [oc][ic][ky][kx]
                    std::copy(nl->bias.begin(), nl->bias.end(), bias.begin());
                    return upload_layer(L, w.data(), bias.data(), nullptr, 1.0f);
                }
                L.cout = cout;
                if (k >= wl.size() || wl[k]->type != "PReLU" || (int)wl[k]->slope.size() != cout) return fail(RIFE_HIP_EMODEL, "PReLU expected after " + nl->name);
                return upload_layer(L, nl->weight.data(), nl->bias.data(), wl[k++]->slope.data(), 1.0f);
            };
            if ((rc = take(B.stem0, b == 0 ? 7 : 12, C[b] / 2, 2, false, SN0[b]))) return rc;
            if ((rc = take(B.stem1, C[b] / 2, C[b], 2, false, SN1[b]))) return rc;
            for (int i = 0; i < 8; i++) if ((rc = take(B.res[i], C[b], C[b], 1, false, TN[b]))) return rc;
            if ((rc = take(B.head, C[b], 5, 2, true, HN[b]))) return rc;
        }
        if (k != wl.size()) return fail(RIFE_HIP_EMODEL, "flownet.bin has extra weighted layers");
        E->loaded = true;
        return 0;
    }
    if (wl.size() != 44) return fail(RIFE_HIP_EMODEL, "unexpected number of weighted layers");
    static const int C[4] = {192, 128, 96, 64}, SC[4] = {8, 4, 2, 1};
    size_t k = 0;
    for (int b = 0; b < 4; b++) {
        rife_hip::Block& B = E->blk[b];
        B.c = C[b]; B.scale = SC[b];
        char name[64];
        auto setup = [&](ConvLayer& L, int cin, int cout, int stride, bool deconv, int epi, float slope, const char* cls, bool fold_skip = false) -> int {
            const NcnnLayer* nl = wl[k++];
            const int kk = deconv ? 16 : 9;
            if (nl->type != (deconv ? "Deconvolution" : "Convolution") || nl->geti(0, 0) != cout || (int)nl->weight.size() != cin * cout * kk ||
                nl->geti(3, 1) != stride)
                return fail(RIFE_HIP_EMODEL, "weighted layer " + nl->name + " does not match the rife-v4.6 schedule");
            free_layer(L);
            L.cin = cin; L.cout = cout; L.stride = deconv ? 1 : stride; L.deconv = deconv; L.epi = epi; L.cls = cls;
            L.tag = std::strcmp(cls, "trunk_b3") == 0 ? 3 : 0;
            L.skip = fold_skip;
            L.want_t64 = fold_skip && cin == cout;
            L.want_s16out = !deconv && stride == 2 && cout == C[b];
            return upload_layer(L, nl->weight.data(), nl->bias.data(), nullptr, slope);
        };
        std::snprintf(name, sizeof name, "stem0_b%d", b);
        if ((rc = setup(B.stem0, b == 0 ? 7 : 12, C[b] / 2, 2, false, EPI_STORE, 0.2f, name))) return rc;
        std::snprintf(name, sizeof name, "stem1_b%d", b);
        if ((rc = setup(B.stem1, C[b] / 2, C[b], 2, false, EPI_STORE, 0.2f, name))) return rc;
        std::snprintf(name, sizeof name, "trunk_b%d", b);
        for (int i = 0; i < 8; i++)
            if ((rc = setup(B.res[i], C[b], C[b], 1, false, EPI_STORE, 0.2f, name, true))) return rc;
        std::snprintf(name, sizeof name, "head_b%d", b);
        if ((rc = setup(B.head, C[b], 24, 2, true, EPI_DECONV_PS, 1.0f, name))) return rc;
    }
    E->loaded = true;
    return 0;
}
int rife_hip_load(rife_hip_t* E, const char* modeldir) {
    return guarded("rife_hip_load", [&] { return rife_hip_load_impl(E, modeldir); });
}

// ---- flow scale (include/rife_hip.h): every IFBlock of rife-v4.6 at 1 / divisor of its resolution ----
int rife_hip_flow_scale(const rife_hip_t* E) { return E ? E->fscale : 1; }
int rife_hip_set_flow_scale(rife_hip_t* E, int divisor) {
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if (!E->loaded) return fail(RIFE_HIP_EINVAL, "set_flow_scale() before load(): the model family is not known yet");
    if (divisor <= 0 || (divisor & (divisor - 1))) return fail(RIFE_HIP_EINVAL, "the flow scale divisor must be a power of two (1 or 2)");
    if (divisor > 1) {
        const char* what = E->v1 ? "model family rife (v1: rife, rife-HD, rife-UHD, rife-anime)" : (!E->v4 && E->v3) ? "model family rife-v3.x" : !E->v4 ? "model family rife-v2.x"
                           : E->v40 ? "model family rife-v4 (4.0)" : E->tta ? "TTA mode (-x)" : E->tta_temporal ? "temporal TTA mode (-z)" : nullptr;
        if (what) return fail(RIFE_HIP_ENOSYS, std::string("flow scale 2 is served for model family rife-v4.6 in plain mode only, not for ") + what);
        if (divisor > 2) return fail(RIFE_HIP_ENOSYS, "flow scale 4 and above (upstream's scale 0.25) is not implemented");
    }
    if (divisor == E->fscale) return 0;
    return guarded("rife_hip_set_flow_scale", [&] {
        std::vector<std::unique_ptr<Ctx>> dead;                          // the workspaces were sized for the other padding and block scales; destroyed outside the lock
        {
            std::lock_guard<std::mutex> g(E->mu);
            if (E->leased > 0) return fail(RIFE_HIP_EINVAL, "set_flow_scale() while a call on the engine is in flight");
            dead.swap(E->free_ctx);
            for (auto& kv : E->stream_ctx) dead.push_back(std::move(kv.second));
            E->stream_ctx.clear();
            static const int SC[4] = {8, 4, 2, 1};
            for (int b = 0; b < 4; b++) E->blk[b].scale = SC[b] * divisor;
            E->fscale = divisor;
        }
        if (!dead.empty()) (void)hipSetDevice(E->gpuid);
        return 0;
    });
}

// ---- precision (include/rife_hip.h): one f16 product per weight tap of the S16 trunk kernels, the skip connection at full precision ----
int rife_hip_precision(const rife_hip_t* E) { return E ? E->precision : RIFE_HIP_PRECISION_FULL; }
int rife_hip_set_precision(rife_hip_t* E, int precision) {
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if (!E->loaded) return fail(RIFE_HIP_EINVAL, "set_precision() before load(): the model family is not known yet");
    if (precision != RIFE_HIP_PRECISION_FULL && precision != RIFE_HIP_PRECISION_FAST)
        return fail(RIFE_HIP_EINVAL, "the precision must be RIFE_HIP_PRECISION_FULL (0) or RIFE_HIP_PRECISION_FAST (1)");
    if (precision == RIFE_HIP_PRECISION_FAST) {
        const char* what = E->v1 ? "model family rife (v1: rife, rife-HD, rife-UHD, rife-anime)" : (!E->v4 && E->v3) ? "model family rife-v3.x" : !E->v4 ? "model family rife-v2.x"
                           : E->v40 ? "model family rife-v4 (4.0)" : E->tta ? "TTA mode (-x)" : E->tta_temporal ? "temporal TTA mode (-z)" : nullptr;
        if (what) return fail(RIFE_HIP_ENOSYS, std::string("fast precision is served for model family rife-v4.6 in plain mode only, not for ") + what);
    }
    if (precision == E->precision) return 0;
    return guarded("rife_hip_set_precision", [&] {
        std::vector<std::unique_ptr<Ctx>> dead;                          // a workspace may hold a captured graph of the other mode's kernels; destroyed outside the lock
        {
            std::lock_guard<std::mutex> g(E->mu);
            if (E->leased > 0) return fail(RIFE_HIP_EINVAL, "set_precision() while a call on the engine is in flight");
            dead.swap(E->free_ctx);
            for (auto& kv : E->stream_ctx) dead.push_back(std::move(kv.second));
            E->stream_ctx.clear();
            E->precision = precision;
        }
        if (!dead.empty()) (void)hipSetDevice(E->gpuid);
        return 0;
    });
}

static int process_common(const rife_hip* E, int w, int h, float timestep) {
    tl_cu_budget = 0;                                                    // every entry point starts on the whole chip; rife_hip_process_device sets its stream's part
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    if (!E->loaded) return fail(RIFE_HIP_EINVAL, "process() before load()");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "bad frame size");
    const int pad = E->pad();                                            // 32n, rife.cpp:2499-2500; flow scale 2: 64n
    if ((long long)((w + pad - 1) / pad * pad) * ((h + pad - 1) / pad * pad) > (1ll << 27))      // element indices are ints and the widest full-resolution tensor has 16 channels; (stem_rs has its own gate, block_on_stem_rs)
        return fail(RIFE_HIP_EINVAL, "frame too large (more than 2^27 padded pixels)");
    (void)timestep;
    if (E->uhd && !E->v4 && ((align_up(w, 32) / 2) % 32 || (align_up(h, 32) / 2) % 32))
        return fail(RIFE_HIP_EINVAL, "UHD mode needs a padded frame whose half size is a multiple of 32 (the reference's graph mis-sizes otherwise)");
    return 0;
}

// ---- deep colour and alpha (include/rife_hip.h RIFE_HIP_PIX_*) ----
// The 10-bit formats and RGBA8 are served by the plain rife-v4.6 schedule only; everything else is refused BEFORE anything is written or enqueued.
// nullptr = the plain rife-v4.6 schedule; otherwise the family or mode by name (the words of every "served for ... only" refusal)
static const char* not_plain_v46(const rife_hip* E) {
    return E->v1 ? "model family rife (v1: rife, rife-HD, rife-UHD, rife-anime)" : (!E->v4 && E->v3) ? "model family rife-v3.x" : !E->v4 ? "model family rife-v2.x"
           : E->v40 ? "model family rife-v4 (4.0)" : E->tta ? "TTA mode (-x)" : E->tta_temporal ? "temporal TTA mode (-z)" : E->uhd ? "UHD mode (-u)" : nullptr;
}
// 0, or the one refusal of everything the plain rife-v4.6 schedule alone serves (-RIFE_HIP_ENOSYS): "<subject> served for model family rife-v4.6 in plain mode only, not
// for <family or mode>"; `subject` ends in its verb ("motion export is", "high bit depth planes are")
static int plain_v46_only(const rife_hip* E, const std::string& subject) {
    const char* what = not_plain_v46(E);
    return what ? fail(RIFE_HIP_ENOSYS, subject + " served for model family rife-v4.6 in plain mode only, not for " + what) : 0;
}
static int pixfmt_supported(const rife_hip* E, int pixfmt) {
    if (pixfmt == RIFE_HIP_PIX_RGB8) return 0;
    return plain_v46_only(E, std::string(pixfmt == RIFE_HIP_PIX_RGBA8 ? "RGBA" : pix_yuv(pixfmt) ? "YUV" : pix_rgbp(pixfmt) ? "planar RGB" : "10-bit") + " frames are");
}
// argument checks of the _px entry points that need no engine; then "no HIP device at all" before anything looks at the engine
// a pixfmt argument = format | colour description (include/rife_hip.h RIFE_HIP_CSP_*): both must be something the library knows
static int pixfmt_check(int pixfmt) {      // the rules and their words: csrc/image_check.h, shared with rife_hip_image_check
    const char* fault = rife_img::pixfmt_fault(pixfmt);
    return fault ? fail(RIFE_HIP_EINVAL, fault) : 0;
}
static int px_precheck(int pixfmt, bool ptrs_ok, int w, int h) {
    int rc;
    if ((rc = pixfmt_check(pixfmt))) return rc;
    if (!ptrs_ok) return fail(RIFE_HIP_EINVAL, "null pointer argument");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "bad frame size");
    return no_hip_device();
}
// timestep 0 / 1 at depth 10: the input frame in canonical form (samples clamped to 1023, alpha bits 3) - what a pass over identical frames would write
// (YUV: the samples' codes - P010 low bits cleared, the planar 10-bit samples clamped to 1023, 8-bit frames unchanged; planar RGB: from10(to10(v)), planar_rgb.h)
static void canon10_host(void* out, const void* in, int w, int h, int pixfmt) {
    const size_t npix = (size_t)w * h;
    if (pix_rgbp(pixfmt)) { canon_row_host(canon_mode(pixfmt), static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), frame_bytes(w, h, pixfmt)); return; }
    if (pix_yuv(pixfmt)) {
        const size_t nbytes = frame_bytes(w, h, pixfmt);
        if (yuv_depth(pix_base(pixfmt)) == 8) { std::memmove(out, in, nbytes); return; }
        const bool p010 = pix_base(pixfmt) == RIFE_HIP_PIX_P010;
        const uint16_t* s = static_cast<const uint16_t*>(in); uint16_t* d = static_cast<uint16_t*>(out);
        for (size_t i = 0; i < nbytes / 2; i++) d[i] = p010 ? (uint16_t)(s[i] & 0xffc0u) : std::min<uint16_t>(s[i], 1023);
        return;
    }
    if (pixfmt == RIFE_HIP_PIX_RGB10_U16) {
        const uint16_t* s = static_cast<const uint16_t*>(in); uint16_t* d = static_cast<uint16_t*>(out);
        for (size_t i = 0; i < npix * 3; i++) d[i] = std::min<uint16_t>(s[i], 1023);
    } else {
        const uint32_t* s = static_cast<const uint32_t*>(in); uint32_t* d = static_cast<uint32_t*>(out);
        for (size_t i = 0; i < npix; i++) d[i] = s[i] | 0xc0000000u;
    }
}
static int copy_frame_device(hipStream_t st, const void* src, void* dst, int w, int h, int pixfmt) {
    const size_t npix = (size_t)w * h;
    if (pixfmt == RIFE_HIP_PIX_RGB10_U16)
        hipLaunchKernelGGL(k_canon10_u16, dim3((unsigned)((npix * 3 + 255) / 256)), dim3(256), 0, st, static_cast<const uint16_t*>(src), static_cast<uint16_t*>(dst), npix * 3);
    else if (pixfmt == RIFE_HIP_PIX_A2B10G10R10)
        hipLaunchKernelGGL(k_canon10_packed, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), npix);
    else if (pix_yuv(pixfmt) && yuv_depth(pix_base(pixfmt)) == 10) {
        const size_t n = frame_bytes(w, h, pixfmt) / 2;
        if (pix_base(pixfmt) == RIFE_HIP_PIX_P010) hipLaunchKernelGGL(k_canon_yuv10<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const uint16_t*>(src), static_cast<uint16_t*>(dst), n);
        else hipLaunchKernelGGL(k_canon_yuv10<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const uint16_t*>(src), static_cast<uint16_t*>(dst), n);
    }
    else if (pix_rgbp(pixfmt) && canon_mode(pixfmt) != CANON_BYTES) {      // a tight planar frame is 3 h rows of w samples
        const size_t rb = (size_t)w * rgbp_elem(pix_base(pixfmt));
        launch_canon_rows(st, canon_mode(pixfmt), static_cast<const uint8_t*>(src), rb, static_cast<uint8_t*>(dst), rb, rb, 3 * h);
    }
    else { HIPCHK(hipMemcpyAsync(dst, src, frame_bytes(w, h, pixfmt), hipMemcpyDeviceToDevice, st)); return 0; }      // RGB8, RGBA8, RGBP8 and 8-bit YUV: the bytes unchanged
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- motion export (include/rife_hip.h rife_hip_motion_t; the rules and their words: csrc/motion_check.h) ----
// served by the plain rife-v4.6 schedule only; everything else is refused BEFORE anything is written or enqueued
static int motion_supported(const rife_hip* E) { return plain_v46_only(E, "motion export is"); }
static int motion_check(const rife_hip_motion_t* m, int w, int h) {
    std::string err;
    return rife_motion::check(m, w, h, err) ? fail(RIFE_HIP_EINVAL, "motion: " + err) : 0;
}
// what a kernel gets (elementwise.h) for buffers in DEVICE memory
static MotionArgs motion_args(const rife_hip_motion_t& m) {
    MotionArgs a;
    a.flow = static_cast<uint8_t*>(m.flow); a.mask = static_cast<uint8_t*>(m.mask);
    a.flow_pitch = (unsigned)m.flow_pitch; a.mask_pitch = (unsigned)m.mask_pitch; a.format = m.format;
    return a;
}
// timestep 0 / 1 (a copy of a frame, no pass): flow 0, mask 1 - timestep; into host buffers, and into device buffers on a stream
static void motion_fill_host(const rife_hip_motion_t& m, int w, int h, float mask) {
    const bool f16 = m.format == RIFE_HIP_MOTION_F16;
    for (int y = 0; y < h; y++) {
        if (m.flow) std::memset(static_cast<uint8_t*>(m.flow) + (size_t)y * m.flow_pitch, 0, rife_motion::flow_row_bytes(w, m.format));
        if (!m.mask) continue;
        uint8_t* row = static_cast<uint8_t*>(m.mask) + (size_t)y * m.mask_pitch;
        if (f16) { const uint16_t v = mask == 1.f ? 0x3c00 : 0; for (int x = 0; x < w; x++) reinterpret_cast<uint16_t*>(row)[x] = v; }      // 1.0 and 0.0 as binary16
        else for (int x = 0; x < w; x++) reinterpret_cast<float*>(row)[x] = mask;
    }
}
static int motion_fill_device(hipStream_t st, const rife_hip_motion_t& m, int w, int h, float mask) {
    hipLaunchKernelGGL(k_motion_fill, grid2d(w, h), dim3(256), 0, st, motion_args(m), w, h, mask);
    HIPCHK(hipGetLastError());
    return 0;
}
// the host calls: the pass writes tight device buffers of the caller's format, allocated by the workspace's first motion call that wants them (largest format: a later
// call of either format fits), and 2-D copies move them into the caller's pitch
static int motion_stage(Ctx& c, const rife_hip_motion_t& hm, MotionArgs& a) {
    int rc;
    const size_t npix = (size_t)c.w * c.h;
    if (hm.flow && !c.mo_flow && (rc = dalloc(c, c.mo_flow, npix * 16))) return rc;
    if (hm.mask && !c.mo_mask && (rc = dalloc(c, c.mo_mask, npix * 4))) return rc;
    a.flow = hm.flow ? c.mo_flow : nullptr; a.mask = hm.mask ? c.mo_mask : nullptr;
    a.flow_pitch = (unsigned)rife_motion::flow_row_bytes(c.w, hm.format); a.mask_pitch = (unsigned)rife_motion::mask_row_bytes(c.w, hm.format); a.format = hm.format;
    return 0;
}
static int motion_download(const Ctx& c, const rife_hip_motion_t& hm, const MotionArgs& a) {
    if (hm.flow) HIPCHK(hipMemcpy2DAsync(hm.flow, hm.flow_pitch, a.flow, a.flow_pitch, a.flow_pitch, (size_t)c.h, hipMemcpyDeviceToHost, c.stream));
    if (hm.mask) HIPCHK(hipMemcpy2DAsync(hm.mask, hm.mask_pitch, a.mask, a.mask_pitch, a.mask_pitch, (size_t)c.h, hipMemcpyDeviceToHost, c.stream));
    return 0;
}

// Workspace pool of the host-buffer entry points (rife_hip_process from the reference's proc threads, process_frames, the workers of process_batch).
// Pool streams are ordinary streams: every workspace sees the whole chip.  Round 6 built and measured the layout VERDICT r5 (item 6) asked for - CU-partitioned
// pool streams from the number of callers in flight (four and more: frames of 4 Mpixel and more two per half of the compute units, smaller ones one per
// quarter, like bench.py's resident-frame legs; "in flight" = the most at any of the last 32 leases, because a layout that follows the count of the moment
// rebuilds a 1.6 GB workspace at every flip) - and it LOSES on this path (profiles/r6/ab_pool_partitions.txt, same call, 96 pairs, two rounds): 4K process()
// from 4 threads 243 - 321 frames/s partitioned against 424 - 450 whole-chip, process_batch() 322 - 372 against 454 - 485; 1080p 559 - 647 against 1,364 - 1,472.
// The H2D / D2H copies of a caller ride on its workspace's stream, and on a CU-masked stream they are no longer SDMA transfers that overlap the other callers'
// kernels.  With whole-chip streams the reference's own surface already reaches the resident-frame headline of the same box within 1 - 3 % (3 caller threads
// 475 - 490, process_batch 483 - 485 frames/s at 4K).  The layout stays reachable for A/B: RIFE_HIP_POOL_PARTS=2 / 4 (test build) forces it, =3 selects the
// from-the-callers rule.
// Trimming: a released workspace is destroyed when the pool holds more than the most callers that were in flight at any of the last 32 leases (a burst of N
// concurrent 4K callers no longer pins N x 1.6 GB for the engine's life); workspaces of a layout that is no longer in use go first, then the
// oldest.
static int pool_layout(int callers, int w, int h) {
    const int forced = process_switches().pool_parts;
    if (forced == 2 || forced == 4) return forced;
    if (forced != 3 || callers < 4) return 1;
    return (long long)w * h >= 4000000ll ? 2 : 4;
}
// the stream of part `part` of `parts` of the chip: CU-masked (the CUs with cu % parts == part) or, for one part, an ordinary non-blocking stream; *cus = the CUs it owns
static hipError_t create_part_stream(int part, int parts, hipStream_t* st, int* cus) {
    const int ncu = device_cus(true);
    *cus = ncu;
    if (parts == 1) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    *cus = 0;
    for (int cu = 0; cu < ncu; cu++) if (cu % parts == part) { mask[cu / 32] |= 1u << (cu % 32); (*cus)++; }
    return hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data());
}
// force_parts = 1: a whole-chip stream whatever the callers in flight (the lockstep groups of process_batch: a group's batched coarse-block launches ride on ONE
// of its two streams and must see the whole chip)
static int lease_ctx(const rife_hip* E, std::unique_ptr<Ctx>& c, int w, int h, int force_parts = 0, int pixfmt = RIFE_HIP_PIX_RGB8) {
    int parts, part = 0;
    {
        std::lock_guard<std::mutex> g(E->mu);
        const int callers = ++E->leased;
        E->lease_hist[E->lease_n++ % 32] = callers;
        int hw = 1;
        for (int v : E->lease_hist) hw = std::max(hw, v);
        parts = force_parts ? force_parts : pool_layout(hw, w, h);
        if (!force_parts) E->pool_parts_now = parts;
        // a pooled workspace of this layout, on the partition with the fewest workspaces in use (newest first among equals: its tensors are the likeliest to
        // have this frame size); none pooled: a new one on the least-used partition
        int pick = -1;
        for (int i = (int)E->free_ctx.size() - 1; i >= 0; i--) {
            const Ctx& f = *E->free_ctx[i];
            if (f.pool_parts != parts) continue;
            if (pick < 0 || E->part_live[parts][f.pool_part] < E->part_live[parts][E->free_ctx[pick]->pool_part]) pick = i;
        }
        if (pick >= 0) { c = std::move(E->free_ctx[pick]); E->free_ctx.erase(E->free_ctx.begin() + pick); part = c->pool_part; }
        else for (int p = 1; p < parts; p++) if (E->part_live[parts][p] < E->part_live[parts][part]) part = p;
        E->part_live[parts][part]++;
    }
    if (!c) {
        c.reset(new Ctx);
        c->pool_parts = parts; c->pool_part = part;
        int mine = 0;
        if (create_part_stream(part, parts, &c->stream, &mine) != hipSuccess) c->stream = nullptr;
        if (parts > 1) c->cu_budget = mine;
        if (!c->stream) {                                                // no stream: the lease never happened (a workspace without one must not reach the pool through the caller's release)
            std::lock_guard<std::mutex> g(E->mu);
            E->leased--; E->part_live[parts][part]--;
            c.reset();
            return fail(RIFE_HIP_EHIP, parts > 1 ? "hipExtStreamCreateWithCUMask failed" : "hipStreamCreate failed");
        }
        c->own_stream = true;
    }
    tl_cu_budget = c->cu_budget;                                         // the caller enqueues on this workspace's stream next
    return E->v4 ? ensure_ctx(*c, w, h, pixfmt, E->pad()) : E->v1 ? ensure_ctx_v1(*c, w, h, E->tta ? 8 : 1, E->tta_temporal ? 2 : 1)
                                                : ensure_ctx_v2(*c, w, h, E->uhd, E->tta ? 8 : 1, E->tta_temporal ? 2 : 1, E->v3, ctx_batch_serves(*E));
}

// the caller has drained the workspace's stream (every path synchronises before it releases)
static void release_ctx(const rife_hip* E, std::unique_ptr<Ctx>& c) {
    std::vector<std::unique_ptr<Ctx>> dead;                              // destroyed outside the lock (hipFree, hipStreamDestroy)
    {
        std::lock_guard<std::mutex> g(E->mu);
        E->leased--;
        E->part_live[c->pool_parts][c->pool_part]--;
        E->free_ctx.push_back(std::move(c));
        int hw = 1;
        for (int v : E->lease_hist) hw = std::max(hw, v);
        while ((int)E->free_ctx.size() + E->leased > hw) {               // another layout's first, then the oldest
            size_t v = 0;
            for (size_t i = 0; i < E->free_ctx.size(); i++) if (E->free_ctx[i]->pool_parts != E->pool_parts_now) { v = i; break; }
            dead.push_back(std::move(E->free_ctx[v])); E->free_ctx.erase(E->free_ctx.begin() + v);
        }
    }
}

extern "C++" {      // templates cannot have C linkage
// The skeleton of a host call that runs a pass: a pool workspace sized for w x h frames of `pixfmt`, `body(workspace)` enqueues everything on its stream (0 or an rc), the
// stream is drained whatever the body said (nothing may still run on the caller's buffers when the call returns; a failing drain is reported only where the body did not
// fail first) and the workspace goes back to the pool.  A workspace whose tensors could not be allocated still returns its lease.
template <typename F>
static int with_leased_ctx(const rife_hip* E, int w, int h, int pixfmt, F&& body) {
    std::unique_ptr<Ctx> c;
    int rc = lease_ctx(E, c, w, h, 0, pixfmt);
    if (!rc) rc = body(*c);
    if (c && hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(RIFE_HIP_EHIP, "stream sync failed");
    if (c) release_ctx(E, c);
    return rc;
}

// Upload token (round 6, RIFE_HIP_H2D_TOKEN=0 in the test build: off): one caller uploads at a time and holds the token until its frames have landed.
// Callers that run in lockstep - all copying over the one PCIe link at once, then all computing - fall out of phase by construction: B's upload rides
// under A's pass (tools/host_path_bench2.py: 2 caller threads read anything between 272 and 446 frames/s at 4K without it, profiles/r6/ab_h2d_token.txt).
// `enqueue()` issues the call's host-to-device copies on `st` and returns their hipError_t; with the token the stream is drained before the token is given up
// (page-locked frames: the copies only enqueue).  0, or -RIFE_HIP_EHIP "H2D: ...".
template <typename F>
static int upload_with_token(const rife_hip* E, hipStream_t st, F&& enqueue) {
    const bool token = process_switches().h2d_token;
    hipError_t e;
    {
        std::unique_lock<std::mutex> g(E->h2d_mu, std::defer_lock);
        if (token) g.lock();
        e = enqueue();
        if (e == hipSuccess && token) e = hipStreamSynchronize(st);
    }
    return e == hipSuccess ? 0 : fail(RIFE_HIP_EHIP, std::string("H2D: ") + hipGetErrorString(e));
}
}  // extern "C++"

// the pass of the engine's model family on workspace c (the caller has made it fit: lease_ctx / ensure_ctx*)
// mo != null: a motion call (the caller has passed motion_supported: plain rife-v4.6) - the plain pass with the motion target; the graph replay does not apply
static int run_pass(const rife_hip* E, Ctx& c, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out, const MotionArgs* mo = nullptr) {
    if (mo) return run_v4(*E, c, in0, in1, timestep, out, nullptr, nullptr, mo);
    if (E->v1) return run_v1(*E, c, in0, in1, out);
    if (!E->v4) return run_v2(*E, c, in0, in1, out);
    if (!E->tta && !E->tta_temporal) return run_v4_replay(*E, c, in0, in1, timestep, out);
    // the TTA workspaces are shared by all callers: serialise, and drain before the next caller may reuse them
    std::lock_guard<std::mutex> g(E->tta_mu);
    int rc = run_v4_tta(*E, c.stream, in0, in1, w, h, timestep, out);
    if (!rc && hipStreamSynchronize(c.stream) != hipSuccess) rc = fail(RIFE_HIP_EHIP, "TTA stream sync failed");
    return rc;
}

// both tight frames of a host call into the workspace's staging, enqueued on its stream (inside upload_with_token)
static hipError_t host_pair_upload(Ctx& c, const void* in0, const void* in1, size_t nbytes) {
    const hipError_t e = hipMemcpyAsync(c.d_in0, in0, nbytes, hipMemcpyHostToDevice, c.stream);
    return e != hipSuccess ? e : hipMemcpyAsync(c.d_in1, in1, nbytes, hipMemcpyHostToDevice, c.stream);
}
// H2D of both frames, the whole pass and the D2H of the result, all enqueued on the workspace's stream (no host wait)
// hm != null: + the pass's motion into the workspace's tight buffers and their download into the caller's host buffers
static int enqueue_host_pair(const rife_hip* E, Ctx& c, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out, const rife_hip_motion_t* hm = nullptr) {
    MotionArgs mo;
    if (hm) { if (int rc = motion_stage(c, *hm, mo)) return rc; }
    const size_t nbytes = frame_bytes(w, h, c.pixfmt);      // c.pixfmt: set by lease_ctx (deep colour: rife-v4.6 plain pass only, pixfmt_supported)
    if (int rc = upload_with_token(E, c.stream, [&] { return host_pair_upload(c, in0, in1, nbytes); })) return rc;
    if (int rc = run_pass(E, c, c.d_in0, c.d_in1, w, h, timestep, c.d_out, hm ? &mo : nullptr)) return rc;
    const hipError_t e = hipMemcpyAsync(out, c.d_out, nbytes, hipMemcpyDeviceToHost, c.stream);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("D2H: ") + hipGetErrorString(e));
    return hm ? motion_download(c, *hm, mo) : 0;
}

// hm (here and in the two impls below): a motion call - host buffers here and in process_frames, device buffers in process_device
static int rife_hip_process_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out, int pixfmt = RIFE_HIP_PIX_RGB8,
                                 const rife_hip_motion_t* hm = nullptr) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (!in0 || !in1 || !out) return fail(RIFE_HIP_EINVAL, "null frame pointer");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if (hm && (rc = motion_supported(E))) return rc;
    const size_t nbytes = frame_bytes(w, h, pixfmt);
    // rife.cpp:2470-2480: timestep 0 / 1 return an input frame unchanged (the reference rebinds the Mat; a copy is pixel-identical)
    if (hm && (timestep == 0.f || timestep == 1.f)) motion_fill_host(*hm, w, h, 1.f - timestep);
    if (pix_deep(pixfmt) && (timestep == 0.f || timestep == 1.f)) { canon10_host(out, timestep == 0.f ? in0 : in1, w, h, pixfmt); return 0; }
    if (timestep == 0.f) { std::memmove(out, in0, nbytes); return 0; }
    if (timestep == 1.f) { std::memmove(out, in1, nbytes); return 0; }
    if ((rc = check_device(E->gpuid))) return rc;
    return with_leased_ctx(E, w, h, pixfmt, [&](Ctx& c) { return enqueue_host_pair(E, c, in0, in1, w, h, timestep, out, hm); });
}
int rife_hip_process(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, uint8_t* out) {
    return guarded("rife_hip_process", [&] { return rife_hip_process_impl(E, in0, in1, w, h, timestep, out); });
}
size_t rife_hip_frame_bytes(int w, int h, int pixfmt) {
    return (w > 0 && h > 0 && pixfmt >= 0) ? frame_bytes(w, h, pix_base(pixfmt)) : 0;      // the colour bits do not change the size
}
int rife_hip_process_px(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt) {
    int rc;
    if ((rc = px_precheck(pixfmt, in0 && in1 && out, w, h))) return rc;
    return guarded("rife_hip_process_px", [&] { return rife_hip_process_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, static_cast<uint8_t*>(out), pixfmt); });
}

// n independent frame pairs from host memory in one call.  Copies from / to pageable host memory block the thread that issues
// them, so overlap of one pair's copies with another pair's kernels needs several host threads - the reference's proc threads
// (src/main.cpp:849-866).  The batch call brings its own: 2 workers (the reference default), each a plain rife_hip_process() loop over its share of
// the pairs (every call leases its own workspace + stream).  Same pixels as n rife_hip_process() calls.
struct rife_hip_frame {
    uint8_t* d = nullptr;      // tight u8 HWC RGB, the layout every run_* entry takes
    int w = 0, h = 0, gpuid = 0;
    int pixfmt = RIFE_HIP_PIX_RGB8;      // the format it was uploaded in (rife_hip_frame_upload_px)
    size_t nbytes = 0;
    std::shared_ptr<FramePool> pool;
};

int rife_hip_process_batch(const rife_hip_t* E, int n, const uint8_t* const* in0, const uint8_t* const* in1, const float* timestep,
                           uint8_t* const* out, int w, int h) {
    int rc;
    if (n < 0 || (n > 0 && (!in0 || !in1 || !timestep || !out))) return fail(RIFE_HIP_EINVAL, "bad batch arguments");
    if ((rc = process_common(E, w, h, 0.5f))) return rc;
    for (int i = 0; i < n; i++) if (!in0[i] || !in1[i] || !out[i]) return fail(RIFE_HIP_EINVAL, "null frame pointer");
    if (n == 0) return 0;
    if ((rc = check_device(E->gpuid))) return rc;
    // three workers = three pairs in flight: tools/host_path_bench2.py, 4K, 48 pairs: process() from 1 / 2 / 3 / 4 caller threads
    // 192 / 341 / 389 / 365 frames/s from pageable frames (resident frames: 395), 244 / 307 / 349 / 344 from page-locked ones
    const int batch_workers = process_switches().batch_workers;
    // round 4: four workers (measured against 3 / 5 / 6 / 8: 4K 439 vs 426 / 426 / 431 / 446, 1080p 1,334 vs 1,251 / 1,367 / 1,443 / 1,398 pageable; page-locked best at 4).
    // Round 6, with conv_rs2 and the trimmed pool (profiles/r6/ab_batch_workers.txt, same call, two rounds): frames of 4 Mpixel and more are better served by SIX -
    // 4K 492 - 495 pageable / 482 - 488 page-locked against 481 - 482 / 450 - 456 from four (3: 468 / 431, 8: 466 - 468 / 436 - 438): at the resident-frame rate;
    // 1080p stays at four (6: + 1 ... 7 % pageable, - 3 ... 5 % page-locked)
    const int K = std::min(n, batch_workers ? batch_workers : ((long long)w * h >= 4000000ll ? 6 : 4));
    // A host frame that serves several pairs of the batch (consecutive pairs of a sequence share one) crosses PCIe once: it becomes a
    // resident frame on first use and is released after its last (stream mode, below).  Batches without shared frames run as before.
    struct Shared { std::mutex mu; rife_hip_frame_t* f = nullptr; int left = 0; };
    std::map<const uint8_t*, std::unique_ptr<Shared>> shared;
    bool any_shared = false;
    for (int i = 0; i < n; i++) {
        if (timestep[i] == 0.f || timestep[i] == 1.f) continue;
        for (const uint8_t* p : {in0[i], in1[i]}) {
            auto& sl = shared[p];
            if (!sl) sl.reset(new Shared);
            any_shared |= ++sl->left > 1;
        }
    }
    auto resident = [&](const uint8_t* p, rife_hip_frame_t*& f) -> int {
        Shared& sl = *shared.find(p)->second;
        std::lock_guard<std::mutex> g(sl.mu);
        const int r = sl.f ? 0 : rife_hip_frame_upload(E, p, w, h, &sl.f);
        f = sl.f;
        return r;
    };
    auto retire = [&](const uint8_t* p) {
        Shared& sl = *shared.find(p)->second;
        std::lock_guard<std::mutex> g(sl.mu);
        if (--sl.left == 0) { rife_hip_frame_release(sl.f); sl.f = nullptr; }
    };
    std::vector<int> rcs(K, 0);
    std::vector<std::string> errs(K);
    // Lockstep groups (plain rife-v4.6 on the S16 trunks): three workers, each takes groups of two consecutive pairs through run_v4_group - the coarse
    // blocks of a group are batched launches - so up to six pairs are in flight and one worker's copies overlap the others' passes.  A trailing odd pair,
    // timestep 0 / 1 copies and every other model family take the per-pair path below.
    // (only where the coarse grids leave CUs idle - block 0 on the row kernel, frames up to ~1080p: at 3840x2160 a coarse layer of ONE pair already
    // fills the chip, measured 405 - 413 frames/s in groups against 400 - 425 per pair; RIFE_HIP_BATCH_GROUPS=1 / 0 forces / forbids the path)
    const int genv = read_switches().batch_groups;      // per call: 1 / 0 force / forbid, -1 by grid size
    const int Ht0 = (h + 31) / 32, Wt0 = (w + 31) / 32;
    const bool small_grid = ((Wt0 + 31) / 32) * Ht0 <= device_cus(true) * 5 / 8;      // MI355X: 160 workgroups, block 0 on the row kernel (block_on_row_kernel)
    const bool groups = E->v4 && !E->v40 && !E->v1 && !E->tta && !E->tta_temporal && E->t64 && n >= 2 && (genv >= 0 ? genv != 0 : small_grid);
    if (groups) {
        std::vector<std::array<int, 2>> grp;                 // pair indices of a group, -1 = none
        std::vector<int> singles;
        {
            int pend = -1;
            for (int i = 0; i < n; i++) {
                if (timestep[i] == 0.f || timestep[i] == 1.f) { singles.push_back(i); continue; }
                if (pend < 0) pend = i; else { grp.push_back({pend, i}); pend = -1; }
            }
            if (pend >= 0) singles.push_back(pend);
        }
        const int KG = std::min<int>(batch_workers ? batch_workers : 4, (int)grp.size() + (singles.empty() ? 0 : 1));      // four workers x two pairs in flight
        std::vector<int> grc(std::max(KG, 1), 0);
        std::vector<std::string> gerr(std::max(KG, 1));
        const size_t nbytes = (size_t)w * h * 3;
        auto one_pair = [&](int i) -> int {
            if (timestep[i] == 0.f || timestep[i] == 1.f) return rife_hip_process(E, in0[i], in1[i], w, h, timestep[i], out[i]);
            rife_hip_frame_t *f0 = nullptr, *f1 = nullptr;
            int r = resident(in0[i], f0);
            if (!r) r = resident(in1[i], f1);
            if (!r) r = rife_hip_process_frames(E, f0, f1, timestep[i], out[i]);
            retire(in0[i]); retire(in1[i]);
            return r;
        };
        auto gworker = [&](int k) {
            (void)hipSetDevice(E->gpuid);
            std::unique_ptr<Ctx> c[2];
            int r = 0;
            for (size_t q = k; q < grp.size() && !r; q += KG) {
                const int ia = grp[q][0], ib = grp[q][1];
                rife_hip_frame_t* f[4] = {nullptr, nullptr, nullptr, nullptr};
                const uint8_t* hp[4] = {in0[ia], in1[ia], in0[ib], in1[ib]};
                int nres = 0;
                for (; nres < 4 && !r; nres++) r = resident(hp[nres], f[nres]);
                if (r) nres--;
                for (int g = 0; g < 2 && !r; g++) if (!c[g]) r = lease_ctx(E, c[g], w, h, 1);
                if (!r) {
                    Ctx* cs[2] = {c[0].get(), c[1].get()};
                    const uint8_t* d0[2] = {f[0]->d, f[2]->d}; const uint8_t* d1[2] = {f[1]->d, f[3]->d};
                    const float ts[2] = {timestep[ia], timestep[ib]};
                    uint8_t* dout[2] = {c[0]->d_out, c[1]->d_out};
                    r = run_v4_group(*E, cs, 2, d0, d1, ts, dout);
                    if (!r && hipMemcpyAsync(out[ia], c[0]->d_out, nbytes, hipMemcpyDeviceToHost, c[0]->stream) != hipSuccess) r = fail(RIFE_HIP_EHIP, "D2H failed");
                    if (!r && hipMemcpyAsync(out[ib], c[1]->d_out, nbytes, hipMemcpyDeviceToHost, c[1]->stream) != hipSuccess) r = fail(RIFE_HIP_EHIP, "D2H failed");
                }
                for (int g = 0; g < 2; g++) if (c[g] && hipStreamSynchronize(c[g]->stream) != hipSuccess && !r) r = fail(RIFE_HIP_EHIP, "stream sync failed");
                for (int j = 0; j < nres; j++) retire(hp[j]);
            }
            for (int g = 0; g < 2; g++) if (c[g]) release_ctx(E, c[g]);
            if (!r && k == KG - 1) for (int i : singles) if ((r = one_pair(i))) break;       // the leftovers ride on the last worker
            if (r) { grc[k] = r; gerr[k] = g_err; }
        };
        std::vector<std::thread> gth;
        for (int k = 1; k < KG; k++) gth.emplace_back(gworker, k);
        if (KG > 0) gworker(0);
        for (auto& t : gth) t.join();
        for (auto& kv : shared) if (kv.second->f) rife_hip_frame_release(kv.second->f);      // only after an error
        for (int k = 0; k < KG; k++) if (grc[k]) { g_err = gerr[k]; return grc[k]; }
        return 0;
    }
    auto worker = [&](int k) {
        (void)hipSetDevice(E->gpuid);
        for (int i = k; i < n; i += K) {
            int r;
            if (!any_shared || timestep[i] == 0.f || timestep[i] == 1.f) r = rife_hip_process(E, in0[i], in1[i], w, h, timestep[i], out[i]);
            else {
                rife_hip_frame_t *f0 = nullptr, *f1 = nullptr;
                r = resident(in0[i], f0);
                if (!r) r = resident(in1[i], f1);
                if (!r) r = rife_hip_process_frames(E, f0, f1, timestep[i], out[i]);
                retire(in0[i]); retire(in1[i]);
            }
            if (r) { rcs[k] = r; errs[k] = g_err; return; }     // g_err is thread-local: carry it back to the caller
        }
    };
    std::vector<std::thread> th;
    for (int k = 1; k < K; k++) th.emplace_back(worker, k);
    worker(0);
    for (auto& t : th) t.join();
    for (auto& kv : shared) if (kv.second->f) rife_hip_frame_release(kv.second->f);      // only after an error
    for (int k = 0; k < K; k++) if (rcs[k]) { g_err = errs[k]; return rcs[k]; }
    return 0;
}

// ---- stream mode: frames resident in device memory across calls (include/rife_hip.h) ----

// a copy stream borrowed from E->upload_streams (a new one when the pool is empty), given back on every exit path; never the legacy stream
extern "C++" struct CopyStreamLease {
    const rife_hip* E;
    hipStream_t st = nullptr;
    hipError_t err = hipSuccess;
    explicit CopyStreamLease(const rife_hip* E_) : E(E_) {
        {
            std::lock_guard<std::mutex> g(E->mu);
            if (!E->upload_streams.empty()) { st = E->upload_streams.back(); E->upload_streams.pop_back(); }
        }
        if (!st) err = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    }
    CopyStreamLease(const CopyStreamLease&) = delete;
    ~CopyStreamLease() { if (st) { std::lock_guard<std::mutex> g(E->mu); E->upload_streams.push_back(st); } }
    template <typename F>
    hipError_t run(F&& enqueue) const {                                  // `enqueue(stream)`, then drained: the bytes have landed when it returns
        hipError_t e = err;
        if (e == hipSuccess) e = enqueue(st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e;
    }
    hipError_t copy(void* dst, const void* src, size_t nbytes, hipMemcpyKind kind) const {
        return run([&](hipStream_t s) { return hipMemcpyAsync(dst, src, nbytes, kind, s); });
    }
};

static int rife_hip_frame_upload_impl(const rife_hip_t* E, const uint8_t* rgb, int w, int h, rife_hip_frame_t** frame, int pixfmt = RIFE_HIP_PIX_RGB8) {
    if (frame) *frame = nullptr;
    if (!E || !rgb || !frame) return fail(RIFE_HIP_EINVAL, "null argument");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "bad frame size");
    int rc;
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    std::unique_ptr<rife_hip_frame> f(new rife_hip_frame);
    f->w = w; f->h = h; f->gpuid = E->gpuid; f->pixfmt = pixfmt;
    const size_t nbytes = frame_bytes(w, h, pixfmt);
    f->nbytes = nbytes; f->pool = E->frame_pool;
    if (!(f->d = f->pool->take(nbytes))) return fail(RIFE_HIP_EHIP, "hipMalloc of a resident frame failed");
    // a copy on its own stream, drained here: the frame is complete before any stream of any caller can see the handle
    const hipError_t e = CopyStreamLease(E).copy(f->d, rgb, nbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { f->pool->give(f->d, nbytes); return fail(RIFE_HIP_EHIP, std::string("frame upload: ") + hipGetErrorString(e)); }
    *frame = f.release();
    return 0;
}
int rife_hip_frame_upload(const rife_hip_t* E, const uint8_t* rgb, int w, int h, rife_hip_frame_t** frame) {
    return guarded("rife_hip_frame_upload", [&] { return rife_hip_frame_upload_impl(E, rgb, w, h, frame); });
}
int rife_hip_frame_upload_px(const rife_hip_t* E, const void* pixels, int w, int h, int pixfmt, rife_hip_frame_t** frame) {
    if (frame) *frame = nullptr;
    int rc;
    if ((rc = px_precheck(pixfmt, pixels && frame, w, h))) return rc;
    return guarded("rife_hip_frame_upload_px", [&] { return rife_hip_frame_upload_impl(E, static_cast<const uint8_t*>(pixels), w, h, frame, pixfmt); });
}

void rife_hip_frame_release(rife_hip_frame_t* f) {
    if (!f) return;
    if (f->d) f->pool->give(f->d, f->nbytes);
    delete f;
}

static int rife_hip_process_frames_impl(const rife_hip_t* E, const rife_hip_frame_t* f0, const rife_hip_frame_t* f1, float timestep, uint8_t* out,
                                        const rife_hip_motion_t* hm = nullptr) {
    if (!f0 || !f1 || !out) return fail(RIFE_HIP_EINVAL, "null frame pointer");
    if (f0->w != f1->w || f0->h != f1->h) return fail(RIFE_HIP_EINVAL, "the two frames differ in size");
    if (f0->pixfmt != f1->pixfmt) return fail(RIFE_HIP_EINVAL, "the two frames differ in pixel format or colour description");
    const int w = f0->w, h = f0->h, pixfmt = f0->pixfmt;
    int rc;
    if (hm && (rc = motion_check(hm, w, h))) return rc;      // the frames carry the size: checked here, before the engine is looked at
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (f0->gpuid != E->gpuid || f1->gpuid != E->gpuid) return fail(RIFE_HIP_EINVAL, "frame was uploaded to another device");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if (hm && (rc = motion_supported(E))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    const size_t nbytes = frame_bytes(w, h, pixfmt);
    if (timestep == 0.f || timestep == 1.f) {                 // rife.cpp:2470-2480 (a copy stream of the pool, never the legacy stream)
        const hipError_t e = CopyStreamLease(E).copy(out, timestep == 0.f ? f0->d : f1->d, nbytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("frame download: ") + hipGetErrorString(e));
        if (pix_deep(pixfmt)) canon10_host(out, out, w, h, pixfmt);
        if (hm) motion_fill_host(*hm, w, h, 1.f - timestep);
        return 0;
    }
    return with_leased_ctx(E, w, h, pixfmt, [&](Ctx& C) {
        int rc = 0;
        MotionArgs mo;
        if (hm) rc = motion_stage(C, *hm, mo);
        if (!rc) rc = run_pass(E, C, f0->d, f1->d, w, h, timestep, C.d_out, hm ? &mo : nullptr);
        if (!rc && hipMemcpyAsync(out, C.d_out, nbytes, hipMemcpyDeviceToHost, C.stream) != hipSuccess) rc = fail(RIFE_HIP_EHIP, "D2H failed");
        if (!rc && hm) rc = motion_download(C, *hm, mo);
        return rc;
    });
}
int rife_hip_process_frames(const rife_hip_t* E, const rife_hip_frame_t* f0, const rife_hip_frame_t* f1, float timestep, uint8_t* out) {
    return guarded("rife_hip_process_frames", [&] { return rife_hip_process_frames_impl(E, f0, f1, timestep, out); });
}

// The workspace of a device call: the one of the caller's stream (NULL: of the engine's own stream, created here - never the legacy stream), found or made under E->mu
// and held until the call returns.  rc != 0: no workspace, the error is set.
namespace {      // file-local, like the functions around it: its constructor is no symbol of the library
struct StreamWorkspace {
    int rc = 0;
    Ctx* c = nullptr;
    std::unique_lock<std::mutex> use;
    StreamWorkspace(const rife_hip* E, void* hip_stream) {
        {
            std::lock_guard<std::mutex> g(E->mu);
            auto ps = E->part_streams.find(hip_stream);
            if (ps != E->part_streams.end()) tl_cu_budget = ps->second;      // a stream of rife_hip_stream_create: persistent grids for its part of the chip
            auto& slot = E->stream_ctx[hip_stream];
            if (!slot) {
                slot.reset(new Ctx);
                if (hip_stream) slot->stream = (hipStream_t)hip_stream;
                else if (hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking) == hipSuccess) slot->own_stream = true;
                else {      // no workspace without a stream stays behind: the next call on this key would find it and run on the legacy stream
                    E->stream_ctx.erase(hip_stream);
                    rc = fail(RIFE_HIP_EHIP, "hipStreamCreate failed");
                    return;
                }
            }
            c = slot.get();
        }
        // two host threads on the same stream (in particular NULL = the engine's own) share one workspace: the second waits here instead of
        // racing on its (re)allocation and scratch tensors - work on one stream executes in order anyway
        use = std::unique_lock<std::mutex>(c->use);
    }
    StreamWorkspace(const StreamWorkspace&) = delete;
};
}  // namespace

static int rife_hip_process_device_impl(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, void* hip_stream,
                                        int pixfmt = RIFE_HIP_PIX_RGB8, const rife_hip_motion_t* dm = nullptr) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (!d_in0 || !d_in1 || !d_out) return fail(RIFE_HIP_EINVAL, "null frame pointer");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if (dm && (rc = motion_supported(E))) return rc;
    const MotionArgs mo = dm ? motion_args(*dm) : MotionArgs();
    if ((rc = check_device(E->gpuid))) return rc;
    StreamWorkspace ws(E, hip_stream);
    if (ws.rc) return ws.rc;
    Ctx* const c = ws.c;
    if (timestep == 0.f || timestep == 1.f) {
        if ((rc = copy_frame_device(c->stream, timestep == 0.f ? d_in0 : d_in1, d_out, w, h, pixfmt))) return rc;
        if (dm && (rc = motion_fill_device(c->stream, *dm, w, h, 1.f - timestep))) return rc;
    } else {
        if (E->v1) rc = ensure_ctx_v1(*c, w, h, E->tta ? 8 : 1, E->tta_temporal ? 2 : 1);
        else if (!E->v4) rc = ensure_ctx_v2(*c, w, h, E->uhd, E->tta ? 8 : 1, E->tta_temporal ? 2 : 1, E->v3, ctx_batch_serves(*E));
        else if (!E->tta && !E->tta_temporal) rc = ensure_ctx(*c, w, h, pixfmt, E->pad());      // the TTA pass has workspaces of its own
        if (rc || (rc = run_pass(E, *c, (const uint8_t*)d_in0, (const uint8_t*)d_in1, w, h, timestep, (uint8_t*)d_out, dm ? &mo : nullptr))) return rc;
    }
    if (!hip_stream) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
int rife_hip_process_device(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, void* hip_stream) {
    return guarded("rife_hip_process_device", [&] { return rife_hip_process_device_impl(E, d_in0, d_in1, w, h, timestep, d_out, hip_stream); });
}
int rife_hip_process_device_px(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt, void* hip_stream) {
    int rc;
    if ((rc = px_precheck(pixfmt, d_in0 && d_in1 && d_out, w, h))) return rc;
    return guarded("rife_hip_process_device_px", [&] { return rife_hip_process_device_impl(E, d_in0, d_in1, w, h, timestep, d_out, hip_stream, pixfmt); });
}

// ---- motion export: the three calls (include/rife_hip.h).  Argument checks that need no engine first (-EINVAL), then "no HIP device at all", then the impls above ----
int rife_hip_motion_check(const rife_hip_motion_t* m, int w, int h) { return motion_check(m, w, h); }
static int motion_precheck(int pixfmt, bool ptrs_ok, int w, int h, const rife_hip_motion_t* m) {
    int rc;
    if ((rc = pixfmt_check(pixfmt))) return rc;
    if (!ptrs_ok) return fail(RIFE_HIP_EINVAL, "null pointer argument");
    if ((rc = motion_check(m, w, h))) return rc;
    return px_precheck(pixfmt, true, w, h);
}
int rife_hip_process_motion(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep, void* out, int pixfmt, const rife_hip_motion_t* host_motion) {
    int rc;
    if ((rc = motion_precheck(pixfmt, in0 && in1 && out, w, h, host_motion))) return rc;
    return guarded("rife_hip_process_motion", [&] {
        return rife_hip_process_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, static_cast<uint8_t*>(out), pixfmt, host_motion);
    });
}
int rife_hip_process_device_motion(const rife_hip_t* E, const void* d_in0, const void* d_in1, int w, int h, float timestep, void* d_out, int pixfmt,
                                   const rife_hip_motion_t* device_motion, void* hip_stream) {
    int rc;
    if ((rc = motion_precheck(pixfmt, d_in0 && d_in1 && d_out, w, h, device_motion))) return rc;
    return guarded("rife_hip_process_device_motion", [&] { return rife_hip_process_device_impl(E, d_in0, d_in1, w, h, timestep, d_out, hip_stream, pixfmt, device_motion); });
}
int rife_hip_process_frames_motion(const rife_hip_t* E, const rife_hip_frame_t* f0, const rife_hip_frame_t* f1, float timestep, void* out, const rife_hip_motion_t* host_motion) {
    if (!host_motion) return fail(RIFE_HIP_EINVAL, "motion: null motion descriptor");
    return guarded("rife_hip_process_frames_motion", [&] { return rife_hip_process_frames_impl(E, f0, f1, timestep, static_cast<uint8_t*>(out), host_motion); });
}

// n resident pairs in one call (include/rife_hip.h): lockstep groups of two pairs (run_v4_group: the coarse-block trunks of a group are one
// launch per layer) on leased workspaces and their streams, forked from and joined into `hip_stream` with events - no host wait.
static int rife_hip_process_device_batch_impl(const rife_hip_t* E, int n, const void* const* d_in0, const void* const* d_in1, const float* timestep,
                                              void* const* d_out, int w, int h, void* hip_stream, int pixfmt = RIFE_HIP_PIX_RGB8) {
    int rc;
    if (n < 0 || (n > 0 && (!d_in0 || !d_in1 || !timestep || !d_out))) return fail(RIFE_HIP_EINVAL, "bad batch arguments");
    if ((rc = process_common(E, w, h, 0.5f))) return rc;
    for (int i = 0; i < n; i++) if (!d_in0[i] || !d_in1[i] || !d_out[i]) return fail(RIFE_HIP_EINVAL, "null frame pointer");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if (n == 0) return 0;
    if ((rc = check_device(E->gpuid))) return rc;
    const bool groups = E->v4 && !E->v40 && !E->v1 && !E->tta && !E->tta_temporal && E->t64;
    if (!groups) {      // other families / TTA: the pairs one after the other on the caller's stream
        for (int i = 0; i < n; i++)
            if ((rc = rife_hip_process_device_impl(E, d_in0[i], d_in1[i], w, h, timestep[i], d_out[i], hip_stream, pixfmt))) return rc;
        return 0;
    }
    hipStream_t user = (hipStream_t)hip_stream;
    // the fork event goes back to the pool on EVERY exit path (re-recorded by its next user; waits already enqueued keep their own snapshot of it)
    struct ForkLease {
        const rife_hip_t* E; hipEvent_t ev = nullptr;
        ~ForkLease() { if (ev) { std::lock_guard<std::mutex> g(E->mu); E->batch_fork.push_back(ev); } }
    } fk{E};
    {
        std::lock_guard<std::mutex> g(E->mu);
        if (!E->batch_fork.empty()) { fk.ev = E->batch_fork.back(); E->batch_fork.pop_back(); }
    }
    if (!fk.ev) HIPCHK(hipEventCreateWithFlags(&fk.ev, hipEventDisableTiming));
    hipEvent_t fork = fk.ev;
    if (user) HIPCHK(hipEventRecord(fork, user));      // NULL = "the engine's own streams": nothing to order against, the call synchronises before it returns
    // At most MAXG groups (2 MAXG workspaces) are in flight however many pairs the call carries: further groups re-use them round-robin - work on a
    // workspace's stream executes in order, so a re-used workspace simply queues behind its previous pair (device memory stays O(1) in n).
    constexpr int MAXG = 4;
    std::vector<std::unique_ptr<Ctx>> cs;
    std::unique_ptr<Ctx> copy_ctx;                       // timestep 0 / 1 with no caller stream: one internal stream for the D2D copies
    size_t next_slot = 0;
    auto lease_new = [&](std::unique_ptr<Ctx>& c) -> bool {
        if (lease_ctx(E, c, w, h, 1, pixfmt)) { if (c) release_ctx(E, c); return false; }      // a workspace whose tensors could not be allocated still returns its lease
        if (!c->ev_group && hipEventCreateWithFlags(&c->ev_group, hipEventDisableTiming) != hipSuccess) { release_ctx(E, c); return false; }
        if (user && hipStreamWaitEvent(c->stream, fork, 0) != hipSuccess) { release_ctx(E, c); return false; }
        return true;
    };
    auto lease = [&]() -> Ctx* {
        if (cs.size() < (size_t)(2 * MAXG)) {
            std::unique_ptr<Ctx> c;
            if (!lease_new(c)) return nullptr;
            cs.push_back(std::move(c));
            return cs.back().get();
        }
        Ctx* c = cs[next_slot++ % cs.size()].get();     // always taken in pairs from an even-sized pool: the two of a group are distinct
        tl_cu_budget = c->cu_budget;
        return c;
    };
    rc = 0;
    int pend = -1;
    for (int i = 0; i <= n && !rc; i++) {
        const bool copy = i < n && (timestep[i] == 0.f || timestep[i] == 1.f);
        if (i < n && copy) {             // rife.cpp:2470-2480: an input frame unchanged - a D2D copy, no workspace; on the caller's stream when there is one
            hipStream_t cst = user;
            if (!cst) {
                if (!copy_ctx && !lease_new(copy_ctx)) { rc = fail(RIFE_HIP_EHIP, "rife_hip_process_device_batch: no workspace (" + g_err + ")"); break; }
                cst = copy_ctx->stream;
            }
            if (copy_frame_device(cst, timestep[i] == 0.f ? d_in0[i] : d_in1[i], d_out[i], w, h, pixfmt)) rc = fail(RIFE_HIP_EHIP, "copy failed");
            continue;
        }
        if (i < n && pend < 0) { pend = i; continue; }
        if (pend < 0) break;
        Ctx* a = lease(); Ctx* b = (a && i < n) ? lease() : nullptr;      // the odd pair left over is the call's LAST work item: one workspace, no partner
        if (!a || (i < n && !b)) { rc = fail(RIFE_HIP_EHIP, "rife_hip_process_device_batch: no workspace (" + g_err + ")"); break; }
        if (i < n) {            // group (pend, i)
            Ctx* g2[2] = {a, b};
            const uint8_t* p0[2] = {(const uint8_t*)d_in0[pend], (const uint8_t*)d_in0[i]};
            const uint8_t* p1[2] = {(const uint8_t*)d_in1[pend], (const uint8_t*)d_in1[i]};
            const float ts[2] = {timestep[pend], timestep[i]};
            uint8_t* po[2] = {(uint8_t*)d_out[pend], (uint8_t*)d_out[i]};
            rc = run_v4_group(*E, g2, 2, p0, p1, ts, po);
        } else {
            tl_cu_budget = a->cu_budget;
            rc = run_v4_replay(*E, *a, (const uint8_t*)d_in0[pend], (const uint8_t*)d_in1[pend], timestep[pend], (uint8_t*)d_out[pend]);
        }
        pend = -1;
    }
    // join: the caller's stream continues after every internal stream (also after an error: nothing may still run on the frames when we return control of them)
    if (copy_ctx) cs.push_back(std::move(copy_ctx));
    for (auto& c : cs) {
        if (!user) { if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(RIFE_HIP_EHIP, "stream sync failed"); }
        else if (hipEventRecord(c->ev_group, c->stream) != hipSuccess || hipStreamWaitEvent(user, c->ev_group, 0) != hipSuccess) { (void)hipStreamSynchronize(c->stream); if (!rc) rc = fail(RIFE_HIP_EHIP, "join failed"); }
    }
    for (auto& c : cs) release_ctx(E, c);
    return rc;
}
int rife_hip_process_device_batch(const rife_hip_t* E, int n, const void* const* d_in0, const void* const* d_in1, const float* timestep,
                                  void* const* d_out, int w, int h, void* hip_stream) {
    return guarded("rife_hip_process_device_batch", [&] { return rife_hip_process_device_batch_impl(E, n, d_in0, d_in1, timestep, d_out, w, h, hip_stream); });
}
int rife_hip_process_device_batch_px(const rife_hip_t* E, int n, const void* const* d_in0, const void* const* d_in1, const float* timestep,
                                     void* const* d_out, int w, int h, int pixfmt, void* hip_stream) {
    int rc;
    if ((rc = px_precheck(pixfmt, true, w, h))) return rc;
    return guarded("rife_hip_process_device_batch_px", [&] { return rife_hip_process_device_batch_impl(E, n, d_in0, d_in1, timestep, d_out, w, h, hip_stream, pixfmt); });
}

// ---- streams that own a part of the chip (include/rife_hip.h) ----
int rife_hip_stream_create(const rife_hip_t* E, int part, int nparts, void** hip_stream) {
    if (hip_stream) *hip_stream = nullptr;
    if (!E || !hip_stream) return fail(RIFE_HIP_EINVAL, "null argument");
    int rc;
    if ((rc = check_device(E->gpuid))) return rc;
    const int ncu = device_cus(true);
    if (nparts < 1 || nparts > ncu || part < 0 || part >= nparts) return fail(RIFE_HIP_EINVAL, "bad partition");
    hipStream_t st = nullptr;
    int mine = 0;
    const hipError_t e = create_part_stream(part, nparts, &st, &mine);
    if (e != hipSuccess)
        return fail(RIFE_HIP_EHIP, std::string(nparts == 1 ? "hipStreamCreateWithFlags(&st, hipStreamNonBlocking): " : "hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()): ") + hipGetErrorString(e));
    std::lock_guard<std::mutex> g(E->mu);
    E->part_streams[(void*)st] = mine;
    *hip_stream = (void*)st;
    return 0;
}
int rife_hip_stream_destroy(const rife_hip_t* E, void* hip_stream) {
    if (!E || !hip_stream) return fail(RIFE_HIP_EINVAL, "null argument");
    int rc;
    if ((rc = check_device(E->gpuid))) return rc;
    {
        std::lock_guard<std::mutex> g(E->mu);
        auto it = E->part_streams.find(hip_stream);
        if (it == E->part_streams.end()) return fail(RIFE_HIP_EINVAL, "not a stream of rife_hip_stream_create");
        E->part_streams.erase(it);
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    {
        std::lock_guard<std::mutex> g(E->mu);
        E->stream_ctx.erase(hip_stream);                                 // its workspace
    }
    HIPCHK(hipStreamDestroy((hipStream_t)hip_stream));
    return 0;
}

// ---- page-locked host frames (include/rife_hip.h) ----
void* rife_hip_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { g_err = "hipHostMalloc failed"; return nullptr; }
    return p;
}
void rife_hip_host_free(void* p) { if (p) (void)hipHostFree(p); }
int rife_hip_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) return fail(RIFE_HIP_EINVAL, "null range");
    HIPCHK(hipHostRegister(p, bytes, hipHostRegisterPortable));
    return 0;
}
int rife_hip_host_unregister(void* p) {
    if (!p) return fail(RIFE_HIP_EINVAL, "null pointer");
    HIPCHK(hipHostUnregister(p));
    return 0;
}

int rife_hip_profile_enable(rife_hip_t* E, int on) {
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    E->prof.collect();
    E->prof.on = on != 0;
    if (on) {
        std::lock_guard<std::mutex> g(E->prof.mu);
        std::fill(E->prof.ms.begin(), E->prof.ms.end(), 0.0);
        std::fill(E->prof.flops.begin(), E->prof.flops.end(), 0.0);
        std::fill(E->prof.launches.begin(), E->prof.launches.end(), 0LL);
    }
    return 0;
}

int rife_hip_profile_read(rife_hip_t* E, char* names, size_t names_cap, double* total_ms, long long* launches, double* flops, int max_classes) {
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    E->prof.collect();
    std::lock_guard<std::mutex> g(E->prof.mu);
    std::string all;
    int n = std::min<int>(max_classes, (int)E->prof.names.size());
    for (int i = 0; i < n; i++) {
        all += E->prof.names[i]; all += '\n';
        total_ms[i] = E->prof.ms[i]; launches[i] = E->prof.launches[i]; flops[i] = E->prof.flops[i];
    }
    if (names && names_cap) { std::strncpy(names, all.c_str(), names_cap - 1); names[names_cap - 1] = 0; }
    return n;
}

#ifdef RIFE_HIP_TEST_BUILD      // ======== include/rife_hip_test.h: test and bench builds only ========
// ---- stage tap: flow{fi} with optional injection of flow0..flow{n_inject-1} (rife.cpp:2653-2669) -------------
static int rife_hip_v4_extract_flow_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, int fi,
                                         const float* const* inject, int n_inject, float* out6chw, int pixfmt) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (!E->v4) return fail(RIFE_HIP_EINVAL, "stage taps exist for the rife-v4 family only");
    if (pix_bpp(pixfmt) == 0) return fail(RIFE_HIP_EINVAL, "unknown pixel format");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if (fi < 0 || fi > 3 || n_inject < 0 || n_inject > fi) return fail(RIFE_HIP_EINVAL, "bad stage index");
    if ((rc = check_device(E->gpuid))) return rc;
    Ctx c;
    if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) return fail(RIFE_HIP_EHIP, "hipStreamCreate failed");
    c.own_stream = true;
    if ((rc = ensure_ctx(c, w, h, pixfmt, E->pad()))) return rc;
    const size_t nbytes = frame_bytes(w, h, pixfmt);
    HIPCHK(hipMemcpyAsync(c.d_in0, in0, nbytes, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipMemcpyAsync(c.d_in1, in1, nbytes, hipMemcpyHostToDevice, c.stream));
    launch_preproc(c.stream, c.d_in0, c.w, c.h, c.img0, c.wp, c.hp, pixfmt);
    launch_preproc(c.stream, c.d_in1, c.w, c.h, c.img1, c.wp, c.hp, pixfmt);
    float* tmp = nullptr;
    if ((rc = dalloc(c, tmp, (size_t)c.wp * c.hp * 6))) return rc;
    const int nc = E->v40 ? 5 : 6;      // channels of blob flow{b}: rife-v4.6 PixelShuffle output 6, rife-v4 deconv output 5
    for (int b = 0; b <= fi; b++) {
        const int s = E->flow_div(b), Hb = c.hp / s, Wb = c.wp / s;
        if (b < n_inject) {
            HIPCHK(hipMemcpyAsync(tmp, inject[b], (size_t)Hb * Wb * nc * 4, hipMemcpyHostToDevice, c.stream));
            hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(Wb, Hb), dim3(256), 0, c.stream, tmp, c.flow[b], nc, Hb, Wb, 8);
        } else {
            if ((rc = run_block_convs(*E, c, b, timestep))) return rc;
        }
        if (b < fi && (rc = run_flow_update(*E, c, b))) return rc;
    }
    const int s = E->flow_div(fi), Hb = c.hp / s, Wb = c.wp / s;
    hipLaunchKernelGGL(k_nhwc_to_chw, grid2d(Wb, Hb), dim3(256), 0, c.stream, c.flow[fi], tmp, nc, Hb, Wb, 8);
    HIPCHK(hipMemcpyAsync(out6chw, tmp, (size_t)Hb * Wb * nc * 4, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return 0;
}
int rife_hip_v4_extract_flow(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, int fi,
                             const float* const* inject, int n_inject, float* out6chw) {
    return rife_hip_v4_extract_flow_impl(E, in0, in1, w, h, timestep, fi, inject, n_inject, out6chw, RIFE_HIP_PIX_RGB8);
}
int rife_hip_v4_extract_flow_px(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep, int fi, const float* const* inject,
                                int n_inject, float* out6chw, int pixfmt) {
    if (!in0 || !in1 || !out6chw) return fail(RIFE_HIP_EINVAL, "null frame / output pointer");
    try { return rife_hip_v4_extract_flow_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, fi, inject, n_inject, out6chw, pixfmt); }
    catch (const std::exception& e) { return fail(RIFE_HIP_EINVAL, std::string("v4_extract_flow_px: ") + e.what()); }
}

// ---- parity taps of the gather code (round 3): the 12-channel block input and the tail of the graph, on injected flows --------------------
// Shared prologue: frames -> padded RGBX, then for every block k < n_inject the injected blob flow{k} goes through the hot path's own
// k_flow_update into F, M (flownet.param:47-58, 99-105, 152-158).
// `pending` != null: as in run_v4, the update of the LAST injected flow is left to the fused stem of the next block where the product does so
// (flow_update_fused_into); *pending is then that flow.
// `updates` false (tap 6): the injected flows are placed and F, M are left to the caller.
static int tap_prologue(const rife_hip_t* E, Ctx& c, const uint8_t* in0, const uint8_t* in1, int w, int h, const float* const* inject, int n_inject, float*& tmp,
                        const float** pending = nullptr, int pixfmt = RIFE_HIP_PIX_RGB8, bool updates = true) {
    int rc;
    if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) return fail(RIFE_HIP_EHIP, "hipStreamCreate failed");
    c.own_stream = true;
    if ((rc = ensure_ctx(c, w, h, pixfmt, E->pad()))) return rc;
    const size_t nbytes = frame_bytes(w, h, pixfmt);
    HIPCHK(hipMemcpyAsync(c.d_in0, in0, nbytes, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipMemcpyAsync(c.d_in1, in1, nbytes, hipMemcpyHostToDevice, c.stream));
    launch_preproc(c.stream, c.d_in0, c.w, c.h, c.img0, c.wp, c.hp, pixfmt);
    launch_preproc(c.stream, c.d_in1, c.w, c.h, c.img1, c.wp, c.hp, pixfmt);
    if ((rc = dalloc(c, tmp, (size_t)c.wp * c.hp * 16))) return rc;
    for (int k = 0; k < n_inject; k++) {
        const int s = E->blk[k].scale, Hb = c.hp / s, Wb = c.wp / s;
        HIPCHK(hipMemcpyAsync(tmp, inject[k], (size_t)Hb * Wb * 6 * 4, hipMemcpyHostToDevice, c.stream));
        hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(Wb, Hb), dim3(256), 0, c.stream, tmp, c.flow[k], 6, Hb, Wb, 8);
        if (!updates) continue;
        if (pending && k == n_inject - 1 && k < 3 && flow_update_fused_into(*E, c, k + 1)) { *pending = c.flow[k]; continue; }
        if (k < 3 && (rc = run_flow_update(*E, c, k))) return rc;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// what = 0: block input of IFBlock b (1..3; blobs 99 / 199 / 262 of models/rife-v4.6/flownet.param:62, 115, 165) as k_assemble<S> computes it
//           (the unfused form of the same assemble_pixel<S> / warp_rgbx code); b = 0 (n_inject = 0): the 7-channel input of block 0 (flownet.param:9-10) from
//           k_assemble0 / k_assemble0_d10 / k_assemble0_s<16, D>, 7 x hp/S x wp/S;
// what = 1: the same tensor read back THROUGH THE PRODUCT'S FUSED STEM KERNEL stem0_fused_kernel<S, ...> (stem_fused.h), which keeps it in
//           LDS only: the kernel is run with one-hot weights (output channel 12 p + k = input channel k under tap (1 + p / 2, 1 + p % 2), bias 0,
//           slope 1), so that its stride-2 output holds the block input's four pixel parities; the split-f16 matrix path returns hi + lo of
//           every value, i.e. the value to 2^-22 relative;
// what = 2: blob out0 (flownet.param:217) before the postproc, from the unfused float tail k_final_float (b ignored; n_inject = 4);
// what = 4 / 3: F, M as block b's stem reads them: after k_flow_update / written by the stem that applies the update of flow{b-1} itself.
// what = 5: block 3's input through stem_rs_kernel, the product's kernel for that block (see below).
// what = 6: F, M as k_flow_cascade<b> (flow_cascade.h) writes them from the b injected flows alone, b = 2 / 3; what = 4 is its sequential reference.
// what = 7: the first S16 trunk tensor of block b (0..3), raw, after the block's stems as run_block_convs runs them (n_inject = b).
// out: planar CHW fp32, 12 x hp/S x wp/S (what 0, 1) or 3 x hp x wp (what 2).  n_inject must be b (what 0, 1) or 4 (what 2).
// Flow scale 2: S = 16, 8, 4, 2 and frames padded to 64n (E->blk[b].scale, E->pad()).  what = 0, 1, 4, 7 run the mode's own launches (run_assemble, the
// stem0_fused_kernel instantiations of run_block_convs' flow-scale-2 branch, the three plain k_flow_update launches); what = 2, 3, 5, 6 are kernels of the
// scale-1 schedule that the product never launches in this mode: -RIFE_HIP_EINVAL.
static int rife_hip_v4_tap_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, int what, int b,
                                const float* const* inject, int n_inject, float* out, int pixfmt = RIFE_HIP_PIX_RGB8) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (!E->v4 || E->v40) return fail(RIFE_HIP_EINVAL, "the gather taps exist for the rife-v4.6 graph only");
    if (pix_bpp(pixfmt) == 0) return fail(RIFE_HIP_EINVAL, "unknown pixel format");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if (pixfmt && what == 3) return fail(RIFE_HIP_EINVAL, "tap 3 (an A/B form the product does not run) is served for RGB8 frames only");
    if (what < 0 || what > 7) return fail(RIFE_HIP_EINVAL, "bad tap");
    if (E->fscale != 1) {      // kernels of the scale-1 schedule only: nothing the product runs at this divisor would be under test
        if (what == 2) return fail(RIFE_HIP_EINVAL, "tap 2: the unfused float tail (k_final_float) is a scale-1 kernel; at flow scale 2 the tail is k_final_scaled (rife_hip_v4_process_injected_px)");
        if (what == 3) return fail(RIFE_HIP_EINVAL, "tap 3: no stem applies a flow update at flow scale 2 (the fused update is a scale-1 schedule)");
        if (what == 5) return fail(RIFE_HIP_EINVAL, "tap 5: the row-streaming stem kernel (stem_rs) serves block 3 at scale 1 only; at flow scale 2 block 3 runs the fused tile stem");
        if (what == 6) return fail(RIFE_HIP_EINVAL, "tap 6: the flow cascade is a scale-1 schedule; at flow scale 2 the updates are three plain launches (tap 4)");
    }
    if (what == 7 && pixfmt) return fail(RIFE_HIP_EINVAL, "tap 7 (the block stems) is served for RGB8 frames only");
    if (what == 6 && b != 2 && b != 3) return fail(RIFE_HIP_EINVAL, "the flow cascade runs after block 1 (b = 2) or block 2 (b = 3)");
    if (what == 5 && b != 3) return fail(RIFE_HIP_EINVAL, "the row-streaming stem kernel serves block 3");
    if (what == 2 ? n_inject != 4 : (b < ((what == 7 || what == 0) ? 0 : 1) || b > 3 || n_inject != b)) return fail(RIFE_HIP_EINVAL, "bad block / injection count");
    if ((rc = check_device(E->gpuid))) return rc;
    Ctx c; float* tmp = nullptr;
    const float* pending = nullptr;
    if ((rc = tap_prologue(E, c, in0, in1, w, h, inject, n_inject, tmp, (what == 1 || what == 3 || what == 7) ? &pending : nullptr, pixfmt, what != 6))) return rc;
    hipStream_t st = c.stream;
    if (what == 7) {
        // Block b's stems as a plain pass runs them (run_block_convs with PH_STEMS: run_assemble + stem-0 + stem-1 for block 0, stem0_fused_kernel +
        // conv_h2s2_kernel<NS, true> for blocks 1 - 3, stem_rs_kernel where block_on_stem_rs says so), then the first S16 trunk tensor c.P[b][0], whole and raw:
        // rife_hip_op_s16_geom(C of the block, hp / 4 scale, wp / 4 scale) bytes.
        if (!block_on_s16(*E, c, b)) return fail(RIFE_HIP_EINVAL, "tap 7: this block does not run on S16 trunk tensors at this frame size");
        if ((rc = run_block_convs(*E, c, b, timestep, nullptr, nullptr, PH_STEMS, pending))) return rc;
        const rife_hip::Block& B7 = E->blk[b];
        const size_t nb = S16Geom(c.hp / B7.scale / 4, c.wp / B7.scale / 4).bytes(B7.c);
        HIPCHK(hipMemcpyAsync(out, c.P[b][0], nb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    // what = 3 / 4: F (4 channels) and M as block b's stem finds them, [5][hp][wp]: 4 = after k_flow_update, 3 = as written by the stem that applies
    // the last update itself (only where the product fuses it: EINVAL otherwise)
    auto copy_fm = [&](const float4* F, const float* M) -> int {
        hipLaunchKernelGGL(k_nhwc_to_chw, grid2d(c.wp, c.hp), dim3(256), 0, st, reinterpret_cast<const float*>(F), tmp, 4, c.hp, c.wp, 4);
        HIPCHK(hipGetLastError());
        const size_t P = (size_t)c.wp * c.hp;
        HIPCHK(hipMemcpyAsync(out, tmp, P * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(out + 4 * P, M, P * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    if (what == 4) return copy_fm(c.F, c.M);
    if (what == 6) {
        if (b == 2) launch_flow_cascade<2>(st, c.flow[0], c.flow[1], nullptr, c.F, c.M, c.wp, c.hp);
        else launch_flow_cascade<3>(st, c.flow[0], c.flow[1], c.flow[2], c.F, c.M, c.wp, c.hp);
        HIPCHK(hipGetLastError());
        return copy_fm(c.F, c.M);
    }
    if (what == 5) {
        // Block 3's input THROUGH THE PRODUCT'S ROW-STREAMING STEM KERNEL stem_rs_kernel (stem_rs.h): both of its convolutions run with one-hot
        // weights.  Stem 0: output channel 12 j + k = input channel k under tap (1 + g, 1 + j) (pixel parity p = 2 g + j of the block input; two
        // parities per launch); stem 1: output channel = input channel under tap (ty, tx) in {1, 2}^2 (the four parities of the half-resolution
        // tensor).  Eight launches return every pixel of the 12-channel block input once; each value passed the split-f16 matrix path twice
        // (hi + lo of hi + lo: 2^-21 relative).  Bias 0, slope 1.
        const int Hq = c.hp / 4, Wq = c.wp / 4;
        const S16Geom G(Hq, Wq);
        const size_t nb = G.bytes(64), pl = G.plane();
        unsigned char* dout = nullptr; uint16_t *dw0 = nullptr, *dw1 = nullptr; float *dbias = nullptr, *dslope = nullptr;
        if ((rc = dalloc(c, dout, nb)) || (rc = dalloc(c, dw0, (size_t)9 * 2 * 32 * 8)) || (rc = dalloc(c, dw1, (size_t)2 * 9 * 2 * 64 * 8)) ||
            (rc = dalloc(c, dbias, 64)) || (rc = dalloc(c, dslope, 64))) return rc;
        std::vector<float> hz(64, 0.f), ho(64, 1.f);
        HIPCHK(hipMemcpyAsync(dbias, hz.data(), 256, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dslope, ho.data(), 256, hipMemcpyHostToDevice, st));
        std::vector<unsigned char> host(nb);
        int inv[32];                                                     // row of a 32-row block that holds channel ch (pack_weights_h2_perm)
        for (int i = 0; i < 32; i++) inv[s16_row_channel(i)] = i;
        for (int g = 0; g < 2; g++)
            for (int ty = 1; ty <= 2; ty++)
                for (int tx = 1; tx <= 2; tx++) {
                    std::vector<uint16_t> h0((size_t)9 * 2 * 32 * 8, 0), h1((size_t)2 * 9 * 2 * 64 * 8, 0);
                    for (int j = 0; j < 2; j++)
                        for (int k = 0; k < 12; k++) h0[(((size_t)((1 + g) * 3 + 1 + j) * 2 + k / 8) * 32 + 12 * j + k) * 8 + k % 8] = f2h(1.f);
                    for (int oc = 0; oc < 24; oc++)
                        h1[((((size_t)(oc / 16) * 9 + ty * 3 + tx) * 2 + (oc % 16) / 8) * 64 + inv[oc]) * 8 + oc % 8] = f2h(1.f);
                    HIPCHK(hipMemcpyAsync(dw0, h0.data(), h0.size() * 2, hipMemcpyHostToDevice, st));
                    HIPCHK(hipMemcpyAsync(dw1, h1.data(), h1.size() * 2, hipMemcpyHostToDevice, st));
                    HIPCHK(hipMemsetAsync(dout, 0, nb, st));
                    StemRsArgs a;
                    a.img0 = c.img0; a.img1 = c.img1; a.F = c.F; a.M = c.M; a.w0 = dw0; a.bias0 = dbias; a.slope0 = dslope; a.w1 = dw1; a.bias1 = dbias; a.slope1 = dslope;
                    a.out = dout; a.timestep = timestep; a.tsp = nullptr; a.wp = c.wp; a.hp = c.hp; a.Hq = Hq; a.Wq = Wq; a.pitch = G.pitch; a.plane = G.plane();
                    a.nunits = ((Wq + SRS_SW - 1) / SRS_SW) * Hq;
                    const int nwg = std::min(2 * device_cus(), a.nunits);
                    if (pix_deep(pixfmt)) rc = launch<stem_rs_kernel<0, 10>>("hipGetLastError()", dim3(nwg), dim3(SRS_NTHR), SRS_LDS, st, a);
                    else rc = launch<stem_rs_kernel<0>>("hipGetLastError()", dim3(nwg), dim3(SRS_NTHR), SRS_LDS, st, a);
                    if (rc) return rc;
                    HIPCHK(hipMemcpyAsync(host.data(), dout, nb, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                    for (int j = 0; j < 2; j++)
                        for (int k = 0; k < 12; k++) {
                            const int oc = 12 * j + k;
                            const _Float16* hi = reinterpret_cast<const _Float16*>(host.data() + (size_t)(2 * (oc / 16)) * pl);
                            const _Float16* lo = reinterpret_cast<const _Float16*>(host.data() + (size_t)(2 * (oc / 16) + 1) * pl);
                            for (int q = 0; q < Hq; q++)
                                for (int x = 0; x < Wq; x++) {
                                    const size_t e = ((size_t)(q + 1) * G.pitch + x + 1) * 16 + oc % 16;
                                    out[((size_t)k * c.hp + 4 * q + 2 * (ty - 1) + g) * c.wp + 4 * x + 2 * (tx - 1) + j] = (float)hi[e] + (float)lo[e];
                                }
                        }
                }
        return 0;
    }
    if (what == 3 && !pending) return fail(RIFE_HIP_EINVAL, "the flow update before this block is not fused into its stem");
    if (what == 2) {
        float4* outf = nullptr;
        if ((rc = dalloc(c, outf, (size_t)c.wp * c.hp))) return rc;
        const int nch = pixfmt == RIFE_HIP_PIX_RGBA8 ? 4 : 3;      // RGBA8: the alpha plane before quantisation as a fourth channel
        if (pix_deep(pixfmt)) hipLaunchKernelGGL(k_final_float_d10, grid2d(c.wp, c.hp), dim3(256), 0, st, c.img0, c.img1, c.F, c.M, c.flow[3], outf, c.wp, c.hp);
        else if (nch == 4) hipLaunchKernelGGL(k_final_float_a, grid2d(c.wp, c.hp), dim3(256), 0, st, c.img0, c.img1, c.F, c.M, c.flow[3], outf, c.wp, c.hp);
        else hipLaunchKernelGGL(k_final_float, grid2d(c.wp, c.hp), dim3(256), 0, st, c.img0, c.img1, c.F, c.M, c.flow[3], outf, c.wp, c.hp);
        hipLaunchKernelGGL(k_nhwc_to_chw, grid2d(c.wp, c.hp), dim3(256), 0, st, reinterpret_cast<const float*>(outf), tmp, nch, c.hp, c.wp, 4);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, tmp, (size_t)c.wp * c.hp * nch * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    const rife_hip::Block& B = E->blk[b];
    const int s = B.scale, Hb = c.hp / s, Wb = c.wp / s;
    if (what == 0) {
        if ((rc = run_assemble(*E, c, b, timestep))) return rc;
        const int nch = b == 0 ? 7 : 12, ld = b == 0 ? 8 : 16;      // block 0: X is NHWC8 {in0.rgb, in1.rgb, t, 0}
        hipLaunchKernelGGL(k_nhwc_to_chw, grid2d(Wb, Hb), dim3(256), 0, st, c.X, tmp, nch, Hb, Wb, ld);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, tmp, (size_t)Hb * Wb * nch * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    // what == 1: the fused stem kernel of the product with one-hot weights
    const int NT = 32 * B.stem0.NS, cout = B.c / 2, per = std::min(4, cout / 12), nlaunch = (4 + per - 1) / per;
    const int Ho = Hb / 2, Wo = Wb / 2;
    std::vector<float> hbias(64, 0.f), hslope(64, 1.f), host((size_t)Ho * Wo * cout);
    float *dbias = nullptr, *dslope = nullptr; uint16_t* dw = nullptr;
    if ((rc = dalloc(c, dbias, 64)) || (rc = dalloc(c, dslope, 64)) || (rc = dalloc(c, dw, (size_t)9 * 2 * NT * 8))) return rc;
    HIPCHK(hipMemcpyAsync(dbias, hbias.data(), 256, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dslope, hslope.data(), 256, hipMemcpyHostToDevice, st));
    for (int l = 0; l < nlaunch; l++) {
        std::vector<uint16_t> hw((size_t)9 * 2 * NT * 8, 0);
        for (int q = 0; q < per && l * per + q < 4; q++) {
            const int p = l * per + q, t = (1 + p / 2) * 3 + 1 + p % 2;
            for (int k = 0; k < 12; k++) hw[(((size_t)t * 2 + k / 8) * NT + 12 * q + k) * 8 + k % 8] = f2h(1.f);
        }
        HIPCHK(hipMemcpyAsync(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice, st));
        StemFusedArgs fa;
        fa.img0 = c.img0; fa.img1 = c.img1; fa.F = c.F; fa.M = c.M; fa.wpk = dw; fa.bias = dbias; fa.slope = dslope;
        fa.out = c.S1; fa.timestep = timestep; fa.tsp = nullptr; fa.wp = c.wp; fa.hp = c.hp; fa.Ho = Ho; fa.Wo = Wo; fa.out_ld = cout; fa.Cout = cout;
        fa.tiles_x = (Wo + 31) / 32;
        const dim3 grid(fa.tiles_x * ((Ho + 3) / 4));
        const char* const lname = "hipGetLastError()";      // the error text this site has always had
        if (E->fscale == 2) {      // the instantiations of run_block_convs' flow-scale-2 branch, selected as it selects them
            const bool deep = pix_deep(pixfmt);
            if (pending) return fail(RIFE_HIP_EINVAL, "no fused flow update at flow scale 2");
            if (s == 8 && B.stem0.NS == 2) rc = deep ? launch<stem0_fused_kernel<8, 2, 0, 0, 10>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa)
                                                     : launch<stem0_fused_kernel<8, 2>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
            else if (s == 4 && B.stem0.NS == 2) rc = deep ? launch<stem0_fused_kernel<4, 2, 0, 0, 10>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa)
                                                          : launch<stem0_fused_kernel<4, 2>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
            else if (s == 2 && B.stem0.NS == 1) rc = deep ? launch<stem0_fused_kernel<2, 1, 0, 0, 10>>(lname, grid, dim3(512), stemf_lds_bytes<1>(), st, fa)
                                                          : launch<stem0_fused_kernel<2, 1>>(lname, grid, dim3(512), stemf_lds_bytes<1>(), st, fa);
            else return fail(RIFE_HIP_EINVAL, "no fused stem for this block at flow scale 2");
        } else if (pending && pix_deep(pixfmt)) {
            fa.pend.flow = pending; fa.pend.Fw = c.F2; fa.pend.Mw = c.M2;
            if (s == 2) rc = launch<stem0_fused_kernel<2, 2, 0, 1, 10>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
            else rc = launch<stem0_fused_kernel<1, 1, 256, 1, 10>>(lname, grid, dim3(512), stemf_lds_bytes<1, 256>(), st, fa);
        } else if (pix_deep(pixfmt)) {
            if (s == 4) rc = launch<stem0_fused_kernel<4, 2, 0, 0, 10>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
            else if (s == 2) rc = launch<stem0_fused_kernel<2, 2, 0, 0, 10>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
            else rc = launch<stem0_fused_kernel<1, 1, 256, 0, 10>>(lname, grid, dim3(512), stemf_lds_bytes<1, 256>(), st, fa);
        } else if (pending) {                                                   // every launch reads the old F, M and writes the same new ones
            fa.pend.flow = pending; fa.pend.Fw = c.F2; fa.pend.Mw = c.M2;
            if (s == 2) rc = launch<stem0_fused_kernel<2, 2, 0, true>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
            else rc = launch<stem0_fused_kernel<1, 1, 256, true>>(lname, grid, dim3(512), stemf_lds_bytes<1, 256>(), st, fa);
            if (what == 3) return rc ? rc : copy_fm(c.F2, c.M2);
        } else if (s == 4) rc = launch<stem0_fused_kernel<4, 2>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
        else if (s == 2) rc = launch<stem0_fused_kernel<2, 2>>(lname, grid, dim3(512), stemf_lds_bytes<2>(), st, fa);
        else rc = launch<stem0_fused_kernel<1, 1, 256>>(lname, grid, dim3(512), stemf_lds_bytes<1, 256>(), st, fa);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(host.data(), c.S1, host.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int q = 0; q < per && l * per + q < 4; q++) {
            const int p = l * per + q, py = p / 2, px = p % 2;
            for (int k = 0; k < 12; k++)
                for (int y = 0; y < Ho; y++)
                    for (int x = 0; x < Wo; x++)
                        out[((size_t)k * Hb + 2 * y + py) * Wb + 2 * x + px] = host[((size_t)y * Wo + x) * cout + 12 * q + k];
        }
    }
    return 0;
}
int rife_hip_v4_tap(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep, int what, int b,
                    const float* const* inject, int n_inject, float* out) {      // nothing may throw across the C boundary
    if (!in0 || !in1 || !out) return fail(RIFE_HIP_EINVAL, "null frame / output pointer");
    if (n_inject > 0 && !inject) return fail(RIFE_HIP_EINVAL, "n_inject > 0 without blobs");
    for (int k = 0; k < n_inject && k < 4; k++) if (!inject[k]) return fail(RIFE_HIP_EINVAL, "null injected blob");
    try { return rife_hip_v4_tap_impl(E, in0, in1, w, h, timestep, what, b, inject, n_inject, out); }
    catch (const std::exception& e) { return fail(RIFE_HIP_EINVAL, std::string("v4_tap: ") + e.what()); }
}
int rife_hip_v4_tap_px(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep, int what, int b, const float* const* inject,
                       int n_inject, float* out, int pixfmt) {
    if (!in0 || !in1 || !out) return fail(RIFE_HIP_EINVAL, "null frame / output pointer");
    if (n_inject > 0 && !inject) return fail(RIFE_HIP_EINVAL, "n_inject > 0 without blobs");
    for (int k = 0; k < n_inject && k < 4; k++) if (!inject[k]) return fail(RIFE_HIP_EINVAL, "null injected blob");
    try { return rife_hip_v4_tap_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, what, b, inject, n_inject, out, pixfmt); }
    catch (const std::exception& e) { return fail(RIFE_HIP_EINVAL, std::string("v4_tap_px: ") + e.what()); }
}

// The plain v4 pass with the first n_inject (0..3) blobs flow{k} injected instead of computed: the remaining blocks and the tail run on the
// product's own schedule (fused stems, fused tail of head_h2_kernel<EPI_FINAL>), so that flows which leave the frame by hundreds of pixels
// reach exactly the gather code a real pass runs.  out: w x h u8 RGB.
static int rife_hip_v4_process_injected_impl(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep,
                                             const float* const* inject, int n_inject, uint8_t* out, int pixfmt = RIFE_HIP_PIX_RGB8) {
    int rc;
    if ((rc = process_common(E, w, h, timestep))) return rc;
    if (!E->v4 || E->v40) return fail(RIFE_HIP_EINVAL, "flow injection into the plain pass exists for the rife-v4.6 graph only");
    // flow scale 2: flow3 may be injected too - block 3's update is applied by k_final_scaled, the kernel under test (blobs at the mode's sizes)
    if (n_inject < 0 || n_inject > (E->fscale == 2 ? 4 : 3)) return fail(RIFE_HIP_EINVAL, "bad injection count");
    if (pix_bpp(pixfmt) == 0) return fail(RIFE_HIP_EINVAL, "unknown pixel format");
    if (pixfmt != RIFE_HIP_PIX_RGB8 && E->fscale != 2) return fail(RIFE_HIP_EINVAL, "flow injection at flow scale 1 writes RGB8 frames only");
    if ((rc = pixfmt_supported(E, pixfmt))) return rc;
    if ((rc = check_device(E->gpuid))) return rc;
    Ctx c; float* tmp = nullptr;
    const float* pending = nullptr;
    if ((rc = tap_prologue(E, c, in0, in1, w, h, inject, n_inject, tmp, &pending, pixfmt))) return rc;
    const bool fuse_tail = E->fscale == 1 && trunk_h2() && E->blk[3].head.d_wh != nullptr;
    FinalArgs fin{c.img0, c.img1, c.F, c.M, c.d_out, c.w, c.h, c.wp, c.hp};
    for (int b = n_inject; b < 4; b++) {
        if ((rc = run_block_convs(*E, c, b, timestep, (b == 3 && fuse_tail) ? &fin : nullptr, nullptr, PH_ALL, pending))) return rc;
        pending = nullptr;
        if (b < 3 && flow_update_fused_into(*E, c, b + 1)) pending = c.flow[b];
        else if (b < 3 && (rc = run_flow_update(*E, c, b))) return rc;
    }
    if (E->fscale == 2) launch_final_scaled(c.stream, c, pixfmt, c.d_out);
    else if (!fuse_tail) hipLaunchKernelGGL(k_final, grid2d(c.w, c.h), dim3(256), 0, c.stream, c.img0, c.img1, c.F, c.M, c.flow[3], c.d_out, c.w, c.h, c.wp, c.hp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c.d_out, frame_bytes(w, h, pixfmt), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return 0;
}
int rife_hip_v4_process_injected(const rife_hip_t* E, const uint8_t* in0, const uint8_t* in1, int w, int h, float timestep,
                                 const float* const* inject, int n_inject, uint8_t* out) {      // nothing may throw across the C boundary
    if (!in0 || !in1 || !out) return fail(RIFE_HIP_EINVAL, "null frame / output pointer");
    if (n_inject > 0 && !inject) return fail(RIFE_HIP_EINVAL, "n_inject > 0 without blobs");
    for (int k = 0; k < n_inject && k < 4; k++) if (!inject[k]) return fail(RIFE_HIP_EINVAL, "null injected blob");
    try { return rife_hip_v4_process_injected_impl(E, in0, in1, w, h, timestep, inject, n_inject, out); }
    catch (const std::exception& e) { return fail(RIFE_HIP_EINVAL, std::string("v4_process_injected: ") + e.what()); }
}
int rife_hip_v4_process_injected_px(const rife_hip_t* E, const void* in0, const void* in1, int w, int h, float timestep,
                                    const float* const* inject, int n_inject, void* out, int pixfmt) {
    if (!in0 || !in1 || !out) return fail(RIFE_HIP_EINVAL, "null frame / output pointer");
    if (n_inject > 0 && !inject) return fail(RIFE_HIP_EINVAL, "n_inject > 0 without blobs");
    for (int k = 0; k < n_inject && k < 4; k++) if (!inject[k]) return fail(RIFE_HIP_EINVAL, "null injected blob");
    try { return rife_hip_v4_process_injected_impl(E, static_cast<const uint8_t*>(in0), static_cast<const uint8_t*>(in1), w, h, timestep, inject, n_inject, static_cast<uint8_t*>(out), pixfmt); }
    catch (const std::exception& e) { return fail(RIFE_HIP_EINVAL, std::string("v4_process_injected_px: ") + e.what()); }
}

#endif  // RIFE_HIP_TEST_BUILD

static int rife_hip_graph_check_impl(const char* base) {
    if (!base) return fail(RIFE_HIP_EINVAL, "null argument");
    GraphNet n;
    return graph_load(n, base, true);
}
int rife_hip_graph_check(const char* base) {
    return guarded("rife_hip_graph_check", [&] { return rife_hip_graph_check_impl(base); });
}

#ifdef RIFE_HIP_TEST_BUILD      // ======== include/rife_hip_test.h (continued) ========
int rife_hip_v4_flow_dims(const rife_hip_t* E, int w, int h, int fi, int* channels, int* fh, int* fw) {
    if (!E || !E->loaded || !E->v4) return fail(RIFE_HIP_EINVAL, "flow blobs exist for a loaded rife-v4 family engine only");
    if (fi < 0 || fi > 3 || w <= 0 || h <= 0 || !channels || !fh || !fw) return fail(RIFE_HIP_EINVAL, "bad argument");
    const int pad = E->pad(), wp = (w + pad - 1) / pad * pad, hp = (h + pad - 1) / pad * pad;
    *channels = E->v40 ? 5 : 6; *fh = hp / E->flow_div(fi); *fw = wp / E->flow_div(fi);
    return 0;
}

// ---- the generic graph executor on micro-graphs: the plan graph_load settles on (host only), and one graph_run with host blobs -----------------
// One text line per layer, tab-separated: name, kind, fold=<layer that executes it | ->, out=<blob the result goes to | ->,
// class=<profile class of a convolution | ->, padded=<1 when zero filters pad the output channels to a multiple of 4>
static void graph_plan(const GraphNet& N, std::string& s) {
    static const char* const kinds[] = {"Input", "Split", "Concat", "Crop", "Interp", "Convolution", "Deconvolution", "ConvolutionDirect", "PixelShuffle", "ReLU", "PReLU",
                                        "Sigmoid", "Clip", "BinaryOp", "Eltwise", "UnaryOp", "Pooling", "InnerProduct", "rife.Warp"};
    const std::vector<int> wr = graph_writers(N);
    for (const GLayer& L : N.layers) {
        const bool conv = L.kind == G_CONV || L.kind == G_DECONV, direct = L.kind == G_CONV_DIRECT;
        const int ob = L.folded ? -1 : L.out_blob;
        s += L.nl->name + "\t" + kinds[L.kind];
        s += std::string("\tfold=") + (L.folded ? N.layers[L.folded_into].nl->name : "-");
        s += std::string("\tout=") + (ob >= 0 && wr[ob] >= 0 ? N.blob_names[ob] : "-");
        s += std::string("\tclass=") + (conv ? L.conv.cls : direct ? "direct" : "-");
        s += std::string("\tpadded=") + (conv && L.nl->geti(0, 0) % 4 ? "1" : "0") + "\n";
    }
}

int rife_hip_graph_plan(const char* base, char* buf, size_t cap) {
    return guarded("rife_hip_graph_plan", [&] {
        if (!base || !buf || !cap) return fail(RIFE_HIP_EINVAL, "null argument");
        GraphNet n;
        int rc;
        if ((rc = graph_load(n, base, true))) return rc;
        std::string s;
        graph_plan(n, s);
        if (s.size() + 1 > cap) return fail(RIFE_HIP_EINVAL, "rife_hip_graph_plan: the plan needs " + std::to_string(s.size() + 1) + " bytes");
        std::memcpy(buf, s.c_str(), s.size() + 1);
        return 0;
    });
}

struct GraphEvalKept { std::string base; int gpuid = -1; std::unique_ptr<GraphNet> net; std::unique_ptr<GraphInst> inst; };
// the net and blob storage of the last rife_hip_graph_eval(keep = 1) call: the next call on the same files runs on them.  Heap-allocated and never destroyed: what
// a process leaves kept at exit must not be freed from a static destructor, after the HIP runtime has shut down.
static GraphEvalKept& g_eval_kept = *new GraphEvalKept;
static std::mutex g_eval_mu;

static int rife_hip_graph_eval_impl(int gpuid, const char* base, int n_in, const char* const* in_names, const float* const* in_chw, const int* in_dims, int n_out,
                                    const char* const* out_names, float* const* out_chw, const size_t* out_caps, int* out_dims, int keep) {
    if (!base || n_in < 0 || n_out <= 0 || (n_in && (!in_names || !in_chw || !in_dims)) || !out_names || !out_chw || !out_caps || !out_dims)
        return fail(RIFE_HIP_EINVAL, "rife_hip_graph_eval: null argument");
    for (int i = 0; i < n_in; i++)
        if (!in_names[i] || !in_chw[i] || in_dims[3 * i] <= 0 || in_dims[3 * i + 1] <= 0 || in_dims[3 * i + 2] <= 0) return fail(RIFE_HIP_EINVAL, "rife_hip_graph_eval: bad input blob");
    for (int i = 0; i < n_out; i++) if (!out_names[i] || !out_chw[i]) return fail(RIFE_HIP_EINVAL, "rife_hip_graph_eval: bad output blob");
    int rc;
    if ((rc = check_device(gpuid))) return rc;
    std::lock_guard<std::mutex> g(g_eval_mu);
    std::unique_ptr<GraphNet> net; std::unique_ptr<GraphInst> inst;
    if (g_eval_kept.net && g_eval_kept.base == base && g_eval_kept.gpuid == gpuid) { net = std::move(g_eval_kept.net); inst = std::move(g_eval_kept.inst); }
    g_eval_kept.net.reset(); g_eval_kept.inst.reset();
    if (!net) {
        net.reset(new GraphNet); inst.reset(new GraphInst);
        if ((rc = graph_load(*net, base))) return rc;
    }
    const GraphNet& N = *net; GraphInst& I = *inst;
    std::vector<std::string> wanted(out_names, out_names + n_out);
    if ((rc = graph_check_taps(N, std::vector<std::string>(in_names, in_names + n_in), wanted))) return rc;      // before anything is uploaded or launched
    const size_t nb = N.blob_names.size();
    if (I.v.size() != nb) { I.v.assign(nb, GView{nullptr, 0, 0, 0, 0}); I.owned.assign(nb, nullptr); I.cap.assign(nb, 0); }
    std::vector<std::pair<std::string, GView>> bound;
    std::vector<float> host;
    for (int i = 0; i < n_in; i++) {
        const int b = N.blob(in_names[i]);
        if (b < 0) return fail(RIFE_HIP_EMODEL, N.name + ": no blob named " + in_names[i]);
        const int c = in_dims[3 * i], h = in_dims[3 * i + 1], w = in_dims[3 * i + 2];
        if ((rc = g_alloc(I, b, c, h, w, h == 1 && w == 1, nullptr))) return rc;      // a 1 x 1 x C blob is a vector, like the outputs of Pooling / InnerProduct
        const GView v = I.v[b];
        host.assign((size_t)h * w * v.ld, 0.f);                                       // pad channels go up as zeros, as g_alloc left them
        for (int q = 0; q < c; q++)
            for (size_t p = 0; p < (size_t)h * w; p++) host[p * v.ld + q] = in_chw[i][(size_t)q * h * w + p];
        HIPCHK(hipMemcpy(v.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
        bound.emplace_back(in_names[i], v);
    }
    rife_hip E;                                                                      // graph_run wants the engine for its profiler only
    E.gpuid = gpuid;
    if ((rc = graph_run(E, N, I, nullptr, bound, wanted))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    for (int i = 0; i < n_out; i++) {
        const GView v = I.v[N.blob(out_names[i])];
        const size_t npix = (size_t)v.h * v.w;
        out_dims[3 * i] = v.c; out_dims[3 * i + 1] = v.h; out_dims[3 * i + 2] = v.w;
        if (npix * v.c > out_caps[i]) return fail(RIFE_HIP_EINVAL, N.name + ": blob " + out_names[i] + " has " + std::to_string(npix * v.c) + " elements, more than its buffer holds");
        host.resize(npix * v.ld);
        HIPCHK(hipMemcpy(host.data(), v.p, host.size() * 4, hipMemcpyDeviceToHost));
        for (int q = 0; q < v.c; q++)
            for (size_t p = 0; p < npix; p++) out_chw[i][(size_t)q * npix + p] = host[p * v.ld + q];
    }
    if (keep) { g_eval_kept.base = base; g_eval_kept.gpuid = gpuid; g_eval_kept.net = std::move(net); g_eval_kept.inst = std::move(inst); }
    return 0;
}
int rife_hip_graph_eval(int gpuid, const char* base, int n_in, const char* const* in_names, const float* const* in_chw, const int* in_dims, int n_out,
                        const char* const* out_names, float* const* out_chw, const size_t* out_caps, int* out_dims, int keep) {
    return guarded("rife_hip_graph_eval", [&] { return rife_hip_graph_eval_impl(gpuid, base, n_in, in_names, in_chw, in_dims, n_out, out_names, out_chw, out_caps, out_dims, keep); });
}

// ---- single-kernel entry points ------------------------------------------------------------------------------
static int op_conv_common(int gpuid, const float* x, int c, int h, int w, const float* weight, const float* bias, int outc, int stride,
                          bool deconv, int epi, const float* residual, const float* slope, float* out) {
    int rc;
    if ((rc = check_device(gpuid))) return rc;
    ConvLayer L;
    L.cin = c; L.cout = outc; L.stride = deconv ? 1 : stride; L.deconv = deconv; L.epi = epi;
    if ((rc = upload_layer(L, weight, bias, slope, 1.0f))) { free_layer(L); return rc; }
    const int ho = deconv ? 2 * h : (h + 2 - 3) / stride + 1, wo = deconv ? 2 * w : (w + 2 - 3) / stride + 1;
    const int ldi = L.cin_p;
    float *d_chw = nullptr, *d_x = nullptr, *d_y = nullptr, *d_r = nullptr, *d_o = nullptr;
    auto cleanup = [&]() { (void)hipFree(d_chw); (void)hipFree(d_x); (void)hipFree(d_y); (void)hipFree(d_r); (void)hipFree(d_o); free_layer(L); };
    const size_t nin = (size_t)c * h * w, nout = (size_t)outc * ho * wo;
    hipError_t e = hipMalloc(&d_chw, std::max(nin, nout) * 4);
    if (e == hipSuccess) e = hipMalloc(&d_x, (size_t)h * w * ldi * 4);
    if (e == hipSuccess) e = hipMalloc(&d_y, (size_t)ho * wo * outc * 4);
    if (e == hipSuccess) e = hipMalloc(&d_o, nout * 4);
    if (e == hipSuccess && residual) e = hipMalloc(&d_r, (size_t)ho * wo * outc * 4);
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, "hipMalloc failed"); }
    (void)hipMemcpy(d_chw, x, nin * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(w, h), dim3(256), 0, 0, d_chw, d_x, c, h, w, ldi);
    TensorView rv{d_r, outc, 0};
    if (residual) {
        (void)hipMemcpy(d_chw, residual, nout * 4, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(wo, ho), dim3(256), 0, 0, d_chw, d_r, outc, ho, wo, outc);
    }
    rc = launch_conv(L, {d_x, ldi, 0}, h, w, {d_y, outc, 0}, residual ? &rv : nullptr, 0);
    if (!rc) {
        hipLaunchKernelGGL(k_nhwc_to_chw, grid2d(wo, ho), dim3(256), 0, 0, d_y, d_o, outc, ho, wo, outc);
        e = hipMemcpy(out, d_o, nout * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op: ") + hipGetErrorString(e));
    }
    cleanup();
    return rc;
}

int rife_hip_op_conv3x3(int gpuid, const float* x, int c, int h, int w, const float* weight, const float* bias, int outc, int stride,
                        const float* residual, const float* slope, float* out) {
    if (stride != 1 && stride != 2) return fail(RIFE_HIP_EINVAL, "stride must be 1 or 2");
    return op_conv_common(gpuid, x, c, h, w, weight, bias, outc, stride, false, EPI_STORE, residual, slope, out);
}

int rife_hip_op_deconv4x4(int gpuid, const float* x, int c, int h, int w, const float* weight, const float* bias, int outc, const float* slope, float* out) {
    return op_conv_common(gpuid, x, c, h, w, weight, bias, outc, 2, true, EPI_DECONV, nullptr, slope, out);
}

int rife_hip_pool_state(const rife_hip_t* E, int* pooled, int* leased, int* high_water) {
    if (!E) return fail(RIFE_HIP_EINVAL, "null engine");
    std::lock_guard<std::mutex> g(E->mu);
    int hw = 1;
    for (int v : E->lease_hist) hw = std::max(hw, v);
    if (pooled) *pooled = (int)E->free_ctx.size();
    if (leased) *leased = E->leased;
    if (high_water) *high_water = hw;
    return 0;
}

int rife_hip_op_warp(int gpuid, const float* image, const float* flow, int c, int h, int w, float* out) {
    int rc;
    if ((rc = check_device(gpuid))) return rc;
    float *d_i = nullptr, *d_f = nullptr, *d_o = nullptr;
    const size_t n = (size_t)c * h * w;
    hipError_t e = hipMalloc(&d_i, n * 4);
    if (e == hipSuccess) e = hipMalloc(&d_f, (size_t)2 * h * w * 4);
    if (e == hipSuccess) e = hipMalloc(&d_o, n * 4);
    if (e == hipSuccess) e = hipMemcpy(d_i, image, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_f, flow, (size_t)2 * h * w * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_warp_chw, grid2d(w, h), dim3(256), 0, 0, d_i, d_f, d_o, c, h, w);
        e = hipMemcpy(out, d_o, n * 4, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_i); (void)hipFree(d_f); (void)hipFree(d_o);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_warp: ") + hipGetErrorString(e));
    return 0;
}

// ---- scaffolding of the single-kernel ops (here and in the engine_*.h sections that follow) ----
extern "C++" {      // templates cannot have C linkage
// a pre-processing kernel alone: a padded frame of wp x hp dwords filled with 0xa5 (the kernel writes the padding too), `launch(frame, wp, hp)`, the frame back to the host
template <typename F>
static hipError_t op_padded_rgb10(int w, int h, uint32_t* out_padded, F&& launch) {
    const int wp = align_up(w, 32), hp = align_up(h, 32);
    const size_t nout = (size_t)wp * hp * 4;
    void* d_o = nullptr;
    hipError_t e = hipMalloc(&d_o, nout);
    if (e == hipSuccess) e = hipMemset(d_o, 0xa5, nout);
    if (e == hipSuccess) {
        launch(static_cast<uint32_t*>(d_o), wp, hp);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(out_padded, d_o, nout, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_o);
    return e;
}
// a blend kernel alone: `launch(stream)` (its rc into lrc) on a non-blocking stream of its own, drained and destroyed before the planes are read back
template <typename F>
static hipError_t op_on_own_stream(int& lrc, F&& launch) {
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    lrc = launch(st);
    e = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    return e;
}
}  // extern "C++"

// the YUV kernels alone (yuv.h), in the form the host would pick for a frame at an aligned address: planes -> zero-padded 10:10:10 dwords (hp x wp),
// A2B10G10R10 (h x w) -> planes
int rife_hip_op_yuv_to_rgb10(int gpuid, const void* yuv, int w, int h, int pixfmt, uint32_t* out_padded) {
    int rc;
    if ((rc = pixfmt_check(pixfmt))) return rc;
    if (!pix_yuv(pixfmt) || !yuv || !out_padded || w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "op_yuv_to_rgb10: a YUV format, two arrays and a frame size");
    if ((rc = check_device(gpuid))) return rc;
    const size_t nin = frame_bytes(w, h, pixfmt);
    void* d_i = nullptr;
    hipError_t e = hipMalloc(&d_i, nin);
    if (e == hipSuccess) e = hipMemcpy(d_i, yuv, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = op_padded_rgb10(w, h, out_padded, [&](uint32_t* d_o, int wp, int hp) { launch_preproc_yuv(0, d_i, w, h, d_o, wp, hp, pixfmt); });
    (void)hipFree(d_i);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_yuv_to_rgb10: ") + hipGetErrorString(e));
    return 0;
}
int rife_hip_op_rgb10_to_yuv(int gpuid, const uint32_t* a2b10g10r10, int w, int h, int pixfmt, void* yuv_out) {
    int rc;
    if ((rc = pixfmt_check(pixfmt))) return rc;
    if (!pix_yuv(pixfmt) || !a2b10g10r10 || !yuv_out || w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "op_rgb10_to_yuv: a YUV format, two arrays and a frame size");
    if ((rc = check_device(gpuid))) return rc;
    const size_t nin = (size_t)w * h * 4, nout = frame_bytes(w, h, pixfmt);
    void *d_i = nullptr, *d_o = nullptr;
    hipError_t e = hipMalloc(&d_i, nin);
    if (e == hipSuccess) e = hipMalloc(&d_o, nout);
    if (e == hipSuccess) e = hipMemcpy(d_i, a2b10g10r10, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_postproc_yuv(0, static_cast<const uint32_t*>(d_i), w, h, d_o, pixfmt);
        e = hipMemcpy(yuv_out, d_o, nout, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_i); (void)hipFree(d_o);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_rgb10_to_yuv: ") + hipGetErrorString(e));
    return 0;
}

// ---- the S16 trunk kernels alone: raw S16 tensors in and out, the product's layer upload and the product's launchers (tests/test_gpu_trunk_ops.py) ----
int rife_hip_op_s16_geom(int C, int H, int W, int* pitch, int* rows, unsigned* plane_bytes, size_t* bytes) {
    if (C <= 0 || C % 16 || H <= 0 || W <= 0) return fail(RIFE_HIP_EINVAL, "op_s16_geom: whole 16-channel chunks of a non-empty pixel grid");
    const S16Geom G(H, W);
    if ((unsigned long long)G.rows * G.pitch * 32ull * (C / 8) >= (1ull << 32)) return fail(RIFE_HIP_EINVAL, "op_s16_geom: S16 tensors stay below 4 GB");
    if (pitch) *pitch = G.pitch;
    if (rows) *rows = G.rows;
    if (plane_bytes) *plane_bytes = G.plane();
    if (bytes) *bytes = G.bytes(C);
    return 0;
}

int rife_hip_op_trunk(int gpuid, int kernel, int C, int H, int W, int n_layers, const float* weight, const float* bias, const float* slope, int flip, int cus,
                      int nb, const void* const* in_s16, void* const* out_s16) {
    return rife_hip_op_trunk_prec(gpuid, kernel, C, H, W, n_layers, weight, bias, slope, flip, cus, nb, in_s16, out_s16, RIFE_HIP_PRECISION_FULL);
}
int rife_hip_op_trunk_prec(int gpuid, int kernel, int C, int H, int W, int n_layers, const float* weight, const float* bias, const float* slope, int flip, int cus,
                           int nb, const void* const* in_s16, void* const* out_s16, int precision) {
    int rc;
    if (precision != RIFE_HIP_PRECISION_FULL && precision != RIFE_HIP_PRECISION_FAST) return fail(RIFE_HIP_EINVAL, "op_trunk: unknown precision");
    const bool fast = precision == RIFE_HIP_PRECISION_FAST;
    if (fast && kernel == RIFE_HIP_TRUNK_KS) return fail(RIFE_HIP_ENOSYS, "op_trunk: conv_ks has no fast-precision form");
    size_t bytes = 0;
    if ((rc = rife_hip_op_s16_geom(C, H, W, nullptr, nullptr, nullptr, &bytes))) return rc;
    if (!weight || !bias || !slope || !in_s16 || !out_s16) return fail(RIFE_HIP_EINVAL, "op_trunk: null argument");
    if (n_layers < 1 || n_layers > 2 || cus < 0) return fail(RIFE_HIP_EINVAL, "op_trunk: one or two layers, a CU budget >= 0");
    if (nb < 1 || nb > 4) return fail(RIFE_HIP_EINVAL, "op_trunk: one to four tensors");
    for (int k = 0; k < nb; k++)
        if (!in_s16[k] || !out_s16[k]) return fail(RIFE_HIP_EINVAL, "op_trunk: null tensor");
    const bool batched = kernel == RIFE_HIP_TRUNK_ROW || kernel == RIFE_HIP_TRUNK_KS;
    if (nb > 1 && !batched) return fail(RIFE_HIP_EINVAL, "op_trunk: only conv_row and conv_ks have a batched form");
    // what the launchers refuse, before anything is uploaded or launched
    switch (kernel) {
        case RIFE_HIP_TRUNK_T64: if (C != 64 && C != 96) return fail(RIFE_HIP_EINVAL, "conv_t64 serves 64 and 96 channels"); break;
        case RIFE_HIP_TRUNK_RS:
            if (C != 64) return fail(RIFE_HIP_EINVAL, "conv_rs serves 64 channels");
            if ((H + 1) / 2 < RS_MIN_PAIRS) return fail(RIFE_HIP_EINVAL, "conv_rs needs at least " + std::to_string(2 * RS_MIN_PAIRS - 1) + " rows");
            break;
        case RIFE_HIP_TRUNK_RS2:
            if (C != 64) return fail(RIFE_HIP_EINVAL, "conv_rs2 serves 64 channels");
            if (n_layers != 2) return fail(RIFE_HIP_EINVAL, "conv_rs2 is two layers in one launch");
            break;
        case RIFE_HIP_TRUNK_ROW: if (C != 96 && C != 128 && C != 192) return fail(RIFE_HIP_EINVAL, "conv_row serves 96, 128 and 192 channels"); break;
        case RIFE_HIP_TRUNK_KS: if (C != 96 && C != 128) return fail(RIFE_HIP_EINVAL, "conv_ks serves 96 and 128 channels"); break;
        default: return fail(RIFE_HIP_EINVAL, "op_trunk: unknown kernel");
    }
    for (size_t i = 0; i < (size_t)n_layers * C * C * 9; i++)
        if (!((float)(_Float16)weight[i] == weight[i])) return fail(RIFE_HIP_EINVAL, "op_trunk: the S16 kernels need weights that are exactly fp16");
    if ((rc = check_device(gpuid))) return rc;
    struct BudgetGuard { int keep; ~BudgetGuard() { tl_cu_budget = keep; } } budget_guard{tl_cu_budget};
    tl_cu_budget = cus;
    if (kernel == RIFE_HIP_TRUNK_RS2 && !rs2_applies(H, W)) return fail(RIFE_HIP_EINVAL, "conv_rs2 does not apply to this tensor");

    ConvLayer L[2];
    unsigned char* d[2][4] = {};                                         // [in | out][tensor]
    auto cleanup = [&]() {
        for (auto& s : d) for (unsigned char* p : s) (void)hipFree(p);
        free_layer(L[0]); free_layer(L[1]);
    };
    for (int i = 0; i < n_layers; i++) {                                 // a trunk layer as rife_hip_load sets it up (engine_abi.h: setup(..., fold_skip = true))
        L[i].cin = L[i].cout = C; L[i].stride = 1; L[i].deconv = false; L[i].epi = EPI_STORE; L[i].cls = "trunk";
        L[i].tag = C == 64 ? 3 : 0;
        L[i].skip = true; L[i].want_t64 = true; L[i].want_s16out = false;
        if ((rc = upload_layer(L[i], weight + (size_t)i * C * C * 9, bias + (size_t)i * C, nullptr, slope[i]))) { cleanup(); return rc; }
        if (!L[i].d_t64 || (C == 96 && !L[i].d_row)) { cleanup(); return fail(RIFE_HIP_EINVAL, "op_trunk: the layer upload made no S16 weight image"); }
    }
    hipError_t e = hipSuccess;
    for (int k = 0; k < nb && e == hipSuccess; k++) {
        e = hipMalloc(&d[0][k], bytes);
        if (e == hipSuccess) e = hipMalloc(&d[1][k], bytes);
        if (e == hipSuccess) e = hipMemcpy(d[0][k], in_s16[k], bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d[1][k], out_s16[k], bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, std::string("op_trunk: ") + hipGetErrorString(e)); }
    int cur = 0;                                                         // which of the two buffers holds the layer's input
    const int nlaunch = kernel == RIFE_HIP_TRUNK_RS2 ? 1 : n_layers;
    for (int i = 0; i < nlaunch && !rc; i++, cur ^= 1) {
        const bool dir = ((flip != 0) ^ (i & 1)) != 0;
        const unsigned char* const* pin = d[cur];
        unsigned char* const* pout = d[cur ^ 1];
        switch (kernel) {
            case RIFE_HIP_TRUNK_T64: rc = launch_t64(L[i], pin[0], pout[0], H, W, 0, dir, fast); break;
            case RIFE_HIP_TRUNK_RS: rc = launch_rs(L[i], pin[0], pout[0], H, W, 0, dir, fast); break;
            case RIFE_HIP_TRUNK_RS2: rc = launch_rs2(L[0], L[1], pin[0], pout[0], H, W, 0, dir, fast); break;
            case RIFE_HIP_TRUNK_ROW: rc = nb > 1 ? launch_row(L[i], nullptr, nullptr, H, W, 0, nb, pin, pout, fast) : launch_row(L[i], pin[0], pout[0], H, W, 0, 0, nullptr, nullptr, fast); break;
            default: rc = nb > 1 ? launch_ks(L[i], nullptr, nullptr, H, W, 0, nb, pin, pout) : launch_ks(L[i], pin[0], pout[0], H, W, 0); break;
        }
    }
    e = hipDeviceSynchronize();
    if (!rc && e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_trunk: ") + hipGetErrorString(e));
    for (int k = 0; k < nb && !rc; k++) {
        e = hipMemcpy(out_s16[k], d[cur][k], bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_trunk: ") + hipGetErrorString(e));
    }
    cleanup();
    return rc;
}

// ---- the two ends of the S16 trunk alone (tests/test_gpu_s16_ends.py): the stride-2 stem that writes the first S16 tensor of a block and the PixelShuffle head
// that reads the last one, each through the product's layer upload (the flags rife_hip_load sets) and launch_conv ----
static bool s16_ends_channels(int C) { return C == 64 || C == 96 || C == 128 || C == 192; }
static bool all_fp16(const float* w, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!((float)(_Float16)w[i] == w[i])) return false;
    return true;
}

int rife_hip_op_stem1_s16(int gpuid, int C, int Ht, int Wt, const float* x_chw, const float* weight, const float* bias, float slope, void* out_s16) {
    int rc;
    if (!s16_ends_channels(C)) return fail(RIFE_HIP_EINVAL, "op_stem1_s16: the S16 variant of the stride-2 stem serves 64, 96, 128 and 192 output channels");
    size_t bytes = 0;
    if ((rc = rife_hip_op_s16_geom(C, Ht, Wt, nullptr, nullptr, nullptr, &bytes))) return rc;
    if (!x_chw || !weight || !bias || !out_s16) return fail(RIFE_HIP_EINVAL, "op_stem1_s16: null argument");
    const int cin = C / 2, H = 2 * Ht, W = 2 * Wt;
    if (!all_fp16(weight, (size_t)C * cin * 9)) return fail(RIFE_HIP_EINVAL, "op_stem1_s16: the S16 kernels need weights that are exactly fp16");
    if ((rc = check_device(gpuid))) return rc;
    ConvLayer L;
    float *d_chw = nullptr, *d_x = nullptr; unsigned char* d_o = nullptr;
    auto cleanup = [&]() { (void)hipFree(d_chw); (void)hipFree(d_x); (void)hipFree(d_o); free_layer(L); };
    L.cin = cin; L.cout = C; L.stride = 2; L.deconv = false; L.epi = EPI_STORE; L.cls = "stem1"; L.tag = 0; L.skip = false;      // setup() of rife_hip_load for stem1_b*
    L.want_t64 = false; L.want_s16out = true;
    if ((rc = upload_layer(L, weight, bias, nullptr, slope))) { cleanup(); return rc; }
    if (!L.d_whp) { cleanup(); return fail(RIFE_HIP_EINVAL, "op_stem1_s16: the layer upload made no row-permuted weight image"); }
    const S16Geom G(Ht, Wt);
    const size_t nin = (size_t)cin * H * W;
    hipError_t e = hipMalloc(&d_chw, nin * 4);
    if (e == hipSuccess) e = hipMalloc(&d_x, nin * 4);
    if (e == hipSuccess) e = hipMalloc(&d_o, bytes);
    if (e == hipSuccess) e = hipMemcpy(d_chw, x_chw, nin * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_o, out_s16, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, std::string("op_stem1_s16: ") + hipGetErrorString(e)); }
    hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(W, H), dim3(256), 0, 0, d_chw, d_x, cin, H, W, cin);
    rc = launch_conv(L, {d_x, cin, 0}, H, W, {reinterpret_cast<float*>(d_o), C, 0}, nullptr, 0, nullptr, G.pitch, G.plane());      // run_block_convs: stem-1 on the S16 path
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(out_s16, d_o, bytes, hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_stem1_s16: ") + hipGetErrorString(e));
    cleanup();
    return rc;
}

int rife_hip_op_head_ps(int gpuid, int C, int Ht, int Wt, int s16, const void* input, const float* weight, const float* bias, float* out8hw) {
    int rc;
    if (!s16_ends_channels(C)) return fail(RIFE_HIP_EINVAL, "op_head_ps: the heads of rife-v4.6 read 64, 96, 128 or 192 channels");
    size_t bytes = 0;
    if ((rc = rife_hip_op_s16_geom(C, Ht, Wt, nullptr, nullptr, nullptr, &bytes))) return rc;
    if (!input || !weight || !bias || !out8hw) return fail(RIFE_HIP_EINVAL, "op_head_ps: null argument");
    if (!all_fp16(weight, (size_t)24 * C * 16)) return fail(RIFE_HIP_EINVAL, "op_head_ps: the split-f16 head needs weights that are exactly fp16");
    if ((rc = check_device(gpuid))) return rc;
    ConvLayer L;
    float *d_chw = nullptr, *d_flow = nullptr; unsigned char* d_in = nullptr;
    auto cleanup = [&]() { (void)hipFree(d_chw); (void)hipFree(d_flow); (void)hipFree(d_in); free_layer(L); };
    L.cin = C; L.cout = 24; L.stride = 1; L.deconv = true; L.epi = EPI_DECONV_PS; L.cls = "head"; L.tag = 0; L.skip = false;      // setup() of rife_hip_load for head_b*
    L.want_t64 = false; L.want_s16out = false;
    if ((rc = upload_layer(L, weight, bias, nullptr, 1.0f))) { cleanup(); return rc; }
    if (!L.d_wh) { cleanup(); return fail(RIFE_HIP_EINVAL, "op_head_ps: the layer upload made no split-f16 weight image"); }
    const S16Geom G(Ht, Wt);
    const int Hf = 4 * Ht, Wf = 4 * Wt;
    const size_t nflow = (size_t)8 * Hf * Wf, nin = (size_t)C * Ht * Wt, nx = s16 ? bytes : nin * 4;
    hipError_t e = hipMalloc(&d_chw, std::max(nflow, nin) * 4);
    if (e == hipSuccess) e = hipMalloc(&d_flow, nflow * 4);
    if (e == hipSuccess) e = hipMalloc(&d_in, nx);
    if (e == hipSuccess) e = hipMemcpy(d_chw, out8hw, nflow * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, std::string("op_head_ps: ") + hipGetErrorString(e)); }
    hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(Wf, Hf), dim3(256), 0, 0, d_chw, d_flow, 8, Hf, Wf, 8);
    if (s16) {
        e = hipMemcpy(d_in, input, bytes, hipMemcpyHostToDevice);
    } else {
        e = hipMemcpy(d_chw, input, nin * 4, hipMemcpyHostToDevice);      // the null stream: after the kernel above has read d_chw
        if (e == hipSuccess) hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(Wt, Ht), dim3(256), 0, 0, d_chw, reinterpret_cast<float*>(d_in), C, Ht, Wt, C);
    }
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, std::string("op_head_ps: ") + hipGetErrorString(e)); }
    rc = launch_conv(L, {reinterpret_cast<float*>(d_in), C, 0}, Ht, Wt, {d_flow, 8, 0}, nullptr, 0, nullptr, s16 ? G.pitch : 0, s16 ? G.plane() : 0u);
    if (!rc) {
        hipLaunchKernelGGL(k_nhwc_to_chw, grid2d(Wf, Hf), dim3(256), 0, 0, d_flow, d_chw, 8, Hf, Wf, 8);
        e = hipMemcpy(out8hw, d_chw, nflow * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_head_ps: ") + hipGetErrorString(e));
    } else (void)hipDeviceSynchronize();
    cleanup();
    return rc;
}

// ---- the fused tails alone (tests/test_gpu_tail_parity.py): the kernels that read the last S16 trunk tensor of block 3 and write the quantised frame, one launch
// each through the product's layer upload (the flags rife_hip_load sets for head_b3) and the product's launchers; the unfused pair is the two launches of run_v4 ----
int rife_hip_op_tail(int gpuid, int kernel, int pixfmt, int w, int h, const void* trunk, const float* weight, const float* bias, const float* F, const float* M,
                     const uint32_t* img0, const uint32_t* img1, int cus, void* out) {
    int rc;
    constexpr int C = 64;
    if (!trunk || !weight || !bias || !F || !M || !img0 || !img1 || !out) return fail(RIFE_HIP_EINVAL, "op_tail: null argument");
    if (kernel < RIFE_HIP_TAIL_RS || kernel > RIFE_HIP_TAIL_UNFUSED) return fail(RIFE_HIP_EINVAL, "op_tail: unknown kernel");
    if (pixfmt != RIFE_HIP_PIX_RGB8 && pixfmt != RIFE_HIP_PIX_RGB10_U16 && pixfmt != RIFE_HIP_PIX_A2B10G10R10 && pixfmt != RIFE_HIP_PIX_RGBA8)
        return fail(RIFE_HIP_EINVAL, "op_tail: one of the four packed RGB formats");
    if (w <= 0 || h <= 0 || cus < 0) return fail(RIFE_HIP_EINVAL, "op_tail: a frame size and a CU budget >= 0");
    const long long wpl = align_up((long long)w, 32), hpl = align_up((long long)h, 32);
    if (wpl * hpl >= (1ll << 27)) return fail(RIFE_HIP_EINVAL, "op_tail: frames stay below 2^27 pixels (the kernels address F and the frame with 32-bit byte offsets)");
    const int wp = (int)wpl, hp = (int)hpl, Hq = hp / 4, Wq = wp / 4;
    size_t bytes = 0;
    if ((rc = rife_hip_op_s16_geom(C, Hq, Wq, nullptr, nullptr, nullptr, &bytes))) return rc;
    if (!all_fp16(weight, (size_t)24 * C * 16)) return fail(RIFE_HIP_EINVAL, "op_tail: the split-f16 head needs weights that are exactly fp16");
    // run_block_convs gives block 3's head to tail_rs_kernel only on the S16 path of the split-f16 trunk and with the kernel switched on
    const Switches sw = read_switches();                                 // engine scope in the product (rife_hip_create): per call here, which has no engine
    if (kernel == RIFE_HIP_TAIL_RS && !(sw.tail_rs && sw.t64 && trunk_h2()))
        return fail(RIFE_HIP_EINVAL, "op_tail: the product would not run tail_rs_kernel on this head (RIFE_HIP_TAIL_RS=0, RIFE_HIP_T64=0 or RIFE_HIP_TRUNK=f32)");
    if ((rc = check_device(gpuid))) return rc;
    struct BudgetGuard { int keep; ~BudgetGuard() { tl_cu_budget = keep; } } budget_guard{tl_cu_budget};
    tl_cu_budget = cus;

    rife_hip::Block B;
    ConvLayer& L = B.head;
    float *d_chw = nullptr, *d_flow = nullptr, *d_F = nullptr, *d_M = nullptr; uint32_t *d_i0 = nullptr, *d_i1 = nullptr; unsigned char *d_in = nullptr, *d_out = nullptr;
    auto cleanup = [&]() {
        (void)hipFree(d_chw); (void)hipFree(d_flow); (void)hipFree(d_F); (void)hipFree(d_M); (void)hipFree(d_i0); (void)hipFree(d_i1); (void)hipFree(d_in); (void)hipFree(d_out);
        free_layer(L);
    };
    B.c = C; B.scale = 1;
    L.cin = C; L.cout = 24; L.stride = 1; L.deconv = true; L.epi = EPI_DECONV_PS; L.cls = "head"; L.tag = 0; L.skip = false;      // setup() of rife_hip_load for head_b3
    L.want_t64 = false; L.want_s16out = false;
    if ((rc = upload_layer(L, weight, bias, nullptr, 1.0f))) { cleanup(); return rc; }
    if (!L.d_wh) { cleanup(); return fail(RIFE_HIP_EINVAL, "op_tail: the layer upload made no split-f16 weight image"); }
    const S16Geom G(Hq, Wq);
    const bool s16 = kernel != RIFE_HIP_TAIL_HEAD_F32;
    const size_t npix = (size_t)wp * hp, nin = (size_t)C * Hq * Wq, nx = s16 ? bytes : nin * 4;
    const size_t nframe = frame_bytes(w, h, pixfmt), nout = nframe + 2 * (size_t)RIFE_HIP_TAIL_GUARD;
    hipError_t e = hipMalloc(&d_in, nx);
    if (e == hipSuccess) e = hipMalloc(&d_F, npix * 16);
    if (e == hipSuccess) e = hipMalloc(&d_M, npix * 4);
    if (e == hipSuccess) e = hipMalloc(&d_i0, npix * 4);
    if (e == hipSuccess) e = hipMalloc(&d_i1, npix * 4);
    if (e == hipSuccess) e = hipMalloc(&d_out, nout);
    if (e == hipSuccess && !s16) e = hipMalloc(&d_chw, nin * 4);
    if (e == hipSuccess) e = hipMalloc(&d_flow, npix * 8 * 4);      // the fused kernels get the flow tensor the product hands them and leave it alone
    if (e == hipSuccess) e = hipMemcpy(d_F, F, npix * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_M, M, npix * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_i0, img0, npix * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_i1, img1, npix * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_out, out, nout, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_flow, 0xff, npix * 8 * 4);      // NaN: k_final reads what the head wrote, nothing else
    if (e == hipSuccess) e = hipMemcpy(s16 ? reinterpret_cast<void*>(d_in) : reinterpret_cast<void*>(d_chw), trunk, nx, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, std::string("op_tail: ") + hipGetErrorString(e)); }
    if (!s16) hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(Wq, Hq), dim3(256), 0, 0, d_chw, reinterpret_cast<float*>(d_in), C, Hq, Wq, C);
    uint8_t* const frame = d_out + RIFE_HIP_TAIL_GUARD;
    const FinalArgs fin{d_i0, d_i1, reinterpret_cast<const float4*>(d_F), d_M, frame, w, h, wp, hp, pixfmt};
    const TensorView x{reinterpret_cast<float*>(d_in), C, 0};
    switch (kernel) {
        case RIFE_HIP_TAIL_RS: rc = launch_tail_rs(B, d_in, Hq, Wq, fin, 0); break;
        case RIFE_HIP_TAIL_HEAD_S16: rc = launch_conv(L, x, Hq, Wq, {d_flow, 8, 0}, nullptr, 0, &fin, G.pitch, G.plane()); break;
        case RIFE_HIP_TAIL_HEAD_F32: rc = launch_conv(L, x, Hq, Wq, {d_flow, 8, 0}, nullptr, 0, &fin); break;
        default:
            rc = launch_conv(L, x, Hq, Wq, {d_flow, 8, 0}, nullptr, 0, nullptr, G.pitch, G.plane());
            if (rc) break;
            if (pixfmt == RIFE_HIP_PIX_RGB10_U16) hipLaunchKernelGGL(k_final_px<1>, grid2d(w, h), dim3(256), 0, 0, d_i0, d_i1, fin.F, d_M, d_flow, frame, w, h, wp, hp);
            else if (pixfmt == RIFE_HIP_PIX_A2B10G10R10) hipLaunchKernelGGL(k_final_px<2>, grid2d(w, h), dim3(256), 0, 0, d_i0, d_i1, fin.F, d_M, d_flow, frame, w, h, wp, hp);
            else if (pixfmt == RIFE_HIP_PIX_RGBA8) hipLaunchKernelGGL(k_final_px<4>, grid2d(w, h), dim3(256), 0, 0, d_i0, d_i1, fin.F, d_M, d_flow, frame, w, h, wp, hp);
            else hipLaunchKernelGGL(k_final, grid2d(w, h), dim3(256), 0, 0, d_i0, d_i1, fin.F, d_M, d_flow, frame, w, h, wp, hp);
            break;
    }
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_tail: ") + hipGetErrorString(e));
    cleanup();
    return rc;
}

// op_tail_motion: the same set-up, ONE launch of the motion form of the kernel under test.  A function of its own, so that rife_hip_op_tail stays as it is: flow / mask are
// HOST buffers of RIFE_HIP_TAIL_GUARD bytes, h rows of the given pitch and RIFE_HIP_TAIL_GUARD bytes, uploaded as given and downloaded whole
int rife_hip_op_tail_motion(int gpuid, int kernel, int pixfmt, int w, int h, const void* trunk, const float* weight, const float* bias, const float* F, const float* M,
                            const uint32_t* img0, const uint32_t* img1, int cus, void* out, int motion_format, void* flow, size_t flow_pitch, void* mask, size_t mask_pitch) {
    int rc;
    {   // the rules of the product's motion calls (a frame size among them) on the buffers the kernel will see: RIFE_HIP_TAIL_GUARD bytes into an allocation, i.e. as aligned as the guard size
        rife_hip_motion_t probe{flow ? reinterpret_cast<void*>((uintptr_t)RIFE_HIP_TAIL_GUARD) : nullptr, flow_pitch, mask ? reinterpret_cast<void*>((uintptr_t)RIFE_HIP_TAIL_GUARD) : nullptr,
                                mask_pitch, motion_format};
        std::string err;
        if (rife_motion::check(&probe, w, h, err)) return fail(RIFE_HIP_EINVAL, "op_tail_motion: " + err);
    }
    constexpr int C = 64;
    if (!trunk || !weight || !bias || !F || !M || !img0 || !img1 || !out) return fail(RIFE_HIP_EINVAL, "op_tail: null argument");
    if (kernel < RIFE_HIP_TAIL_RS || kernel > RIFE_HIP_TAIL_UNFUSED) return fail(RIFE_HIP_EINVAL, "op_tail: unknown kernel");
    if (pixfmt != RIFE_HIP_PIX_RGB8 && pixfmt != RIFE_HIP_PIX_RGB10_U16 && pixfmt != RIFE_HIP_PIX_A2B10G10R10 && pixfmt != RIFE_HIP_PIX_RGBA8)
        return fail(RIFE_HIP_EINVAL, "op_tail: one of the four packed RGB formats");
    if (w <= 0 || h <= 0 || cus < 0) return fail(RIFE_HIP_EINVAL, "op_tail: a frame size and a CU budget >= 0");
    const long long wpl = align_up((long long)w, 32), hpl = align_up((long long)h, 32);
    if (wpl * hpl >= (1ll << 27)) return fail(RIFE_HIP_EINVAL, "op_tail: frames stay below 2^27 pixels (the kernels address F and the frame with 32-bit byte offsets)");
    const int wp = (int)wpl, hp = (int)hpl, Hq = hp / 4, Wq = wp / 4;
    size_t bytes = 0;
    if ((rc = rife_hip_op_s16_geom(C, Hq, Wq, nullptr, nullptr, nullptr, &bytes))) return rc;
    if (!all_fp16(weight, (size_t)24 * C * 16)) return fail(RIFE_HIP_EINVAL, "op_tail: the split-f16 head needs weights that are exactly fp16");
    // run_block_convs gives block 3's head to tail_rs_kernel only on the S16 path of the split-f16 trunk and with the kernel switched on
    const Switches sw = read_switches();                                 // engine scope in the product (rife_hip_create): per call here, which has no engine
    if (kernel == RIFE_HIP_TAIL_RS && !(sw.tail_rs && sw.t64 && trunk_h2()))
        return fail(RIFE_HIP_EINVAL, "op_tail: the product would not run tail_rs_kernel on this head (RIFE_HIP_TAIL_RS=0, RIFE_HIP_T64=0 or RIFE_HIP_TRUNK=f32)");
    if ((rc = check_device(gpuid))) return rc;
    struct BudgetGuard { int keep; ~BudgetGuard() { tl_cu_budget = keep; } } budget_guard{tl_cu_budget};
    tl_cu_budget = cus;

    rife_hip::Block B;
    ConvLayer& L = B.head;
    float *d_chw = nullptr, *d_flow = nullptr, *d_F = nullptr, *d_M = nullptr; uint32_t *d_i0 = nullptr, *d_i1 = nullptr; unsigned char *d_in = nullptr, *d_out = nullptr;
    uint8_t *d_mflow = nullptr, *d_mmask = nullptr;
    const size_t nmflow = flow ? (size_t)h * flow_pitch + 2 * (size_t)RIFE_HIP_TAIL_GUARD : 0, nmmask = mask ? (size_t)h * mask_pitch + 2 * (size_t)RIFE_HIP_TAIL_GUARD : 0;
    auto cleanup = [&]() {
        (void)hipFree(d_mflow); (void)hipFree(d_mmask);
        (void)hipFree(d_chw); (void)hipFree(d_flow); (void)hipFree(d_F); (void)hipFree(d_M); (void)hipFree(d_i0); (void)hipFree(d_i1); (void)hipFree(d_in); (void)hipFree(d_out);
        free_layer(L);
    };
    B.c = C; B.scale = 1;
    L.cin = C; L.cout = 24; L.stride = 1; L.deconv = true; L.epi = EPI_DECONV_PS; L.cls = "head"; L.tag = 0; L.skip = false;      // setup() of rife_hip_load for head_b3
    L.want_t64 = false; L.want_s16out = false;
    if ((rc = upload_layer(L, weight, bias, nullptr, 1.0f))) { cleanup(); return rc; }
    if (!L.d_wh) { cleanup(); return fail(RIFE_HIP_EINVAL, "op_tail: the layer upload made no split-f16 weight image"); }
    const S16Geom G(Hq, Wq);
    const bool s16 = kernel != RIFE_HIP_TAIL_HEAD_F32;
    const size_t npix = (size_t)wp * hp, nin = (size_t)C * Hq * Wq, nx = s16 ? bytes : nin * 4;
    const size_t nframe = frame_bytes(w, h, pixfmt), nout = nframe + 2 * (size_t)RIFE_HIP_TAIL_GUARD;
    hipError_t e = hipMalloc(&d_in, nx);
    if (e == hipSuccess) e = hipMalloc(&d_F, npix * 16);
    if (e == hipSuccess) e = hipMalloc(&d_M, npix * 4);
    if (e == hipSuccess) e = hipMalloc(&d_i0, npix * 4);
    if (e == hipSuccess) e = hipMalloc(&d_i1, npix * 4);
    if (e == hipSuccess) e = hipMalloc(&d_out, nout);
    if (e == hipSuccess && !s16) e = hipMalloc(&d_chw, nin * 4);
    if (e == hipSuccess) e = hipMalloc(&d_flow, npix * 8 * 4);      // the fused kernels get the flow tensor the product hands them and leave it alone
    if (e == hipSuccess) e = hipMemcpy(d_F, F, npix * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_M, M, npix * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_i0, img0, npix * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_i1, img1, npix * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_out, out, nout, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_flow, 0xff, npix * 8 * 4);      // NaN: k_final reads what the head wrote, nothing else
    if (e == hipSuccess) e = hipMemcpy(s16 ? reinterpret_cast<void*>(d_in) : reinterpret_cast<void*>(d_chw), trunk, nx, hipMemcpyHostToDevice);
    if (e == hipSuccess && nmflow) e = hipMalloc(&d_mflow, nmflow);
    if (e == hipSuccess && nmflow) e = hipMemcpy(d_mflow, flow, nmflow, hipMemcpyHostToDevice);
    if (e == hipSuccess && nmmask) e = hipMalloc(&d_mmask, nmmask);
    if (e == hipSuccess && nmmask) e = hipMemcpy(d_mmask, mask, nmmask, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return fail(RIFE_HIP_EHIP, std::string("op_tail_motion (upload): ") + hipGetErrorString(e)); }
    if (!s16) hipLaunchKernelGGL(k_chw_to_nhwc, grid2d(Wq, Hq), dim3(256), 0, 0, d_chw, reinterpret_cast<float*>(d_in), C, Hq, Wq, C);
    uint8_t* const frame = d_out + RIFE_HIP_TAIL_GUARD;
    const FinalArgs fin{d_i0, d_i1, reinterpret_cast<const float4*>(d_F), d_M, frame, w, h, wp, hp, pixfmt};
    const TensorView x{reinterpret_cast<float*>(d_in), C, 0};
    MotionArgs mo;
    mo.flow = d_mflow ? d_mflow + RIFE_HIP_TAIL_GUARD : nullptr; mo.flow_pitch = (unsigned)flow_pitch;
    mo.mask = d_mmask ? d_mmask + RIFE_HIP_TAIL_GUARD : nullptr; mo.mask_pitch = (unsigned)mask_pitch; mo.format = motion_format;
    switch (kernel) {
        case RIFE_HIP_TAIL_RS: rc = launch_tail_rs_motion(B, d_in, Hq, Wq, fin, mo, 0); break;
        case RIFE_HIP_TAIL_HEAD_S16: rc = launch_conv(L, x, Hq, Wq, {d_flow, 8, 0}, nullptr, 0, &fin, G.pitch, G.plane(), nullptr, nullptr, nullptr, &mo); break;
        case RIFE_HIP_TAIL_HEAD_F32: rc = launch_conv(L, x, Hq, Wq, {d_flow, 8, 0}, nullptr, 0, &fin, 0, 0, nullptr, nullptr, nullptr, &mo); break;
        default:
            rc = launch_conv(L, x, Hq, Wq, {d_flow, 8, 0}, nullptr, 0, nullptr, G.pitch, G.plane());
            if (rc) break;
            launch_final_motion(0, d_i0, d_i1, fin.F, d_M, d_flow, frame, w, h, wp, hp, pixfmt, mo);
            break;
    }
    e = hipDeviceSynchronize();
    if (!rc && e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_tail_motion (after the launch): ") + hipGetErrorString(e));
    if (!rc) e = hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost);
    if (!rc && e == hipSuccess && nmflow) e = hipMemcpy(flow, d_mflow, nmflow, hipMemcpyDeviceToHost);
    if (!rc && e == hipSuccess && nmmask) e = hipMemcpy(mask, d_mmask, nmmask, hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(RIFE_HIP_EHIP, std::string("op_tail_motion (download): ") + hipGetErrorString(e));
    cleanup();
    return rc;
}

#endif  // RIFE_HIP_TEST_BUILD

#ifdef RIFE_HIP_BENCH_BUILD
#include "bench_hooks.h"      // bench-only / probe entry points and ablation instantiations: librife_hip_bench.so (tools/*.py), never the product
#endif

// tooling: structural hash of a named blob of a .param file (used to derive / test the compiled-in constants)
static int rife_hip_param_hash_impl(const char* param_path, const char* blob, uint64_t* out) {
    NcnnModel m;
    if (!m.load_param(param_path)) return fail(RIFE_HIP_EIO, m.error);
    *out = m.structural_hash(blob);
    return *out ? 0 : fail(RIFE_HIP_EMODEL, "no such blob");
}
int rife_hip_param_hash(const char* param_path, const char* blob, uint64_t* out) {
    return guarded("rife_hip_param_hash", [&] { return rife_hip_param_hash_impl(param_path, blob, out); });
}

}  // extern "C"
