// engine_v2_ops.h: single-launch entry points of the rife-v2.x / v3.x schedule's own kernels (include/rife_hip_test.h "rife-v2 / v3 kernels alone";
// tests/test_gpu_v2_ops.py) - elementwise_v2.h, stem_fused_v2.h, conv_img.h and the two-tensor / second-destination forms of launch_conv.  TEST BUILD ONLY: the
// schedule (engine_v2.h) and the product library do not change; every kernel launched here is an instantiation the product has.
// One translation unit (engine.hip includes the engine_*.h sections in dependency order; every function here is file-local).
// No include guard on purpose: a section is included exactly once, by engine.hip.
// Host arrays in and out; every OUTPUT buffer goes to the device as the caller filled it and comes back whole, so a store outside a kernel's domain shows up.

#ifdef RIFE_HIP_TEST_BUILD

namespace {
struct V2Buf {                                  // one device allocation, freed with the scope
    void* p = nullptr;
    size_t n = 0;
    ~V2Buf() { if (p) (void)hipFree(p); }
    hipError_t up(const void* host, size_t bytes) {
        n = bytes;
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        return e != hipSuccess || !host ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    }
    hipError_t down(void* host) const { return hipMemcpy(host, p, n, hipMemcpyDeviceToHost); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};
struct V2Layer { ConvLayer L; ~V2Layer() { free_layer(L); } };

// launch error, then the drain, then the downloads `back()` does
template <typename F>
int v2_finish(const char* op, int rc, F&& back) {
    hipError_t e = hipGetLastError();
    const hipError_t s = hipDeviceSynchronize();
    if (rc) return rc;
    if (e == hipSuccess) e = s;
    if (e == hipSuccess) e = back();
    return e == hipSuccess ? 0 : fail(RIFE_HIP_EHIP, std::string(op) + ": " + hipGetErrorString(e));
}
int v2_frame_dims(const char* op, int imgf4, int wp, int hp) {
    const int m = imgf4 ? 16 : 32;              // ImgF4 frames are the halves of frames padded to 32n (run_v2_flow, UHD mode)
    if (wp <= 0 || hp <= 0 || wp % m || hp % m || (long long)wp * hp >= (1ll << 27))
        return fail(RIFE_HIP_EINVAL, std::string(op) + ": padded frames are multiples of 32 (float4 half frames: 16) below 2^27 pixels");
    return 0;
}
bool v2_assemble_served(int S, bool first, bool fscale) {      // the launches of run_v2_ifnet / run_v2_synth
    if (first) return !fscale && (S == 8 || S == 4);
    return fscale ? S == 2 : (S == 4 || S == 2 || S == 1);
}
template <typename IMG>
void v2_launch_assemble(int S, bool first, bool fscale, IMG i0, IMG i1, const float4* acc, float* X, int wp, int hp) {
    const dim3 g = grid2d(wp / S, hp / S), b(256);
    if (first && S == 8) hipLaunchKernelGGL((k2_assemble0<8, IMG>), g, b, 0, 0, i0, i1, X, wp, hp);
    else if (first) hipLaunchKernelGGL((k2_assemble0<4, IMG>), g, b, 0, 0, i0, i1, X, wp, hp);
    else if (fscale) hipLaunchKernelGGL((k2_assemble<2, IMG, true>), g, b, 0, 0, i0, i1, acc, X, wp, hp);
    else if (S == 4) hipLaunchKernelGGL((k2_assemble<4, IMG>), g, b, 0, 0, i0, i1, acc, X, wp, hp);
    else if (S == 2) hipLaunchKernelGGL((k2_assemble<2, IMG>), g, b, 0, 0, i0, i1, acc, X, wp, hp);
    else hipLaunchKernelGGL((k2_assemble<1, IMG>), g, b, 0, 0, i0, i1, acc, X, wp, hp);
}
}  // namespace

extern "C" {

// k2_assemble0<8 | 4, IMG> (first) / k2_assemble<4 | 2 | 1, IMG, FSCALE>: the block input with its pad channels
int rife_hip_op_v2_assemble(int gpuid, int S, int first, int fscale, int imgf4, const void* img0, const void* img1, int wp, int hp, const float* acc, float* out) {
    int rc;
    if (!img0 || !img1 || !out || (!first && !acc)) return fail(RIFE_HIP_EINVAL, "op_v2_assemble: null argument");
    if (!v2_assemble_served(S, first != 0, fscale != 0)) return fail(RIFE_HIP_EINVAL, "op_v2_assemble: the schedule launches k2_assemble0<8 | 4> and k2_assemble<4 | 2 | 1> (x 1/S: S = 2 only)");
    if ((rc = v2_frame_dims("op_v2_assemble", imgf4, wp, hp))) return rc;
    if ((rc = check_device(gpuid))) return rc;
    const size_t P = (size_t)wp * hp, nout = P / S / S * (first ? 8 : 16) * 4;
    V2Buf d0, d1, da, dx;
    hipError_t e = d0.up(img0, P * (imgf4 ? 16 : 4));
    if (e == hipSuccess) e = d1.up(img1, P * (imgf4 ? 16 : 4));
    if (e == hipSuccess) e = da.up(first ? nullptr : acc, P / 4 * 16);
    if (e == hipSuccess) e = dx.up(out, nout);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_assemble: ") + hipGetErrorString(e));
    if (imgf4) v2_launch_assemble(S, first != 0, fscale != 0, ImgF4{d0.as<const float4>()}, ImgF4{d1.as<const float4>()}, da.as<const float4>(), dx.as<float>(), wp, hp);
    else v2_launch_assemble(S, first != 0, fscale != 0, ImgU8{d0.as<const uint32_t>()}, ImgU8{d1.as<const uint32_t>()}, da.as<const float4>(), dx.as<float>(), wp, hp);
    return v2_finish("op_v2_assemble", 0, [&] { return dx.down(out); });
}

// the 10 -> cout stride-2 stem of IFNet blocks 1.. and of the FusionNet: route RIFE_HIP_V2_STEM_PRODUCT = launch_stem2_fused as run_v2_ifnet / run_v2_synth call it,
// _NO_R64 = the same with the R64 choice off (RIFE_HIP_V2_STEM_R64=0 is process scope: the one launch it changes is restated here), _UNFUSED = k2_assemble + launch_conv
int rife_hip_op_v2_stem(int gpuid, int route, int S, int fscale, int imgf4, const void* img0, const void* img1, int wp, int hp, const float* acc, const float* weight,
                        const float* bias, const float* slope, int cout, int out_ld, float* out) {
    int rc;
    if (!img0 || !img1 || !acc || !weight || !bias || !slope || !out) return fail(RIFE_HIP_EINVAL, "op_v2_stem: null argument");
    if (route < RIFE_HIP_V2_STEM_PRODUCT || route > RIFE_HIP_V2_STEM_UNFUSED) return fail(RIFE_HIP_EINVAL, "op_v2_stem: unknown route");
    if (!(S == 1 || S == 2) || (fscale && S != 2)) return fail(RIFE_HIP_EINVAL, "op_v2_stem: scale 1 or 2, the x 1/S of rife-v3.x at scale 2 only");
    if (cout <= 0 || cout > 96 || cout % 4 || out_ld < cout || out_ld % 4) return fail(RIFE_HIP_EINVAL, "op_v2_stem: 4n <= 96 output channels in a view of 4n floats per pixel");
    if ((rc = v2_frame_dims("op_v2_stem", imgf4, wp, hp))) return rc;
    if (!all_fp16(weight, (size_t)cout * 90)) return fail(RIFE_HIP_EINVAL, "op_v2_stem: the split-f16 stems need weights that are exactly fp16");
    const bool h2s2 = trunk_h2() && process_switches().v2_stem16;      // upload_layer then packs the split-f16 image of a 10-channel stride-2 layer (checked again below)
    if (!h2s2 || (route != RIFE_HIP_V2_STEM_UNFUSED && !v2_fused_stem()))
        return fail(RIFE_HIP_EINVAL, "op_v2_stem: the product would not run this route (RIFE_HIP_TRUNK=f32, RIFE_HIP_V2_STEM16=0 or RIFE_HIP_V2_FUSED_STEM=0)");
    if ((rc = check_device(gpuid))) return rc;
    rife_hip E;
    E.gpuid = gpuid;
    ConvLayer& L = E.fblk[1].stem0;              // freed with E
    L.cin = 10; L.cout = cout; L.stride = 2; L.deconv = false; L.epi = EPI_STORE; L.cls = "v2_flow_stem"; L.tag = 0;      // take() of load_v2
    if ((rc = upload_layer(L, weight, bias, slope, 1.0f))) return rc;
    if (route != RIFE_HIP_V2_STEM_UNFUSED && !stem2_fusable(L, S, wp, hp)) return fail(RIFE_HIP_EINVAL, "op_v2_stem: the product would not run stem2_fused_kernel on this layer");
    if (route == RIFE_HIP_V2_STEM_UNFUSED && !conv_is_h2s2(L, nullptr)) return fail(RIFE_HIP_EINVAL, "op_v2_stem: the product would not run conv_h2s2_kernel on this layer");
    const size_t P = (size_t)wp * hp;
    const int Hb = hp / S, Wb = wp / S, Ho = Hb / 2, Wo = Wb / 2;
    V2Buf d0, d1, da, dx, dy;
    hipError_t e = d0.up(img0, P * (imgf4 ? 16 : 4));
    if (e == hipSuccess) e = d1.up(img1, P * (imgf4 ? 16 : 4));
    if (e == hipSuccess) e = da.up(acc, P / 4 * 16);
    if (e == hipSuccess) e = dy.up(out, (size_t)Ho * Wo * out_ld * 4);
    if (e == hipSuccess && route == RIFE_HIP_V2_STEM_UNFUSED) e = dx.up(nullptr, (size_t)Hb * Wb * 16 * 4);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_stem: ") + hipGetErrorString(e));
    const float4* const a4 = da.as<const float4>();
    const ImgU8 u0{d0.as<const uint32_t>()}, u1{d1.as<const uint32_t>()};
    const ImgF4 f0{d0.as<const float4>()}, f1{d1.as<const float4>()};
    if (route == RIFE_HIP_V2_STEM_UNFUSED) {
        if (imgf4) v2_launch_assemble(S, false, fscale != 0, f0, f1, a4, dx.as<float>(), wp, hp);
        else v2_launch_assemble(S, false, fscale != 0, u0, u1, a4, dx.as<float>(), wp, hp);
        rc = launch_conv(L, {dx.as<float>(), 16, 0}, Hb, Wb, {dy.as<float>(), out_ld, 0}, nullptr, 0);
    } else if (route == RIFE_HIP_V2_STEM_NO_R64 && S == 1 && !imgf4) {
        Stem2Args<ImgU8> a;                      // launch_stem2_fused's arguments, then its S == 1 launch without the R64 form
        a.img0 = u0; a.img1 = u1; a.acc = a4; a.wpk = reinterpret_cast<const unsigned char*>(L.d_wh); a.bias = L.d_bias; a.slope = L.d_slope; a.out = dy.as<float>();
        a.wp = wp; a.hp = hp; a.Ho = Ho; a.Wo = Wo; a.out_ld = out_ld; a.Cout = L.cout; a.tiles_x = (a.Wo + 31) / 32;
        a.NS = L.NS; a.nsub = (L.cout + 31) / 32;
        rc = launch_stem2_cfg<1, ImgU8, false>(a, a.tiles_x * ((a.Ho + 3) / 4), 0);
    } else if (imgf4) rc = launch_stem2_fused(E, L, S, fscale != 0, f0, f1, a4, wp, hp, dy.as<float>(), out_ld, 0);
    else rc = launch_stem2_fused(E, L, S, fscale != 0, u0, u1, a4, wp, hp, dy.as<float>(), out_ld, 0);
    return v2_finish("op_v2_stem", rc, [&] { return dy.down(out); });
}

// k2_flow_accum<S, FIRST, MUL>: D [hh / S][wh / S][4] into the running flow acc [hh][wh][4]
int rife_hip_op_v2_flow_accum(int gpuid, int S, int first, int mul, const float* D, int wh, int hh, float* acc) {
    int rc;
    if (!D || !acc) return fail(RIFE_HIP_EINVAL, "op_v2_flow_accum: null argument");
    const int key = S * 4 + (first ? 2 : 0) + (mul ? 1 : 0);
    if (key != 8 * 4 + 2 && key != 4 * 4 && key != 2 * 4 && key != 1 * 4 && key != 4 * 4 + 3 && key != 2 * 4 + 1)
        return fail(RIFE_HIP_EINVAL, "op_v2_flow_accum: run_v2_ifnet launches <8, first>, <4>, <2>, <1> and, for rife-v3.x, <4, first, mul>, <2, mul>");
    if (wh <= 0 || hh <= 0 || wh % 16 || hh % 16 || (long long)wh * hh >= (1ll << 25)) return fail(RIFE_HIP_EINVAL, "op_v2_flow_accum: the running flow is half of a frame padded to 32n");
    if ((rc = check_device(gpuid))) return rc;
    V2Buf dd, da;
    hipError_t e = dd.up(D, (size_t)(wh / S) * (hh / S) * 16);
    if (e == hipSuccess) e = da.up(acc, (size_t)wh * hh * 16);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_flow_accum: ") + hipGetErrorString(e));
    const dim3 g = grid2d(wh, hh), b(256);
    const float4* const d4 = dd.as<const float4>();
    float4* const a4 = da.as<float4>();
    if (key == 8 * 4 + 2) hipLaunchKernelGGL((k2_flow_accum<8, true>), g, b, 0, 0, d4, a4, wh, hh);
    else if (key == 4 * 4) hipLaunchKernelGGL((k2_flow_accum<4, false>), g, b, 0, 0, d4, a4, wh, hh);
    else if (key == 2 * 4) hipLaunchKernelGGL((k2_flow_accum<2, false>), g, b, 0, 0, d4, a4, wh, hh);
    else if (key == 1 * 4) hipLaunchKernelGGL((k2_flow_accum<1, false>), g, b, 0, 0, d4, a4, wh, hh);
    else if (key == 4 * 4 + 3) hipLaunchKernelGGL((k2_flow_accum<4, true, true>), g, b, 0, 0, d4, a4, wh, hh);
    else hipLaunchKernelGGL((k2_flow_accum<2, false, true>), g, b, 0, 0, d4, a4, wh, hh);
    return v2_finish("op_v2_flow_accum", 0, [&] { return da.down(acc); });
}

// the ContextNet's flow pyramids and warps as run_v2_synth launches them: batch = 0 the k2_flow_half chain and four k2_warp_nhwc launches per frame, batch = 1 both chains and
// ONE k2_warp_nhwc_batch launch.  feat / fl: [4 frame + level]; cat: B1..B4
int rife_hip_op_v2_ctx_warps(int gpuid, int batch, const float* acc, int wp, int hp, const float* const* feat, float* const* fl, float* const* cat) {
    int rc;
    if (!acc || !feat || !fl || !cat) return fail(RIFE_HIP_EINVAL, "op_v2_ctx_warps: null argument");
    for (int z = 0; z < 8; z++) if (!feat[z] || !fl[z] || !cat[z & 3]) return fail(RIFE_HIP_EINVAL, "op_v2_ctx_warps: null tensor");
    if ((rc = v2_frame_dims("op_v2_ctx_warps", 0, wp, hp))) return rc;
    if ((rc = check_device(gpuid))) return rc;
    static const int cat_ld[4] = {128, 256, 512, 1024}, cat_off[4] = {64, 128, 256, 512}, lvl_c[4] = {32, 64, 128, 256};      // run_v2_synth
    const int wh = wp / 2, hh = hp / 2;
    V2Buf da, df[8], dl[8], dc[4];
    hipError_t e = da.up(acc, (size_t)wh * hh * 16);
    for (int z = 0; z < 8 && e == hipSuccess; z++) {
        const size_t np = (size_t)(wp >> ((z & 3) + 2)) * (hp >> ((z & 3) + 2));
        e = df[z].up(feat[z], np * lvl_c[z & 3] * 4);
        if (e == hipSuccess) e = dl[z].up(fl[z], np * 8);
    }
    for (int l = 0; l < 4 && e == hipSuccess; l++) e = dc[l].up(cat[l], (size_t)(wp >> (l + 2)) * (hp >> (l + 2)) * cat_ld[l] * 4);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_ctx_warps: ") + hipGetErrorString(e));
    auto chain = [&](int im) {
        hipLaunchKernelGGL(k2_flow_half<true>, grid2d(wh / 2, hh / 2), dim3(256), 0, 0, da.as<const float>(), im * 2, dl[4 * im].as<float2>(), wh, hh);
        for (int l = 1; l < 4; l++)
            hipLaunchKernelGGL(k2_flow_half<false>, grid2d((wh >> l) / 2, (hh >> l) / 2), dim3(256), 0, 0, dl[4 * im + l - 1].as<const float>(), 0, dl[4 * im + l].as<float2>(),
                               wh >> l, hh >> l);
    };
    if (batch) {
        chain(0); chain(1);
        WarpBatch wb;
        for (int im = 0; im < 2; im++)
            for (int l = 0; l < 4; l++) {
                const int z = 4 * im + l;
                wb.feat[z] = df[z].as<const float>(); wb.flow[z] = dl[z].as<const float2>(); wb.out[z] = dc[l].as<float>(); wb.C[z] = lvl_c[l]; wb.out_ld[z] = cat_ld[l];
                wb.out_coff[z] = cat_off[l] + im * lvl_c[l]; wb.w[z] = wp >> (l + 2); wb.h[z] = hp >> (l + 2);
            }
        const int W0 = wp >> 2, H0 = hp >> 2, ppb0 = 256 / (lvl_c[0] / 4);
        hipLaunchKernelGGL(k2_warp_nhwc_batch, dim3((W0 + ppb0 - 1) / ppb0, H0, 8), dim3(256), 0, 0, wb);
    } else
        for (int im = 0; im < 2; im++) {
            chain(im);
            for (int l = 0; l < 4; l++) {
                const int Hl = hp >> (l + 2), Wl = wp >> (l + 2), nq = lvl_c[l] / 4, ppb = 256 / nq;
                hipLaunchKernelGGL(k2_warp_nhwc, dim3((Wl + ppb - 1) / ppb, Hl), dim3(256), 0, 0, df[4 * im + l].as<const float>(), lvl_c[l], dl[4 * im + l].as<const float2>(),
                                   dc[l].as<float>(), cat_ld[l], cat_off[l] + im * lvl_c[l], Wl, Hl);
            }
        }
    return v2_finish("op_v2_ctx_warps", 0, [&] {
        hipError_t d = hipSuccess;
        for (int z = 0; z < 8 && d == hipSuccess; z++) d = dl[z].down(fl[z]);
        for (int l = 0; l < 4 && d == hipSuccess; l++) d = dc[l].down(cat[l]);
        return d;
    });
}

// k2_final (float_form = 0: the u8 w x h frame) / k2_final_float (the wp x hp float4 frame) between two guards of RIFE_HIP_TAIL_GUARD bytes
int rife_hip_op_v2_final(int gpuid, int float_form, const uint32_t* img0, const uint32_t* img1, int w, int h, const float* acc, const float* head, void* out) {
    int rc;
    if (!img0 || !img1 || !acc || !head || !out) return fail(RIFE_HIP_EINVAL, "op_v2_final: null argument");
    if (w <= 0 || h <= 0) return fail(RIFE_HIP_EINVAL, "op_v2_final: a frame size");
    const long long wpl = align_up((long long)w, 32), hpl = align_up((long long)h, 32);
    if (wpl * hpl >= (1ll << 27)) return fail(RIFE_HIP_EINVAL, "op_v2_final: frames stay below 2^27 padded pixels");
    if ((rc = check_device(gpuid))) return rc;
    const int wp = (int)wpl, hp = (int)hpl;
    const size_t P = (size_t)wp * hp, nframe = float_form ? P * 16 : (size_t)w * h * 3, nout = nframe + 2 * (size_t)RIFE_HIP_TAIL_GUARD;
    V2Buf d0, d1, da, dh, dout;
    hipError_t e = d0.up(img0, P * 4);
    if (e == hipSuccess) e = d1.up(img1, P * 4);
    if (e == hipSuccess) e = da.up(acc, P / 4 * 16);
    if (e == hipSuccess) e = dh.up(head, P * 16);
    if (e == hipSuccess) e = dout.up(out, nout);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_final: ") + hipGetErrorString(e));
    uint8_t* const frame = dout.as<uint8_t>() + RIFE_HIP_TAIL_GUARD;
    if (float_form) hipLaunchKernelGGL(k2_final_float, grid2d(wp, hp), dim3(256), 0, 0, d0.as<const uint32_t>(), d1.as<const uint32_t>(), da.as<const float4>(), dh.as<const float4>(),
                                       reinterpret_cast<float4*>(frame), wp, hp);
    else hipLaunchKernelGGL(k2_final, grid2d(w, h), dim3(256), 0, 0, d0.as<const uint32_t>(), d1.as<const uint32_t>(), da.as<const float4>(), dh.as<const float4>(), frame, w, h, wp, hp);
    return v2_finish("op_v2_final", 0, [&] { return dout.down(out); });
}

// UHD mode's resamplers (run_v2_flow): what = 0 k2_image_half, a wp x hp frame -> float4 [hp / 2][wp / 2]; what = 1 k2_flow_up2_double, float4 [hp / 2][wp / 2] -> [hp][wp]
int rife_hip_op_v2_uhd(int gpuid, int what, const void* in, int wp, int hp, float* out) {
    int rc;
    if (!in || !out) return fail(RIFE_HIP_EINVAL, "op_v2_uhd: null argument");
    if (what != 0 && what != 1) return fail(RIFE_HIP_EINVAL, "op_v2_uhd: 0 = k2_image_half, 1 = k2_flow_up2_double");
    if ((rc = v2_frame_dims("op_v2_uhd", what, wp, hp))) return rc;      // the flow field of what = 1 is half of a padded frame
    if ((rc = check_device(gpuid))) return rc;
    const size_t P = (size_t)wp * hp;
    V2Buf di, dout;
    hipError_t e = di.up(in, what ? P / 4 * 16 : P * 4);
    if (e == hipSuccess) e = dout.up(out, what ? P * 16 : P / 4 * 16);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_uhd: ") + hipGetErrorString(e));
    if (what) hipLaunchKernelGGL(k2_flow_up2_double, grid2d(wp, hp), dim3(256), 0, 0, di.as<const float4>(), dout.as<float4>(), wp, hp);
    else hipLaunchKernelGGL(k2_image_half, grid2d(wp / 2, hp / 2), dim3(256), 0, 0, di.as<const uint32_t>(), dout.as<float4>(), wp, hp);
    return v2_finish("op_v2_uhd", 0, [&] { return dout.down(out); });
}

// conv_img_s2_kernel as run_v2_synth launches it: two = 0 one frame (gridDim.y = 1, grid capped at 8 workgroups per CU), two = 1 both frames (gridDim.y = 2, 4 per CU);
// cus > 0: the cap counts that many compute units instead of the chip's
int rife_hip_op_v2_conv_img(int gpuid, int two, int cus, const uint32_t* img0, const uint32_t* img1, int wp, int hp, const float* weight, const float* bias, const float* slope,
                            float* out0, float* out1) {
    int rc;
    if (!img0 || !weight || !bias || !slope || !out0 || (two && (!img1 || !out1))) return fail(RIFE_HIP_EINVAL, "op_v2_conv_img: null argument");
    if (cus < 0) return fail(RIFE_HIP_EINVAL, "op_v2_conv_img: a CU budget >= 0");
    if ((rc = v2_frame_dims("op_v2_conv_img", 0, wp, hp))) return rc;
    if (!all_fp16(weight, 32 * 27)) return fail(RIFE_HIP_EINVAL, "op_v2_conv_img: the frame kernel needs weights that are exactly fp16");
    if ((rc = check_device(gpuid))) return rc;
    V2Layer lay;
    ConvLayer& L = lay.L;
    L.cin = 3; L.cout = 32; L.stride = 2; L.deconv = false; L.epi = EPI_STORE; L.cls = "v2_context"; L.tag = 0;      // take() of load_v2 for ctxc[0]
    if ((rc = upload_layer(L, weight, bias, slope, 1.0f))) return rc;
    if (!(L.d_wimg != nullptr && trunk_h2() && process_switches().ctx0_img)) return fail(RIFE_HIP_EINVAL, "op_v2_conv_img: the product would not run conv_img_s2_kernel on this layer");
    const size_t P = (size_t)wp * hp, nout = P / 4 * 32 * 4;
    V2Buf d0, d1, o0, o1;
    hipError_t e = d0.up(img0, P * 4);
    if (e == hipSuccess) e = o0.up(out0, nout);
    if (e == hipSuccess && two) e = d1.up(img1, P * 4);
    if (e == hipSuccess && two) e = o1.up(out1, nout);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_v2_conv_img: ") + hipGetErrorString(e));
    ImgConvArgs ia;
    ia.img = d0.as<const uint32_t>(); ia.out = o0.as<float>(); ia.wpk = L.d_wimg; ia.bias = L.d_bias; ia.slope = L.d_slope;
    if (two) { ia.img1 = d1.as<const uint32_t>(); ia.out1 = o1.as<float>(); }
    ia.wp = wp; ia.hp = hp; ia.Wo = wp / 2; ia.Ho = hp / 2; ia.tiles_x = (ia.Wo + 31) / 32; ia.ntiles = ia.tiles_x * ia.Ho;
    const int nwg = std::max(1, std::min((ia.ntiles + 3) / 4, (two ? 4 : 8) * (cus > 0 ? cus : device_cus(true))));
    hipLaunchKernelGGL(conv_img_s2_kernel, dim3(nwg, two ? 2 : 1), dim3(256), 0, 0, ia);
    return v2_finish("op_v2_conv_img", 0, [&] {
        const hipError_t d = o0.down(out0);
        return d != hipSuccess || !two ? d : o1.down(out1);
    });
}

// launch_conv with a second tensor pair (x1 -> y1: gridDim.y = 2) or a second destination view (y2) on a layer built as load_v2 builds it.  x: NHWC [H][W][cin];
// y0 / y1: [Ho][Wo][y_ld], the layer's channels at y_coff; y2: [Ho][Wo][y2_ld] at y2_coff
int rife_hip_op_conv_pair(int gpuid, int cin, int cout, int stride, int deconv, int H, int W, const float* weight, const float* bias, const float* slope, const float* x0,
                          const float* x1, float* y0, float* y1, int y_ld, int y_coff, float* y2, int y2_ld, int y2_coff) {
    int rc;
    if (!weight || !bias || !slope || !x0 || !y0 || (x1 != nullptr) != (y1 != nullptr)) return fail(RIFE_HIP_EINVAL, "op_conv_pair: null argument, or one half of the second tensor pair");
    if (cin <= 0 || cout <= 0 || cin % 16 || cout % 4 || H <= 0 || W <= 0 || (long long)H * W >= (1 << 24)) return fail(RIFE_HIP_EINVAL, "op_conv_pair: 16n input channels, 4n output channels, a tensor size");
    if (deconv ? stride != 2 : (stride != 1 && stride != 2)) return fail(RIFE_HIP_EINVAL, "op_conv_pair: 3x3 stride 1 | 2, or the 4x4 stride-2 transposed layer");
    if (deconv && (x1 || y2)) return fail(RIFE_HIP_EINVAL, "op_conv_pair: the transposed layers have neither a two-tensor nor a two-destination form");
    if (y2 && (x1 || stride != 1)) return fail(RIFE_HIP_EINVAL, "op_conv_pair: the second destination is a form of the one-tensor stride-1 launch");
    if (y_ld % 4 || y_coff % 4 || y_coff < 0 || y_coff + cout > y_ld || (y2 && (y2_ld % 4 || y2_coff % 4 || y2_coff < 0 || y2_coff + cout > y2_ld)))
        return fail(RIFE_HIP_EINVAL, "op_conv_pair: the layer's channels must lie inside the destination views, at multiples of 4");
    const size_t nw = (size_t)cin * cout * (deconv ? 16 : 9);
    if ((x1 || y2) && !all_fp16(weight, nw)) return fail(RIFE_HIP_EINVAL, "op_conv_pair: the two-tensor and two-destination forms are split-f16 kernels: weights that are exactly fp16");
    V2Layer lay;
    ConvLayer& L = lay.L;
    L.cin = cin; L.cout = cout; L.stride = deconv ? 1 : stride; L.deconv = deconv != 0; L.epi = deconv ? EPI_DECONV : EPI_STORE; L.cls = "v2_op"; L.tag = 0;      // take() of load_v2
    if (y2) {                                    // dual_ok of run_v2_synth: where split-K would serve the layer the product copies the skip instead
        configure(L);
        const long nb = (long)((W + 31) / 32) * ((H + 7) / 8) * L.ntiles;
        const int nchunksh = cin / 16;           // what upload_layer gives a stride-1 layer of fp16 weights
        if (!(!process_switches().v2_skip_copy && trunk_h2() && L.NS <= 2 && !(L.NS == 2 && nb <= 64 && nchunksh >= 4)))
            return fail(RIFE_HIP_EINVAL, "op_conv_pair: the product would not give this layer a second destination at this size");
    }
    if ((rc = check_device(gpuid))) return rc;
    if ((rc = upload_layer(L, weight, bias, slope, 1.0f))) return rc;
    const int Ho = deconv ? 2 * H : (H - 1) / stride + 1, Wo = deconv ? 2 * W : (W - 1) / stride + 1;
    V2Buf dx0, dx1, dy0, dy1, dy2;
    hipError_t e = dx0.up(x0, (size_t)H * W * cin * 4);
    if (e == hipSuccess) e = dy0.up(y0, (size_t)Ho * Wo * y_ld * 4);
    if (e == hipSuccess && x1) e = dx1.up(x1, (size_t)H * W * cin * 4);
    if (e == hipSuccess && y1) e = dy1.up(y1, (size_t)Ho * Wo * y_ld * 4);
    if (e == hipSuccess && y2) e = dy2.up(y2, (size_t)Ho * Wo * y2_ld * 4);
    if (e != hipSuccess) return fail(RIFE_HIP_EHIP, std::string("op_conv_pair: ") + hipGetErrorString(e));
    const TensorView v2{dy2.as<float>(), y2_ld, y2_coff};
    rc = launch_conv(L, {dx0.as<float>(), cin, 0}, H, W, {dy0.as<float>(), y_ld, y_coff}, nullptr, 0, nullptr, 0, 0, x1 ? dx1.as<const float>() : nullptr,
                     y1 ? dy1.as<float>() : nullptr, y2 ? &v2 : nullptr);
    return v2_finish("op_conv_pair", rc, [&] {
        hipError_t d = dy0.down(y0);
        if (d == hipSuccess && y1) d = dy1.down(y1);
        if (d == hipSuccess && y2) d = dy2.down(y2);
        return d;
    });
}

}  // extern "C"

#endif  // RIFE_HIP_TEST_BUILD
