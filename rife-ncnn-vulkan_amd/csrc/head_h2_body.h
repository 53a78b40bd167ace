// head_h2_body.h: the body of head_h2_kernel (head_h2.h), included once per kernel that has it - the plain kernel, where HD_MOTION is empty and the text is the kernel as
// it always was, token for token, and head_h2_motion_kernel, where it stores the finished pixel's final flow and blend weight.  No include guard on purpose.
// Contract with the including kernel: it provides `ConvArgs a`, `FinalArgs fa`, the compile-time constants `EPI`, `S16IN` and `PX`, and the hook
//   HD_MOTION(FX, FY, F, M)   in the EPI_FINAL epilogue, inside the lane's `valid` branch (pixel FX, FY inside w x h), where its final flow `f` and blend weight `m` exist
// (the motion kernel also provides `MotionArgs mo`, which only its hook names).  The body may `return`, and defines and undefines its own HD_* helper macros.
    constexpr int IH = 10, IW = 34, CC = 16, NT = 32;
    constexpr int PIXB = 80;
    constexpr int IN_F4 = IH * IW * 4;
    constexpr int W_16 = 16 * 2 * NT;                        // 16-byte units per weight chunk (16 pairs)
    constexpr int NIN = (IN_F4 + 511) / 512, NW = (W_16 + 511) / 512;
    constexpr int INB = IH * IW * PIXB;
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
    unsigned char* const lw = ldsb + 2 * INB;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, li = lane & 31;
    int L;
    {
        const int n = gridDim.x, b = blockIdx.x;
        const int q = n >> 3, r = n & 7, xcd = b & 7;
        L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    }
    const int tile = L / a.nz, ntile = L - tile * a.nz;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int oy0 = ty * 8, ox0 = tx * 32;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;

    int goff[NIN];
    unsigned inside = 0;
#pragma unroll
    for (int k = 0; k < NIN; k++) {
        const int idx = tid + k * 512;
        const int p = idx >> 2, q = idx & 3;
        const int py = p / IW, px = p - py * IW;
        const int gy = iy0 + py, gx = ix0 + px;
        const bool ok = idx < IN_F4 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        // S16 planes: quarter q of a pixel's chunk = 16 bytes of the hi (q < 2) or lo plane; offsets in floats; border and ragged edge are stored zeros
        if (S16IN) goff[k] = idx < IN_F4 ? (int)((q >> 1) * (a.s16_plane / 4)) + ((gy + 1) * a.s16_pitch + gx + 1) * 8 + (q & 1) * 4 : 0;
        else goff[k] = ok ? (gy * a.W + gx) * a.in_ld + a.in_coff + q * 4 : a.in_coff;
        inside |= ok ? (1u << k) : 0u;
    }
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(a.wpk) + (size_t)ntile * a.nchunks * W_16;

    f32x4 rin[NIN], rw[NW];
#define HD_ISSUE_IN(CH)                                                                                     \
    _Pragma("unroll") for (int k = 0; k < NIN; k++) rin[k] = *reinterpret_cast<const f32x4*>(a.in + goff[k] + (S16IN ? (size_t)(CH) * (a.s16_plane / 2) : (size_t)(CH) * CC));
#define HD_ISSUE_W(CH)                                                                                      \
    _Pragma("unroll") for (int k = 0; k < NW; k++) rw[k] = wsrc[(size_t)(CH) * W_16 + tid + k * 512];
#define HD_WRITE_IN(BUFP)                                                                                   \
    _Pragma("unroll") for (int k = 0; k < NIN; k++) {                                                       \
        const int idx = tid + k * 512;                                                                      \
        const int p = idx >> 2, q = idx & 3;                                                                \
        if (S16IN) {                                                                                        \
            if (IN_F4 % 512 == 0 || idx < IN_F4) *reinterpret_cast<f32x4*>((BUFP) + p * PIXB + q * 16) = rin[k]; \
            continue;                                                                                       \
        }                                                                                                   \
        f16x4 hi4, lo4;                                                                                     \
        _Pragma("unroll") for (int e = 0; e < 4; e++) {                                                     \
            const float v = ((inside >> k) & 1u) ? rin[k][e] : 0.f;                                         \
            const _Float16 h = (_Float16)v;                                                                 \
            hi4[e] = h;                                                                                     \
            lo4[e] = (_Float16)(v - (float)h);                                                              \
        }                                                                                                   \
        if (IN_F4 % 512 == 0 || idx < IN_F4) {                                                              \
            *reinterpret_cast<f16x4*>((BUFP) + p * PIXB + q * 8) = hi4;                                     \
            *reinterpret_cast<f16x4*>((BUFP) + p * PIXB + 32 + q * 8) = lo4;                                \
        }                                                                                                   \
    }
#define HD_WRITE_W() _Pragma("unroll") for (int k = 0; k < NW; k++) reinterpret_cast<f32x4*>(lw)[tid + k * 512] = rw[k];
#define HD_TAPS(BUFP, T0, T1)                                                                               \
    {                                                                                                       \
        const unsigned char* ab_ = (BUFP) + (wv * IW + li) * PIXB + half * 16;                              \
        const unsigned char* bb_ = lw + (half * NT + li) * 16;                                              \
        _Pragma("unroll") for (int t = (T0); t < (T1); t++) {                                               \
            const f16x8 ah = *reinterpret_cast<const f16x8*>(ab_ + ((t / 3) * IW + (t % 3)) * PIXB);        \
            const f16x8 al = *reinterpret_cast<const f16x8*>(ab_ + ((t / 3) * IW + (t % 3)) * PIXB + 32);   \
            _Pragma("unroll") for (int par = 0; par < 4; par++)                                             \
                if (head_uses(t, par)) {                                                                    \
                    const f16x8 bw = *reinterpret_cast<const f16x8*>(bb_ + head_pair_index(t, par) * 2 * NT * 16); \
                    acc[par] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bw, ah, acc[par], 0, 0, 0);           \
                    acc[par] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bw, al, acc[par], 0, 0, 0);           \
                }                                                                                           \
        }                                                                                                   \
    }

    f32x16 acc[4];
#pragma unroll
    for (int n = 0; n < 4; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[n][r] = 0.f;

    static_assert(W_16 % 512 == 0, "weight slab must be a whole number of 512-thread passes");
    const int nch = a.nchunks;
    HD_ISSUE_IN(0)
    HD_ISSUE_W(0)
    HD_WRITE_IN(ldsb)
    HD_WRITE_W()
    if (nch > 1) { HD_ISSUE_IN(1) HD_ISSUE_W(1) }
    __syncthreads();
    for (int ch = 0; ch < nch; ch++) {
        unsigned char* cur = ldsb + (ch & 1) * INB;
        unsigned char* oth = ldsb + ((ch & 1) ^ 1) * INB;
        HD_TAPS(cur, 0, 4)
        if (ch + 1 < nch) { HD_WRITE_IN(oth) }
        if (ch + 2 < nch) { HD_ISSUE_IN(ch + 2) }
        HD_TAPS(cur, 4, 9)
        if (ch + 1 < nch) {
            __syncthreads();
            HD_WRITE_W()
            if (ch + 2 < nch) { HD_ISSUE_W(ch + 2) }
            __syncthreads();
        }
    }
#undef HD_ISSUE_IN
#undef HD_ISSUE_W
#undef HD_WRITE_IN
#undef HD_WRITE_W
#undef HD_TAPS

#ifndef HEAD_ABL
#define HEAD_ABL 0
#endif
    if (EPI == EPI_FINAL || EPI == EPI_DECONV_PS) {
        if (EPI == EPI_FINAL && RIFE_ABL(HEAD_ABL & 1)) {     // ablation: no tail at all (keep the accumulators alive)
            float sacc = 0.f;
#pragma unroll
            for (int par = 0; par < 4; par++)
#pragma unroll
                for (int r = 0; r < 16; r++) sacc += acc[par][r];
            if (sacc == 123.456f) fa.out[0] = 1;
            return;
        }
        // Per parity the lane holds deconv channels 8q + 4 half + k = PixelShuffle channel 2q + half at sub-position k of one trunk
        // pixel, i.e. a 4 x 4 block of full-resolution flow deltas spread over a lane pair.  Finishing the pixels in that layout
        // means 64-byte-strided F reads, scattered image taps and byte stores, so the wave first transposes its 4 rows x 128
        // columns of (dx, dy, dz, dw, dm) through LDS (two rows at a time; the staging buffers are free now) and then runs the
        // body of k_final with one lane per pixel along a row: F / M reads and the warp taps are row-contiguous and the u8
        // output leaves as whole dwords.
        __syncthreads();
        constexpr int NPL = EPI == EPI_FINAL ? 5 : 6;      // flow3 channel 5 is never used by the graph tail; the flow{b} blobs keep it
        float* const reg = reinterpret_cast<float*>(ldsb) + wv * (NPL * 2 * 128);
        const int oy = oy0 + wv;
#pragma unroll
        for (int py = 0; py < 2; py++) {
#pragma unroll
            for (int px = 0; px < 2; px++) {
                const int par = 2 * py + px;
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(a.bias + 8 * q + 4 * half);
                    if (EPI == EPI_FINAL && q == 2 && half == 1) continue;
#pragma unroll
                    for (int k = 0; k < 4; k++) reg[((2 * q + half) * 2 + (k >> 1)) * 128 + 4 * li + 2 * px + (k & 1)] = acc[par][4 * q + k] + b4[k];
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ky = 0; ky < 2; ky++) {
                const int fy = 4 * oy + 2 * py + ky;
#pragma unroll
                for (int cb = 0; cb < 2; cb++) {
                    const int col = 64 * cb + lane;
                    const int fxb = 4 * ox0 + 64 * cb, fx = fxb + lane;
                    const float dx = reg[(0 * 2 + ky) * 128 + col], dy = reg[(1 * 2 + ky) * 128 + col], dz = reg[(2 * 2 + ky) * 128 + col];
                    const float dw = reg[(3 * 2 + ky) * 128 + col], dm = reg[(4 * 2 + ky) * 128 + col];
                    if (EPI == EPI_DECONV_PS) {                  // flow{b} tensor [4 Ho][4 Wo][8]: 32 contiguous bytes per lane, 2 KB per wave
                        const float d5 = reg[(5 * 2 + ky) * 128 + col];
                        if (oy < a.Ho && fx < 4 * a.Wo) {
                            float* o = a.out + ((size_t)fy * (4 * a.Wo) + fx) * a.out_ld + a.out_coff;
                            *reinterpret_cast<f32x4*>(o) = f32x4{dx, dy, dz, dw};
                            *reinterpret_cast<float2*>(o + 4) = make_float2(dm, d5);
                        }
                        continue;
                    }
                    if (fy >= fa.h || fxb >= fa.w) continue;     // wave-uniform
                    const bool valid = fx < fa.w;
                    uint32_t pk = 0;
                    if (valid) {
                        const size_t i = (size_t)fy * fa.wp + fx;
                        float4 f = RIFE_ABL(HEAD_ABL & 2) ? make_float4(0.1f, 0.2f, 0.3f, 0.4f) : fa.F[i];
                        f.x = f.x + dx; f.y = f.y + dy; f.z = f.z + dz; f.w = f.w + dw;
                        const float mm = (RIFE_ABL(HEAD_ABL & 2) ? 0.5f : fa.M[i]) + dm;
                        const float m = RIFE_ABL(HEAD_ABL & 8) ? mm * 0.01f : 1.f / (1.f + expf(-mm));
                        const float rm = 1.0f - m;
                        HD_MOTION(fx, fy, f, m)
                        if (PX == 4) {      // RGBA8: alpha from the same taps as the colour, one dword per pixel
                            const WarpLoads t1 = warp_issue(fa.img1, fx, fy, f.z, f.w, fa.wp, fa.hp);
                            const WarpLoads t0 = warp_issue(fa.img0, fx, fy, f.x, f.y, fa.wp, fa.hp);
                            const float3 w1 = warp_finish<8>(t1);
                            const float3 w0 = warp_finish<8>(t0);
                            const float r = w0.x * m + w1.x * rm, g = w0.y * m + w1.y * rm, b = w0.z * m + w1.z * rm;
                            const float al = warp_finish_a(t0) * m + warp_finish_a(t1) * rm;
                            const uint32_t q = quant8(r) | (quant8(g) << 8) | (quant8(b) << 16) | (quant8(al) << 24);
                            uint8_t* o = fa.out + ((size_t)fy * fa.w + fx) * 4;      // byte stores: a device frame may sit at any address
                            o[0] = (uint8_t)q; o[1] = (uint8_t)(q >> 8); o[2] = (uint8_t)(q >> 16); o[3] = (uint8_t)(q >> 24);
                            continue;
                        }
                        const float3 w1 = RIFE_ABL(HEAD_ABL & 4) ? make_float3(f.z, f.w, f.z) : warp_rgbx<px_depth(PX)>(fa.img1, fx, fy, f.z, f.w, fa.wp, fa.hp);
                        const float3 w0 = RIFE_ABL(HEAD_ABL & 4) ? make_float3(f.x, f.y, f.x) : warp_rgbx<px_depth(PX)>(fa.img0, fx, fy, f.x, f.y, fa.wp, fa.hp);
                        const float r = w0.x * m + w1.x * rm, g = w0.y * m + w1.y * rm, b = w0.z * m + w1.z * rm;
                        if (px_deep(PX)) { store_px10<PX>(fa.out, (size_t)fy * fa.w + fx, quant10(r, g, b)); continue; }
                        pk = (uint32_t)min(max((int)(r * 255.f + 0.5f), 0), 255) | ((uint32_t)min(max((int)(g * 255.f + 0.5f), 0), 255) << 8) |
                             ((uint32_t)min(max((int)(b * 255.f + 0.5f), 0), 255) << 16);
                    }
                    if (PX) continue;
                    uint8_t* const orow = fa.out + ((size_t)fy * fa.w + fxb) * 3;
                    if ((fa.w & 3) == 0 && fxb + 64 <= fa.w) {
                        // 64 pixels = 192 bytes = 48 dwords: dword d takes bytes from pixels 4d/3 and 4d/3 + 1
                        const int d = lane < 48 ? lane : 0;
                        const int pa = (4 * d) / 3, sh = 8 * (4 * d - 3 * pa);
                        const uint32_t va = (uint32_t)__shfl((int)pk, pa), vb = (uint32_t)__shfl((int)pk, pa + 1);
                        const uint32_t word = sh == 0 ? (va | (vb << 24)) : ((va >> sh) | (vb << (24 - sh)));
                        if (lane < 48) reinterpret_cast<uint32_t*>(orow)[lane] = word;
                    } else if (valid) {
                        uint8_t* o = orow + lane * 3;
                        o[0] = (uint8_t)(pk & 255u); o[1] = (uint8_t)((pk >> 8) & 255u); o[2] = (uint8_t)(pk >> 16);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    // epilogue: deconv pixel (2oy+py, 2ox+px), channels c0..c0+3 of this 32-wide N-tile
    const int oy = oy0 + wv, ox = ox0 + li;
    const bool pok = oy < a.Ho && ox < a.Wo;
#pragma unroll
    for (int par = 0; par < 4; par++) {
        const int py = par >> 1, px = par & 1;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c0 = ntile * 32 + 8 * q + 4 * half;
            const bool ok = pok && c0 < a.Cout;
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(a.bias + c0);
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = acc[par][4 * q + k] + b4[k];
            if (EPI == EPI_DECONV_PS) {          // one PixelShuffle group c = c0>>2 -> a 2x2 block of the flow tensor [4H][4W][8]
                const int c = c0 >> 2;
                const int fy = 2 * (2 * oy + py), fx = 2 * (2 * ox + px);
                if (ok) {
#pragma unroll
                    for (int k = 0; k < 4; k++) a.out[((size_t)(fy + (k >> 1)) * (4 * a.Wo) + fx + (k & 1)) * a.out_ld + a.out_coff + c] = v[k];
                }
            } else {
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(a.slope + c0);
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = EPI == EPI_DECONV_SIG ? 1.f / (1.f + expf(-v[k])) : (v[k] < 0.f ? v[k] * s4[k] : v[k]);
                if (ok) *reinterpret_cast<f32x4*>(a.out + ((size_t)(2 * oy + py) * (2 * a.Wo) + 2 * ox + px) * a.out_ld + a.out_coff + c0) = v;
            }
        }
    }
