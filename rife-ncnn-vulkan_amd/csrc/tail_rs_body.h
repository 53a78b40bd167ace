// tail_rs_body.h: the body of tail_rs_kernel (tail_rs.h), included once per kernel that has it - the plain kernel, where the two TRS_MOTION_* macros are empty and the
// text is the kernel as it always was, token for token, and tail_rs_motion_kernel, where they store the pixel's final flow and blend weight.  No include guard on purpose.
// Contract with the including kernel: it provides `TailRsArgs a`, the compile-time constants `TAG` (ablation bits, 0 in the product) and `PX`, and the two hooks
//   TRS_MOTION_FLOW(FX, FY, F)   at the point where the pixel's final flow `f` is live (the step that issues the taps); FX, FY = the pixel, unclamped
//   TRS_MOTION_MASK(OX, OY, M)   at the two points where the blend weight `m` is formed; the body has `bool valid` (the lane's pixel is inside w x h) in scope there
// (the motion kernel also provides `MotionArgs mo`, which only its hooks name).  The body may `return`.  f is stored in the step that issues the taps, where it is live, and m a step later, where it is formed
// (finish_pixel and the last-pixel block): nothing is carried across the step for it.
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, li = lane & 31;

    const int nwg = gridDim.x, wg = blockIdx.x;
    const int u0 = (int)((long long)a.nunits * wg / nwg), u1 = (int)((long long)a.nunits * (wg + 1) / nwg);
    const int S = u1 - u0;
    if (S <= 0) return;

    if (tid < 32) reinterpret_cast<float*>(ldsb + TRS_LDS_BIAS)[tid] = a.bias[tid];      // (a global load in the combine phase would wait for every prefetch in flight)

    // this wave's matrix role: parity par, K half kh (chunks 2 kh, 2 kh + 1); its four taps and eight weight fragments
    const int par = wv & 3, kh = wv >> 2;
    f16x8 Wf[2][4];
    int tapdy[4], tapdx[4];
    {
        int n = 0;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            // head_uses(t, par) with a runtime parity: offsets 0 and (p ? +1 : -1) in each axis
            const int dy = t / 3 - 1, dx = t % 3 - 1, py = par >> 1, px = par & 1;
            const bool use = (dy == 0 || dy == (py ? 1 : -1)) && (dx == 0 || dx == (px ? 1 : -1));
            if (use) {
                // position of (t, par) in the packed pair order: pairs of earlier taps + earlier parities of this tap
                int idx = 0;
                for (int tt = 0; tt < 9; tt++)
                    for (int pp = 0; pp < 4; pp++) {
                        if (tt > t || (tt == t && pp >= par)) continue;
                        const int ddy = tt / 3 - 1, ddx = tt % 3 - 1, ppy = pp >> 1, ppx = pp & 1;
                        if ((ddy == 0 || ddy == (ppy ? 1 : -1)) && (ddx == 0 || ddx == (ppx ? 1 : -1))) idx++;
                    }
                // n is wave-uniform but not a compile-time constant per t: select by comparison below
#pragma unroll
                for (int s = 0; s < 4; s++)
                    if (s == n) {
                        tapdy[s] = dy + 1; tapdx[s] = dx + 1;
#pragma unroll
                        for (int c = 0; c < 2; c++)
                            Wf[c][s] = *reinterpret_cast<const f16x8*>(reinterpret_cast<const unsigned char*>(a.w) + ((size_t)(((2 * kh + c) * 16 + idx) * 2 + half) * 32 + li) * 16);
                    }
                n++;
            }
        }
    }

    // row loader role: 16-byte unit tid (and 512 + tid for tid < 32) of the 544 of a ring row: (segment, pixel, half)
    unsigned lsrc[2], ldst[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int u = min(tid + 512 * k, 543);
        const int seg = u / 68, within = u - seg * 68;
        const int px = within >> 1, pos = within & 1;
        lsrc[k] = (unsigned)seg * a.plane + (unsigned)(px * 32 + ((pos ^ ((px >> 3) & 1)) << 4));
        ldst[k] = (unsigned)(seg * TRS_SEG + px * 32 + pos * 16);
    }
    auto row_load = [&](int strip, int y, f32x4 (&r)[2]) {              // trunk row y (-1 .. Hq: the zero border rows exist) of the strip
        const unsigned base = (unsigned)((y + 1) * a.pitch + 32 * strip) * 32u;
        if (RIFE_ABL(TAG & TRS_NOROW)) { r[0] = r[1] = f32x4{0.f, 0.f, 0.f, 0.f}; return; }
        r[0] = *reinterpret_cast<const f32x4*>(a.in + base + lsrc[0]);
        if (tid < 32) r[1] = *reinterpret_cast<const f32x4*>(a.in + base + lsrc[1]);
    };
    auto row_store = [&](int y, const f32x4 (&r)[2]) {
        unsigned char* const d = ldsb + ((y + 1) & 3) * TRS_ROWB;
        *reinterpret_cast<f32x4*>(d + ldst[0]) = r[0];
        if (tid < 32) *reinterpret_cast<f32x4*>(d + ldst[1]) = r[1];
    };

    // pixel role: row prow (0..3) and column pcol (0..127) of the step's output block; a wave = 64 consecutive pixels of one row
    const int prow = tid >> 7, pcol = tid & 127;
    struct PixIn { float4 f; float m; };
    auto fm_load = [&](int strip, int q) -> PixIn {
        const int fy = min(4 * q + prow, a.hp - 1), fx = min(128 * strip + pcol, a.wp - 1);
        const size_t i = (size_t)fy * a.wp + fx;
        PixIn r;
        if (RIFE_ABL(TAG & TRS_NOFM)) { r.f = make_float4(0.25f * (float)(fx & 7), -0.5f, 1.5f, 0.75f); r.m = 0.1f; return r; }
        r.f = a.F[i]; r.m = a.M[i];
        return r;
    };

    int strip = u0 / a.Hq, q = u0 - strip * a.Hq;
    {   // first step of the range: rows q - 1, q, q + 1
        f32x4 r[2];
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) { row_load(strip, q + dy, r); row_store(q + dy, r); }
    }
    PixIn fm_cur = fm_load(strip, q);
    WarpLoads wa, wb; float mm_prev = 0.f; int pstrip = 0, pq = 0; bool have_prev = false;
    wa.r0 = wa.r1 = wb.r0 = wb.r1 = make_uint2(0u, 0u); wa.alpha = wa.beta = wb.alpha = wb.beta = 0.f; wa.l0 = wa.l1 = wb.l0 = wb.l1 = false;
    TRS_SYNC();

    for (int k = 0; k < S; k++) {
        int hf = half, l32 = li, ln = lane;
        asm volatile("" : "+v"(hf), "+v"(l32), "+v"(ln));               // opaque copies: nothing loop-invariant to hoist and spill (stem_rs.h)
        // the step after this one: its new trunk row and its F, M - loads that fly during the matrix phase
        int nstrip = strip, nq = q + 1;
        bool fresh = false;
        if (nq >= a.Hq) { nq = 0; nstrip++; fresh = true; }
        const bool has_next = k + 1 < S;
        f32x4 rnext[2];
        PixIn fm_next;
        if (has_next && !fresh) row_load(nstrip, nq + 1, rnext);
        if (has_next) fm_next = fm_load(nstrip, nq);

        // ---- deconvolution of trunk row q: this wave's parity and K half
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 2; c++) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int pxl = l32 + tapdx[s];
                const unsigned ad = (unsigned)(((q + tapdy[s]) & 3) * TRS_ROWB + (2 * (2 * kh + c)) * TRS_SEG + pxl * 32 + ((hf ^ ((pxl >> 3) & 1)) << 4));
                const f16x8 ah = *reinterpret_cast<const f16x8*>(ldsb + ad);
                const f16x8 al = *reinterpret_cast<const f16x8*>(ldsb + ad + TRS_SEG);
                if (RIFE_ABL(TAG & TRS_NOMATH)) { acc[s] += (float)ah[0] + (float)al[1] + (float)Wf[c][s][2]; continue; }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Wf[c][s], ah, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Wf[c][s], al, acc, 0, 0, 0);
            }
        }
        if (kh == 1) {
            f32x4* const sd = reinterpret_cast<f32x4*>(ldsb + TRS_LDS_PART + par * 4096 + ln * 16);
#pragma unroll
            for (int qd = 0; qd < 4; qd++) sd[qd * 64] = f32x4{acc[4 * qd], acc[4 * qd + 1], acc[4 * qd + 2], acc[4 * qd + 3]};
        }
        TRS_SYNC();
        if (kh == 0) {
            // + the other K half + bias, PixelShuffle: deconv channel 8 qd + 4 half + kk = flow channel 2 qd + half at sub-position kk of the
            // trunk pixel's 2 x 2 block of this parity
            const f32x4* const sd = reinterpret_cast<const f32x4*>(ldsb + TRS_LDS_PART + par * 4096 + ln * 16);
            float* const dl = reinterpret_cast<float*>(ldsb + TRS_LDS_DELTA);
            const int py = par >> 1, px = par & 1;
#pragma unroll
            for (int qd = 0; qd < 3; qd++) {
                const f32x4 p = sd[qd * 64];
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(ldsb + TRS_LDS_BIAS + (8 * qd + 4 * hf) * 4);
                const int ch = 2 * qd + hf;
                if (ch < 5) {
#pragma unroll
                    for (int kk = 0; kk < 4; kk++)
                        dl[(ch * 4 + 2 * py + (kk >> 1)) * 128 + 4 * l32 + 2 * px + (kk & 1)] = (acc[4 * qd + kk] + p[kk]) + b4[kk];
                }
            }
        }
        TRS_SYNC();

        // ---- this thread's pixel of step k: F, M + deltas, tap loads issued
        const int fy = 4 * q + prow, fx = 128 * strip + pcol;
        WarpLoads na, nb; float mm_now;
        {
            const float* const dl = reinterpret_cast<const float*>(ldsb + TRS_LDS_DELTA) + prow * 128 + pcol;
            float4 f = fm_cur.f;
            f.x = f.x + dl[0 * 512]; f.y = f.y + dl[1 * 512]; f.z = f.z + dl[2 * 512]; f.w = f.w + dl[3 * 512];
            mm_now = fm_cur.m + dl[4 * 512];
            TRS_MOTION_FLOW(fx, fy, f)
            const int cy = min(fy, a.hp - 1), cx = min(fx, a.wp - 1);    // out-of-frame lanes compute on clamped coordinates and store nothing
            if (RIFE_ABL(TAG & TRS_NOTAPS)) {
                na.r0 = na.r1 = nb.r0 = nb.r1 = make_uint2((unsigned)cx * 0x10101u, (unsigned)cy * 0x10101u);
                na.alpha = nb.alpha = f.x - floorf(f.x); na.beta = nb.beta = f.y - floorf(f.y); na.l0 = nb.l0 = true; na.l1 = nb.l1 = false;
            } else {
            nb = warp_issue(a.img1, cx, cy, f.z, f.w, a.wp, a.hp);
            na = warp_issue(a.img0, cx, cy, f.x, f.y, a.wp, a.hp);
            }
        }
        // ---- the pixel of step k - 1: its taps have been in flight for a whole step
        auto finish_pixel = [&](const WarpLoads& ta, const WarpLoads& tb, float mm, int ostrip, int oq) {
            const int oy = 4 * oq + prow, oxb = 128 * ostrip + 64 * ((tid >> 6) & 1), ox = oxb + ln;
            if (oy >= a.h_ || oxb >= a.w_) return;                       // wave-uniform
            if (RIFE_ABL(TAG & TRS_NOPIX)) { if (mm == 123.456f && ta.alpha == 7.f && tb.r0.x == 99u) a.out[0] = 1; return; }
            const bool valid = ox < a.w_ && (!RIFE_ABL(TAG & TRS_NOSTORE) || mm == 123.456f);
            const float m = 1.f / (1.f + expf(-mm));
            const float rm = 1.0f - m;
            TRS_MOTION_MASK(ox, oy, m)
            const float3 w1 = warp_finish<px_depth(PX)>(tb);
            const float3 w0 = warp_finish<px_depth(PX)>(ta);
            const float r = w0.x * m + w1.x * rm, g = w0.y * m + w1.y * rm, b = w0.z * m + w1.z * rm;
            if (px_deep(PX)) { if (valid) trs_put_px10<PX>(a.out, (unsigned)(oy * a.w_ + ox), quant10(r, g, b)); return; }
            if (PX == 4) {
                const float al = warp_finish_a(ta) * m + warp_finish_a(tb) * rm;
                if (valid) trs_store_dword(a.out, (unsigned)(oy * a.w_ + ox) * 4u, quant8(r) | (quant8(g) << 8) | (quant8(b) << 16) | (quant8(al) << 24));
                return;
            }
            const uint32_t pk = (uint32_t)min(max((int)(r * 255.f + 0.5f), 0), 255) | ((uint32_t)min(max((int)(g * 255.f + 0.5f), 0), 255) << 8) |
                                ((uint32_t)min(max((int)(b * 255.f + 0.5f), 0), 255) << 16);
            const unsigned orow = (unsigned)(oy * a.w_ + oxb) * 3u;     // byte offset of the segment (frames stay below 4 GB)
            if ((a.w_ & 3) == 0 && oxb + 64 <= a.w_) {
                // 64 pixels = 192 bytes = 48 dwords: dword d takes bytes from pixels 4d/3 and 4d/3 + 1
                const int d = ln < 48 ? ln : 0;
                const int pa = (4 * d) / 3, sh = 8 * (4 * d - 3 * pa);
                const uint32_t va = (uint32_t)__shfl((int)pk, pa), vb = (uint32_t)__shfl((int)pk, pa + 1);
                const uint32_t word = sh == 0 ? (va | (vb << 24)) : ((va >> sh) | (vb << (24 - sh)));
                if (ln < 48 && (!RIFE_ABL(TAG & TRS_NOSTORE) || mm == 123.456f)) trs_store_dword(a.out, orow + 4u * (unsigned)ln, word);
            } else if (valid) {
                const unsigned o = orow + 3u * (unsigned)ln;
                trs_store_byte(a.out, o, pk & 255u); trs_store_byte(a.out, o + 1, (pk >> 8) & 255u); trs_store_byte(a.out, o + 2, pk >> 16);
            }
        };
        if (have_prev) finish_pixel(wa, wb, mm_prev, pstrip, pq);
        wa = na; wb = nb; mm_prev = mm_now; pstrip = strip; pq = q; have_prev = true;

        // ---- ring for the next step
        if (has_next) {
            if (fresh) {
                TRS_SYNC();                                              // everybody is done with this strip's rows
                f32x4 r[2];
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) { row_load(nstrip, nq + dy, r); row_store(nq + dy, r); }
            } else row_store(nq + 1, rnext);
            fm_cur = fm_next;
        }
        TRS_SYNC();
        strip = nstrip; q = nq;
    }
    // the last pixel
    {
        const int ln = lane;
        const int oy = 4 * pq + prow, oxb = 128 * pstrip + 64 * ((tid >> 6) & 1), ox = oxb + ln;
        if (!(oy >= a.h_ || oxb >= a.w_)) {
            const bool valid = ox < a.w_;
            const float m = 1.f / (1.f + expf(-mm_prev));
            const float rm = 1.0f - m;
            TRS_MOTION_MASK(ox, oy, m)
            const float3 w1 = warp_finish<px_depth(PX)>(wb);
            const float3 w0 = warp_finish<px_depth(PX)>(wa);
            const float r = w0.x * m + w1.x * rm, g = w0.y * m + w1.y * rm, b = w0.z * m + w1.z * rm;
            if (px_deep(PX)) { if (valid) trs_put_px10<PX>(a.out, (unsigned)(oy * a.w_ + ox), quant10(r, g, b)); return; }
            if (PX == 4) {
                const float al = warp_finish_a(wa) * m + warp_finish_a(wb) * rm;
                if (valid) trs_store_dword(a.out, (unsigned)(oy * a.w_ + ox) * 4u, quant8(r) | (quant8(g) << 8) | (quant8(b) << 16) | (quant8(al) << 24));
                return;
            }
            const uint32_t pk = (uint32_t)min(max((int)(r * 255.f + 0.5f), 0), 255) | ((uint32_t)min(max((int)(g * 255.f + 0.5f), 0), 255) << 8) |
                                ((uint32_t)min(max((int)(b * 255.f + 0.5f), 0), 255) << 16);
            const unsigned orow = (unsigned)(oy * a.w_ + oxb) * 3u;
            if ((a.w_ & 3) == 0 && oxb + 64 <= a.w_) {
                const int d = ln < 48 ? ln : 0;
                const int pa = (4 * d) / 3, sh = 8 * (4 * d - 3 * pa);
                const uint32_t va = (uint32_t)__shfl((int)pk, pa), vb = (uint32_t)__shfl((int)pk, pa + 1);
                const uint32_t word = sh == 0 ? (va | (vb << 24)) : ((va >> sh) | (vb << (24 - sh)));
                if (ln < 48) trs_store_dword(a.out, orow + 4u * (unsigned)ln, word);
            } else if (valid) {
                const unsigned o = orow + 3u * (unsigned)ln;
                trs_store_byte(a.out, o, pk & 255u); trs_store_byte(a.out, o + 1, (pk >> 8) & 255u); trs_store_byte(a.out, o + 2, pk >> 16);
            }
        }
    }
