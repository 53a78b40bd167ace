"""The fused tails of rife-v4.6 restated in float64 (no GPU): the reference and the case table of tests/test_gpu_tail_parity.py, next to tests/s16_ref.py (layout,
split, pack) and tests/s16_ends_ref.py (head_ps).

What the kernels compute from the last trunk tensor x of block 3 (csrc/tail_rs.h, csrc/head_h2.h EPI_FINAL, csrc/elementwise.h k_final / k_final_px):
  d = head_ps(x, w, b)[:5];  F += d[:4];  M += d[4];  m = 1 / (1 + exp(-M));  w0 = Warp(img0, F.xy), w1 = Warp(img1, F.zw) with the clamp-then-alpha rule of
  warp_issue (both taps clamped to the padded frame, alpha and beta from the clamped first tap);  v = w0 m + w1 (1 - m);  code = clip(floor(v top + 0.5), 0, top),
  top = 255 or 1023; the alpha of RGBA8 the same way from byte 3; cropped to w x h and packed in the format's layout.

A quantised frame is held byte for byte EXCEPT where the float64 value v top + 0.5 lies within tau of an integer (a rounding boundary); there one code either way
is allowed.  tau per pixel = 2^-6 code x max(1, |alpha|, |beta|) over both warps: the fp32 chain has about 20 roundings of 2^-24 of full scale (the unpack by
1 / top, six lerp steps per warp, the blend, expf to 2 ulp, the quantiser) = 1.2e-3 code at 10 bits, 2^-6 is 13 times that, and a clamped tap pair
(v0 (1 - alpha) + v0 alpha) multiplies the rounding by |alpha|.  Where the flow deltas are not exact tau gains g (4e-6 max|d| + 1e-6): the bar of the head's dense
cases (tests/test_gpu_s16_ends.py) times g = the larger of the images' largest step between neighbouring pixels and top / 4, the mask's slope.

Three kinds of case, each a function of (w, h, depth), cached per process:
  planted  the lo planes ALONE carry the flow deltas: channels in pairs with hi = +h, -h (h an f16 in (16, 32)) and equal integer weights, so the hi products cancel
           exactly; lo = k 2^-10, k = 1..7.  Everything on the grid 2^-10 and every partial sum below 2^24 grid steps: fp32 sums are exact in any order, so all four
           kernels see the same deltas, and a lost lo plane, lo product or K partial sum moves the frame by many codes (asserted per case, below).
  dense    Gaussian activations and fp16 Gaussian weights (s16_ends_ref.head_gauss_case) scaled to max|d| < 4 px: the hi path, which planted cancels.
  far      the planted trunk with flows that leave the padded frame, a few by hundreds of pixels: the clamps."""
import numpy as np

import s16_ends_ref as ends
import s16_ref

PIX_RGB8, PIX_RGB10_U16, PIX_A2B10G10R10, PIX_RGBA8 = 0, 1, 2, 4      # include/rife_hip.h RIFE_HIP_PIX_*
FORMATS = (PIX_RGB8, PIX_RGB10_U16, PIX_A2B10G10R10, PIX_RGBA8)
TAIL_RS, TAIL_HEAD_S16, TAIL_HEAD_F32, TAIL_UNFUSED = 0, 1, 2, 3      # include/rife_hip_test.h RIFE_HIP_TAIL_*
GUARD = 256
C = 64
G = 10                         # the grid of the planted and far cases: 2^-10
CAP = 0.08                     # the boundary set stays below 8 % of the codes of a case; a case over it gets another seed, never a wider cap


def depth_of(pixfmt):
    return 10 if pixfmt in (PIX_RGB10_U16, PIX_A2B10G10R10) else 8


def channels_of(pixfmt):
    return 4 if pixfmt == PIX_RGBA8 else 3


def top_of(depth):
    return 1023 if depth == 10 else 255


def padded(w, h):
    return (w + 31) // 32 * 32, (h + 31) // 32 * 32


# ---- the case table: (kernel, w, h, cus) ------------------------------------------------------------------------------------------------------------------
TAIL_RS_ROWS = [(1, 1, 0), (32, 32, 1), (100, 60, 0), (100, 60, 3), (130, 9, 7), (257, 130, 1), (257, 130, 7), (288, 32, 1), (288, 32, 7)]
TILE_SHAPES = [(1, 1), (100, 60), (130, 9), (257, 130)]      # (257, 130): 5 x 3 = 15 tiles, so the XCD remap of blockIdx.x has a remainder
CASES = [(TAIL_RS, w, h, cus) for w, h, cus in TAIL_RS_ROWS] + [(k, w, h, 0) for k in (TAIL_HEAD_S16, TAIL_HEAD_F32, TAIL_UNFUSED) for w, h in TILE_SHAPES]
DENSE_CASES = [(TAIL_RS, 100, 60, 0), (TAIL_RS, 257, 130, 0), (TAIL_RS, 257, 130, 7), (TAIL_HEAD_S16, 100, 60, 0), (TAIL_HEAD_S16, 257, 130, 0)]
FAR_CASES = [(TAIL_RS, 100, 60, 3), (TAIL_RS, 257, 130, 7), (TAIL_HEAD_S16, 257, 130, 0)]
CHIP_CUS = (256, 304)          # the range assertions hold for whatever CU count a row with cus = 0 meets; asserted for these two


def shapes():
    """every (w, h) a case is built for, by kind"""
    return {"planted": sorted({(w, h) for _, w, h, _ in CASES}), "dense": sorted({(w, h) for _, w, h, _ in DENSE_CASES}),
            "far": sorted({(w, h) for _, w, h, _ in FAR_CASES})}


def tail_rs_ranges(w, h, cus, chip_cus):
    """launch_tail_rs + the prologue of tail_rs_kernel restated: the unit range [u0, u1) of every workgroup (unit = one trunk row of one 32-column strip, strips
    outermost) and what the ranges reach."""
    wp, hp = padded(w, h)
    Hq, Wq = hp // 4, wp // 4
    strips = (Wq + 31) // 32
    nunits = strips * Hq
    nwg = min(2 * (cus if cus > 0 else chip_cus), nunits)
    ranges = [(nunits * wg // nwg, nunits * (wg + 1) // nwg) for wg in range(nwg)]
    steps = [u1 - u0 for u0, u1 in ranges]
    return dict(Hq=Hq, Wq=Wq, strips=strips, nunits=nunits, nwg=nwg, ranges=ranges, smin=min(steps), smax=max(steps),
                strip_changes=sum(1 for u0, u1 in ranges for u in range(u0 + 1, u1) if u % Hq == 0),      # the `fresh` branch of the step loop
                mid_starts=sum(1 for u0, u1 in ranges if u1 > u0 and u0 % Hq != 0),
                last_strip_cols=Wq - 32 * (strips - 1),
                dword_segments=sum(1 for oxb in range(0, w, 64) if w % 4 == 0 and oxb + 64 <= w),           # depth 8, RGB8: the 48-dword store path
                byte_segments=sum(1 for oxb in range(0, w, 64) if not (w % 4 == 0 and oxb + 64 <= w)))


# what the rows of TAIL_RS_ROWS must reach: (w, h, cus) -> conditions on tail_rs_ranges()
RANGE_EXPECT = {
    (1, 1, 0): dict(smin=1, smax=1, strip_changes=0, nwg=8),
    (32, 32, 1): dict(smin=4, smax=4, strip_changes=0, mid_starts=1),
    (100, 60, 0): dict(smin=1, smax=1, strip_changes=0, dword_segments=1, byte_segments=1),
    (100, 60, 3): dict(smin=2, smax=3, strip_changes=0, mid_starts=5, dword_segments=1, byte_segments=1),
    (130, 9, 7): dict(smin=1, smax=2, last_strip_cols=8, dword_segments=0, byte_segments=3),
    (257, 130, 1): dict(smin=60, smax=60, strip_changes=2, mid_starts=1, last_strip_cols=8, dword_segments=0, byte_segments=5),
    (257, 130, 7): dict(smin=8, smax=9, mid_starts=13, last_strip_cols=8),
    (288, 32, 1): dict(smin=12, smax=12, strip_changes=2, mid_starts=1, last_strip_cols=8, dword_segments=4, byte_segments=1),
    (288, 32, 7): dict(smin=1, smax=2, strip_changes=1, last_strip_cols=8),
}


def check_ranges():
    """The range assertions; returns the figures per row for the record."""
    out = {}
    for (w, h, cus) in TAIL_RS_ROWS:
        for chip in CHIP_CUS:
            r = tail_rs_ranges(w, h, cus, chip)
            assert r["ranges"][0][0] == 0 and r["ranges"][-1][1] == r["nunits"] and all(a[1] == b[0] for a, b in zip(r["ranges"], r["ranges"][1:]))
            assert r["smin"] >= 1
            for k, v in RANGE_EXPECT[(w, h, cus)].items():
                assert r[k] == v, ((w, h, cus), chip, k, r[k], v)
            out[(w, h, cus, chip)] = {k: r[k] for k in ("nunits", "nwg", "smin", "smax", "strip_changes", "mid_starts", "last_strip_cols")}
    # between them the rows reach every path of the step loop
    r = {row: tail_rs_ranges(*row, 256) for row in TAIL_RS_ROWS}
    assert any(v["smax"] >= 16 for v in r.values()), "no row walks the 16 steps of the product's regime"
    assert any(v["strip_changes"] > 0 and v["smax"] > 2 for v in r.values()) and any(v["mid_starts"] > 0 for v in r.values())
    assert any(v["smax"] == 1 for v in r.values())
    return out


# ---- the frames ------------------------------------------------------------------------------------------------------------------------------------------
def _tri(t, phase):
    return 1.0 - np.abs(((t + phase) % 16) - 8.0) / 8.0      # a triangle wave of period 16 px and full amplitude


def frame_planes(w, h, depth, which):
    """integer codes (4, hp, wp; depth 10: 3, hp, wp) of resident frame `which` (0, 1): R runs along x, G along y, B along x +- y, the alpha plane (depth 8) along the other diagonal."""
    wp, hp = padded(w, h)
    y, x = np.mgrid[0:hp, 0:wp]
    t = top_of(depth)
    if which == 0:
        p = [_tri(x, 0), _tri(y, 0), _tri(x + y, 0), _tri(x - y, 0)]
    else:
        p = [_tri(x, 10), _tri(y, 11), _tri(x - y, 3), _tri(x + y, 7)]
    return np.rint(np.stack(p if depth == 8 else p[:3]) * t).astype(np.int64)


def pack_resident(planes, depth):
    p = planes.astype(np.uint32)
    if depth == 10:
        return p[0] | (p[1] << 10) | (p[2] << 20)
    return p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24)


def largest_step(planes):
    return int(max(np.abs(np.diff(planes, axis=1)).max(), np.abs(np.diff(planes, axis=2)).max()))


# ---- float64 definitions -----------------------------------------------------------------------------------------------------------------------------------
def warp(img, fx, fy):
    """rife.Warp with the clamp-then-alpha rule: img (n, H, W), flow planes (H, W) -> (values (n, H, W), alpha, beta, outside)."""
    n, H, W = img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    sx, sy = xs + np.asarray(fx, np.float64), ys + np.asarray(fy, np.float64)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)
    y0, y1 = np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
    alpha, beta = sx - x0, sy - y0
    v4 = img[:, y0, x0] * (1 - alpha) + img[:, y0, x1] * alpha
    v5 = img[:, y1, x0] * (1 - alpha) + img[:, y1, x1] * alpha
    outside = (sx < 0) | (sx > W - 1) | (sy < 0) | (sy > H - 1)
    return v4 * (1 - beta) + v5 * beta, alpha, beta, outside


def tail(d, F, M, p0, p1, w, h, depth):
    """d (5, hp, wp) float64 deltas, F (hp, wp, 4), M (hp, wp), p0 / p1 (n, hp, wp) integer codes -> dict(code (h, w, n) int, val (h, w, n) = v top + 0.5
    unquantised, amax (h, w) = max(1, |alpha|, |beta|) over both warps, outside (2, h, w))."""
    t = float(top_of(depth))
    f = np.asarray(F, np.float64) + np.moveaxis(np.asarray(d[:4], np.float64), 0, -1)
    mm = np.asarray(M, np.float64) + d[4]
    m = 1.0 / (1.0 + np.exp(-mm))
    w0, a0, b0, o0 = warp(p0 / t, f[..., 0], f[..., 1])
    w1, a1, b1, o1 = warp(p1 / t, f[..., 2], f[..., 3])
    val = (w0 * m + w1 * (1.0 - m)) * t + 0.5
    amax = np.maximum.reduce([np.ones_like(a0), np.abs(a0), np.abs(b0), np.abs(a1), np.abs(b1)])
    val = np.ascontiguousarray(np.moveaxis(val, 0, -1)[:h, :w])
    return dict(code=np.clip(np.floor(val), 0, t).astype(np.int64), val=val, amax=amax[:h, :w], outside=np.stack([o0, o1])[:, :h, :w])


def reference(x, wgt, b, F, M, p0, p1, w, h, depth):
    """the whole definition from the trunk values x (64, hp / 4, wp / 4)"""
    return tail(ends.head_ps(x, wgt, b)[:5], F, M, p0, p1, w, h, depth)


def boundary(ref, tau):
    """bool (h, w, n): the codes that may differ by one - v top + 0.5 within tau (h, w) of an integer."""
    return np.abs(ref["val"] - np.rint(ref["val"])) <= tau[..., None]


def allowed_range(ref, tau, depth):
    """(lo, hi) codes (h, w, n): what the quantiser may return for a value within tau of the reference's."""
    t = top_of(depth)
    return (np.clip(np.floor(ref["val"] - tau[..., None]), 0, t).astype(np.int64), np.clip(np.floor(ref["val"] + tau[..., None]), 0, t).astype(np.int64))


def pack_frame(code, pixfmt):
    """codes (h, w, >= 3) -> the frame's bytes (flat uint8) in the format's layout"""
    c = np.asarray(code)
    if pixfmt == PIX_RGB8:
        return np.ascontiguousarray(c[..., :3].astype(np.uint8)).reshape(-1)
    if pixfmt == PIX_RGBA8:
        return np.ascontiguousarray(c[..., :4].astype(np.uint8)).reshape(-1)
    if pixfmt == PIX_RGB10_U16:
        return np.ascontiguousarray(c[..., :3].astype("<u2")).reshape(-1).view(np.uint8)
    c = c.astype(np.uint32)
    return np.ascontiguousarray((c[..., 0] | (c[..., 1] << 10) | (c[..., 2] << 20) | np.uint32(3 << 30)).astype("<u4")).reshape(-1).view(np.uint8)


def unpack_frame(buf, w, h, pixfmt):
    """the frame's bytes -> (codes (h, w, n) int64, well_formed): A2B10G10R10 is well formed where the alpha bits are 3; a u16 with high bits set is a code > 1023."""
    b = np.ascontiguousarray(buf, np.uint8).reshape(-1)
    if pixfmt in (PIX_RGB8, PIX_RGBA8):
        return b.reshape(h, w, channels_of(pixfmt)).astype(np.int64), True
    if pixfmt == PIX_RGB10_U16:
        return b.view("<u2").reshape(h, w, 3).astype(np.int64), True
    v = b.view("<u4").reshape(h, w).astype(np.int64)
    return np.stack([v & 1023, (v >> 10) & 1023, (v >> 20) & 1023], axis=-1), bool(np.all((v >> 30) == 3))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------
def _grid(rng, amp, shape):
    return rng.integers(-amp * 2 ** G + 1, amp * 2 ** G, shape) * 2.0 ** -G


def _planted_trunk(w, h, rng):
    wp, hp = padded(w, h)
    Hq, Wq = hp // 4, wp // 4
    hpair = 16.0 + rng.integers(1, 1024, (C // 2, Hq, Wq)) * 2.0 ** -6          # an f16 in (16, 32), never 16 itself: -16 + lo leaves the binade
    hi = np.empty((C, Hq, Wq)); hi[0::2] = hpair; hi[1::2] = -hpair
    lo = rng.integers(1, 8, (C, Hq, Wq)) * 2.0 ** -G                             # below half an f16 step (2^-7) of the binade
    x = (hi + lo).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), hi + lo)
    shi, slo = s16_ref.split(x)
    assert np.array_equal(shi.astype(np.float64), hi) and np.array_equal(slo.astype(np.float64), lo), "the split does not return the planted lo"
    wpair = rng.choice([1.0, 2.0], (24, C // 2, 4, 4)) * np.where(rng.random((24, C // 2, 4, 4)) < 0.8, 1.0, -1.0)
    wgt = np.repeat(wpair, 2, axis=1).astype(np.float32)                         # equal within a pair: the hi products cancel
    b = _grid(rng, 1, 24).astype(np.float32)
    assert not ends.head_ps(hi, wgt, np.zeros(24)).any(), "the hi planes do not cancel"
    bound = ends.head_abs_sum(shi, slo, wgt, b) * 2.0 ** G
    assert bound < 2.0 ** 24, "|partial sums| reach %.3g grid steps (limit 2^24 = 1.7e7)" % bound
    return dict(x=x, hi=hi, lo=lo, wgt=wgt, b=b, bound=bound / 2.0 ** 24)


def _moved(a, b, n):
    return np.abs(a["code"][..., :3] - b["code"][..., :3]) >= n


def _finish(c, w, h, depth, d, tau_extra):
    """the reference, tau and the boundary set of a case; asserts the cap"""
    ref = tail(d, c["F"], c["M"], c["p0"], c["p1"], w, h, depth)
    tau = 2.0 ** -6 * ref["amax"] + tau_extra
    bnd = boundary(ref, tau)
    frac = float(bnd.mean())
    assert frac < CAP, "the boundary set is %.3f of the codes (cap %.2f)" % (frac, CAP)
    c.update(ref=ref, tau=tau, boundary=bnd, boundary_frac=frac, d=d, img0=pack_resident(c["p0"], depth), img1=pack_resident(c["p1"], depth))
    return c


def planted_case(w, h, depth, seed):
    rng = np.random.default_rng([1, w, h, depth, seed])
    wp, hp = padded(w, h)
    c = _planted_trunk(w, h, rng)
    c.update(F=_grid(rng, 3, (hp, wp, 4)).astype(np.float32), M=_grid(rng, 1, (hp, wp)).astype(np.float32),
             p0=frame_planes(w, h, depth, 0), p1=frame_planes(w, h, depth, 1), seed=seed)
    zero = np.zeros(24)
    d_lo = [ends.head_ps(np.where((np.arange(C) // 16 == k)[:, None, None], c["lo"], 0.0), c["wgt"], zero)[:5] for k in range(4)]
    d_b = ends.head_ps(np.zeros_like(c["lo"]), c["wgt"], c["b"])[:5]
    d = d_b + sum(d_lo)
    assert np.array_equal(d, ends.head_ps(c["x"], c["wgt"], c["b"])[:5]) and s16_ref._on_grid(d, G)
    _finish(c, w, h, depth, d, 0.0)
    # power: how far the reference frame moves when lo is dropped from its input
    ref = c["ref"]
    run = lambda dd: tail(dd, c["F"], c["M"], c["p0"], c["p1"], w, h, depth)
    c["lo_part"] = (float(sum(d_lo)[:, :h, :w].mean()), float(sum(d_lo)[:, :h, :w].std()))
    c["power_all"] = float(_moved(run(d_b), ref, 4).mean())
    c["power_chunk"] = [float(_moved(run(d - d_lo[k]), ref, 2).mean()) for k in range(4)]
    c["power_plane"] = []
    for p in range(5):
        dd = d.copy(); dd[p] = d_b[p]
        c["power_plane"].append(float(_moved(run(dd), ref, 2).any(axis=-1).mean()))
    assert c["power_all"] > 0.75, "all lo dropped moves only %.2f of the codes by 4 and more" % c["power_all"]
    assert min(c["power_chunk"]) > 0.5, "a 16-channel chunk of lo dropped moves only %.2f of the codes by 2 and more" % min(c["power_chunk"])
    assert min(c["power_plane"]) > 0.75, "one delta plane's lo dropped moves only %.2f of the pixels by 2 codes and more" % min(c["power_plane"])
    return c


def dense_case(w, h, depth, seed):
    rng = np.random.default_rng([2, w, h, depth, seed])
    wp, hp = padded(w, h)
    g = ends.head_gauss_case(C, hp // 4, wp // 4, rng)
    s = 2.0 ** np.floor(np.log2(3.9 / np.abs(g["want"][:5]).max()))              # a power of two: x and b scale exactly, d with them
    x = ends._through_split((g["x"] * s).astype(np.float32))
    c = dict(x=x, wgt=g["w"], b=(g["b"] * s).astype(np.float32), F=_grid(rng, 3, (hp, wp, 4)).astype(np.float32), M=_grid(rng, 1, (hp, wp)).astype(np.float32),
             p0=frame_planes(w, h, depth, 0), p1=frame_planes(w, h, depth, 1), seed=seed)
    d = ends.head_ps(x, c["wgt"], c["b"])[:5]
    dmax = float(np.abs(d).max())
    assert 1.0 < dmax < 4.0, dmax
    gslope = max(largest_step(c["p0"]), largest_step(c["p1"]), top_of(depth) / 4.0)
    c.update(dmax=dmax, gslope=gslope)
    return _finish(c, w, h, depth, d, gslope * (4e-6 * dmax + 1e-6))


FAR_NEAR, FAR_FAR = 0.28, 0.01     # of the samples of each warp: out of the frame by less than 2 px / by A / 2 .. A px


def far_case(w, h, depth, seed):
    """The planted trunk with flows that leave the padded frame.  tau scales with |alpha|, so a pixel hundreds of pixels out is in the boundary set whatever its
    value: such pixels stay at 1 % per warp and the amplitude A halves until the cap holds."""
    rng = np.random.default_rng([3, w, h, depth, seed])
    wp, hp = padded(w, h)
    c = _planted_trunk(w, h, rng)
    d = ends.head_ps(c["x"], c["wgt"], c["b"])[:5]
    assert s16_ref._on_grid(d, G)
    base = _grid(rng, 3, (hp, wp, 4))
    M = _grid(rng, 1, (hp, wp)).astype(np.float32)
    pick = rng.random((2, hp, wp)); side = rng.integers(0, 4, (2, hp, wp))
    unit = rng.integers(1, 2 ** G, (2, hp, wp)) * 2.0 ** -G                      # (0, 1) on the grid
    ys, xs = np.mgrid[0:hp, 0:wp]
    c.update(M=M, p0=frame_planes(w, h, depth, 0), p1=frame_planes(w, h, depth, 1), seed=seed)
    A = 512
    while True:
        F = base.copy()
        for k in range(2):
            far = pick[k] < FAR_FAR
            out = pick[k] < FAR_FAR + FAR_NEAR
            u = np.where(far, A / 2 + unit[k] * (A / 2), 2 * unit[k])            # how far outside the sample lands
            tx = np.where(side[k] == 0, -u, wp - 1 + u); ty = np.where(side[k] == 2, -u, hp - 1 + u)
            fx = np.where(out & (side[k] < 2), tx - xs - d[2 * k], F[..., 2 * k])
            fy = np.where(out & (side[k] >= 2), ty - ys - d[2 * k + 1], F[..., 2 * k + 1])
            F[..., 2 * k] = fx; F[..., 2 * k + 1] = fy
        assert s16_ref._on_grid(F, G) and np.array_equal(F.astype(np.float32).astype(np.float64), F)
        c["F"] = F.astype(np.float32)
        try:
            _finish(c, w, h, depth, d, 0.0)
            break
        except AssertionError:
            if A <= 4:
                raise
            A //= 2
    c["amplitude"] = A
    c["max_alpha"] = float(c["ref"]["amax"].max())
    c["outside"] = [float(c["ref"]["outside"][k].mean()) for k in range(2)]
    assert min(c["outside"]) > 0.25, "only %.2f of a warp's samples leave the frame" % min(c["outside"])
    assert F.min() < -wp / 2 and F.max() > wp / 2, "the flows do not reach both ends of the frame"
    return c


_BUILDERS = {"planted": planted_case, "dense": dense_case, "far": far_case}
MAX_SEEDS = 512
# where the search below ends, so that it need not be walked again: a frame of ONE pixel has three codes, all of which must move and none of which may sit on a
# rounding boundary.  A hint is only where the search starts - the builder asserts everything for that seed too, and the search goes on from 0 if it fails.
SEED_HINT = {("planted", 1, 1, 8): 372, ("planted", 1, 1, 10): 7}
_CACHE = {}


def cached(kind, w, h, depth):
    """The case of (kind, w, h, depth): the first seed 0, 1, .. whose builder assertions all hold (a case over the cap or under a power threshold gets another
    seed, never a wider bar), computed once per process and shared - do not modify the arrays.  c["tries"] says which seeds failed and why."""
    key = (kind, w, h, depth)
    if key not in _CACHE:
        tries = []
        for seed in ([SEED_HINT[key]] if key in SEED_HINT else []) + list(range(MAX_SEEDS)):
            try:
                c = _BUILDERS[kind](w, h, depth, seed)
            except AssertionError as e:
                tries.append((seed, str(e)))
                continue
            c["tries"] = tries
            _CACHE[key] = c
            break
        else:
            raise AssertionError("no seed below %d gives a %s case at %s: %s" % (MAX_SEEDS, kind, key[1:], tries[-3:]))
    return _CACHE[key]
