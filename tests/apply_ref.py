"""Apply motion (include/rife_hip.h "apply motion") restated in float64 (no GPU): the reference and the case builders of tests/test_gpu_apply.py, on top of
tests/tail_ref.py (its warp, boundary and allowed_range idiom, its cap) and tests/motion_ref.py (the admissible halves).

  S(p, xi, yi) = p[yi][xi] inside w x h, 0 in the virtual padding up to the extent wp x hp
  W(p, dx, dy) = rife.Warp with the clamp-then-alpha rule over the extent (tail_ref.warp on the planes zero-extended to the extent)
  v            = W(p0[k], dx0, dy0) m + W(p1[k], dx1, dy1) (1 - m)
  integer out  = clip(floor(v + 0.5), 0, maxval);  float out = v;  half out = v rounded to nearest even

The sample position sx = x + dx is ONE correctly rounded fp32 add in the definition, so the reference takes it from numpy's float32 add (the same bits) and goes on in
float64: everything after it is what the bars below cover.  F16 motion is widened to float32 first, exactly.

Three kinds of case, each cached per process (do not modify the arrays):
  planted  flows on the 2^-2 grid within a few pixels, masks k / 16, integer-valued samples up to maxval: every fp32 intermediate has at most 16 + 2 + 2 + 4 = 24
           significant bits, so the fp32 result is exact whatever the evaluation order, and the expected output is BYTE FOR BYTE in all four sample types (half: the
           one RNE rounding of the exact v; float planes carry integer values up to 65535, half planes up to 1023).
  far      planted values at maxval <= 1023 with flows that leave the extent by up to 300 pixels: alpha extrapolates, both clamped taps are the same sample, the
           products stay below 2^19 on the 2^-2 grid and the two terms sum back to the sample exactly.
  dense    smooth random flows of a few pixels and a smooth mask in (0, 1), not on a grid; random samples.

Bars of the dense cases - derived, not measured.  u = 2^-24 is the unit roundoff of fp32, A = amax = max(1, |alpha|, |beta|) over both warps, S = the largest
sample magnitude in the two footprints.  Worst case through the path (|1 - alpha| <= 2 A, so a row lerp is bounded by 3 A S and the column lerp by 9 A^2 S):
  alpha (rounded only where the tap was clamped) u A; 1 - alpha 3 u A; the row lerp's two products and sum 10 u A S; the column lerp 60 u A^2 S; 1 - m one more u;
  the two blend products and their sum 87 u A^2 S; the quantiser's v + 0.5 another 9.5 u A^2 S (integer samples: S >= 1 wherever v != 0).
That is under c = 100 rounded-operation units:      tau = 100 * 2^-24 * amax^2 * S.
  integer out  equals floor(v64 + 0.5) outside the boundary set |frac(v64 + 0.5) - nearest integer| <= tau, and lies in the allowed range inside it;
  float out    within tau;
  half out     the RNE half of some value within tau (motion_ref.mask_half_ok).
The boundary set of a dense integer case stays under tail_ref.CAP (8 %); a case over it gets another seed, never a wider cap.  Dense integer cases are u8 / 255,
u16 / 1023 and u16 / 4095 (tau = 0.024 code at A = 1: 4.9 % of the codes); u16 / 65535 (tau = 0.39 code) gets planted cases plus one dense case judged by
|got - v64| <= 0.5 + tau alone, which claims no equality and needs no cap."""
import numpy as np

import motion_ref as mr
import tail_ref as tr

SAMPLE_U8, SAMPLE_U16, SAMPLE_F16, SAMPLE_F32 = 0, 1, 2, 3      # include/rife_hip.h RIFE_HIP_SAMPLE_*
DTYPE = {SAMPLE_U8: np.uint8, SAMPLE_U16: np.uint16, SAMPLE_F16: np.float16, SAMPLE_F32: np.float32}
C_OPS = 100.0
U = 2.0 ** -24
CAP = tr.CAP
# (sample, maxval) of the dense cases that claim equality, and the one that does not
DENSE_KINDS = [(SAMPLE_U8, 255), (SAMPLE_U16, 1023), (SAMPLE_U16, 4095), (SAMPLE_F16, 0), (SAMPLE_F32, 0)]
DENSE_WIDE = (SAMPLE_U16, 65535)
SIZES = [(1, 1), (33, 47), (100, 60), (257, 130)]


def padded(w, h, pad=32):
    return (w + pad - 1) // pad * pad, (h + pad - 1) // pad * pad


def is_int(sample):
    return sample in (SAMPLE_U8, SAMPLE_U16)


def _extend(a, hp, wp):
    out = np.zeros(a.shape[:-2] + (hp, wp), np.float64)
    out[..., :a.shape[-2], :a.shape[-1]] = a
    return out


def _footprint_max(img, fx, fy):
    """largest |sample| among the four clamped taps of each pixel: (H, W)"""
    n, H, W = img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    sx, sy = xs + fx, ys + fy
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    a = np.abs(img)
    return np.maximum.reduce([a[:, y0, x0], a[:, y0, x1], a[:, y1, x0], a[:, y1, x1]]).max(axis=0)


def apply64(p0, p1, flow, mask, extent=None):
    """p0, p1 (n, h, w) samples, flow (h, w, 4) float32 / float16, mask (h, w) -> dict(v (n, h, w) float64, amax (h, w), S (h, w), tau (h, w))."""
    p0 = np.asarray(p0); p1 = np.asarray(p1)
    n, h, w = p0.shape
    wp, hp = extent if extent else (w, h)
    assert wp >= w and hp >= h
    f32 = np.asarray(flow).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    # sx = x + dx as the definition's ONE fp32 add; handed to tail_ref.warp as the flow that reproduces it exactly in float64
    fx = [np.zeros((hp, wp)) for _ in range(4)]
    for k in range(4):
        base = (xs if k % 2 == 0 else ys)
        s32 = base.astype(np.float32) + f32[..., k]
        assert s32.dtype == np.float32
        fx[k][:h, :w] = s32.astype(np.float64) - base
    m = np.zeros((hp, wp)); m[:h, :w] = np.asarray(mask).astype(np.float32).astype(np.float64)
    e0, e1 = _extend(p0.astype(np.float64), hp, wp), _extend(p1.astype(np.float64), hp, wp)
    w0, a0, b0, _ = tr.warp(e0, fx[0], fx[1])
    w1, a1, b1, _ = tr.warp(e1, fx[2], fx[3])
    v = w0 * m + w1 * (1.0 - m)
    amax = np.maximum.reduce([np.ones_like(a0), np.abs(a0), np.abs(b0), np.abs(a1), np.abs(b1)])
    S = np.maximum(_footprint_max(e0, fx[0], fx[1]), _footprint_max(e1, fx[2], fx[3]))
    tau = C_OPS * U * amax * amax * S
    return dict(v=np.ascontiguousarray(v[:, :h, :w]), amax=amax[:h, :w], S=S[:h, :w], tau=tau[:h, :w])


def expected_exact(ref, sample, maxval):
    """the output of a planted / far case, bit for bit"""
    v = ref["v"]
    if is_int(sample):
        return np.clip(np.floor(v + 0.5), 0, maxval).astype(DTYPE[sample])
    return v.astype(DTYPE[sample])      # float64 -> half / float directly: one rounding to nearest even (float: exact)


def boundary(ref):
    val = ref["v"] + 0.5
    return np.abs(val - np.rint(val)) <= ref["tau"][None]


def holds(got, ref, sample, maxval, equality=True):
    """(ok, figures): `got` (n, h, w) against the reference under the bars of this module's docstring."""
    v, tau = ref["v"], ref["tau"][None]
    g = np.asarray(got)
    if is_int(sample):
        g = g.astype(np.int64)
        if not equality:
            err = np.abs(g - np.clip(v, -0.5, maxval + 0.5))
            return bool(np.all(err <= 0.5 + tau)), dict(max_err=float(err.max()))
        bnd = boundary(ref)
        want = np.clip(np.floor(v + 0.5), 0, maxval).astype(np.int64)
        lo = np.clip(np.floor(v + 0.5 - tau), 0, maxval).astype(np.int64); hi = np.clip(np.floor(v + 0.5 + tau), 0, maxval).astype(np.int64)
        ok = np.array_equal(g[~bnd], want[~bnd]) and bool(np.all((g >= lo) & (g <= hi)))
        return ok, dict(boundary=float(bnd.mean()), differ=int((g != want).sum()))
    if sample == SAMPLE_F32:
        err = np.abs(g.astype(np.float64) - v)
        return bool(np.all(err <= tau)), dict(max_err=float(err.max()), max_tau=float(tau.max()))
    ok = mr.mask_half_ok(g, v, tau)
    return bool(ok.all()), dict(not_admissible=int((~ok).sum()))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
def _top(sample, maxval):
    return maxval if is_int(sample) else (1023 if sample == SAMPLE_F16 else 65535)


def _planes(rng, n, h, w, sample, maxval, integer_valued):
    top = _top(sample, maxval)
    if is_int(sample) or integer_valued:
        return rng.integers(0, top + 1, (2, n, h, w)).astype(DTYPE[sample])
    return rng.random((2, n, h, w)).astype(DTYPE[sample])      # nominal range [0, 1)


def _grid_motion(rng, h, w):
    flow = (rng.integers(-12, 13, (h, w, 4)) * 0.25).astype(np.float32)      # 2^-2 grid, |d| <= 3 px
    mask = (rng.integers(0, 17, (h, w)) / 16.0).astype(np.float32)           # k / 16, 0 and 1 included
    return flow, mask


def planted_case(w, h, n, sample, maxval, seed=0):
    rng = np.random.default_rng([11, w, h, n, sample, maxval, seed])
    p = _planes(rng, n, h, w, sample, maxval, True)
    flow, mask = _grid_motion(rng, h, w)
    return dict(p0=p[0], p1=p[1], flow=flow, mask=mask, sample=sample, maxval=maxval, kind="planted")


FAR_A = 300


def far_case(w, h, n, sample, maxval, extent, seed=0):
    """planted values (at most 1023) with 30 % of each warp's samples pushed out of the extent, a tenth of those by up to FAR_A pixels"""
    rng = np.random.default_rng([12, w, h, n, sample, maxval, seed])
    top = min(_top(sample, maxval), 1023)
    p = rng.integers(0, top + 1, (2, n, h, w)).astype(DTYPE[sample])
    flow, mask = _grid_motion(rng, h, w)
    wp, hp = extent
    ys, xs = np.mgrid[0:h, 0:w]
    for k in range(2):
        pick = rng.random((h, w)); side = rng.integers(0, 4, (h, w))
        u = np.where(pick < 0.03, rng.integers(8, 4 * FAR_A + 1, (h, w)), rng.integers(1, 9, (h, w))) * 0.25      # how far outside the sample lands
        out = pick < 0.30
        tx = np.where(side == 0, -u, wp - 1 + u); ty = np.where(side == 2, -u, hp - 1 + u)
        flow[..., 2 * k] = np.where(out & (side < 2), tx - xs, flow[..., 2 * k])
        flow[..., 2 * k + 1] = np.where(out & (side >= 2), ty - ys, flow[..., 2 * k + 1])
    assert np.array_equal(flow * 4, np.rint(flow * 4))
    return dict(p0=p[0], p1=p[1], flow=flow, mask=mask, sample=sample, maxval=maxval, kind="far")


def _smooth(rng, h, w, amp):
    """low-resolution noise, bilinearly upsampled: smooth, and on no grid"""
    gh, gw = h // 16 + 3, w // 16 + 3
    g = rng.standard_normal((gh, gw))
    yy = np.linspace(0, gh - 1.001, h)[:, None]; xx = np.linspace(0, gw - 1.001, w)[None, :]
    y0, x0 = np.floor(yy).astype(int), np.floor(xx).astype(int)
    fy, fx = yy - y0, xx - x0
    v = (g[y0, x0] * (1 - fx) + g[y0, x0 + 1] * fx) * (1 - fy) + (g[y0 + 1, x0] * (1 - fx) + g[y0 + 1, x0 + 1] * fx) * fy
    return amp * v / max(np.abs(v).max(), 1e-9)


def dense_case(w, h, n, sample, maxval, seed=0):
    rng = np.random.default_rng([13, w, h, n, sample, maxval, seed])
    p = _planes(rng, n, h, w, sample, maxval, False)
    flow = np.stack([_smooth(rng, h, w, 3.7) + rng.random((h, w)) * 1e-3 for _ in range(4)], axis=-1).astype(np.float32)
    mask = (0.5 + 0.45 * _smooth(rng, h, w, 1.0)).astype(np.float32)
    return dict(p0=p[0], p1=p[1], flow=flow, mask=mask, sample=sample, maxval=maxval, kind="dense")


_CACHE = {}
MAX_SEEDS = 64


def cached(kind, w, h, n, sample, maxval, extent=None, half_motion=False):
    """The case and its reference for (kind, w, h, n, sample, maxval, extent, motion format): computed once per process and shared - do not modify the arrays.
    half_motion: flow and mask are rounded to float16 FIRST and the reference is that of the rounded motion (F16 motion is widened exactly, so the bars are
    unchanged; a grid value a half cannot hold moves to a coarser grid, never off it).  A dense integer case whose boundary set exceeds the cap gets the next seed
    (c["seed"] says which one holds)."""
    ext = tuple(extent) if extent else (w, h)
    key = (kind, w, h, n, sample, maxval, ext, bool(half_motion))
    if key in _CACHE:
        return _CACHE[key]
    for seed in range(MAX_SEEDS):
        c = planted_case(w, h, n, sample, maxval, seed) if kind == "planted" else far_case(w, h, n, sample, maxval, ext, seed) if kind == "far" \
            else dense_case(w, h, n, sample, maxval, seed)
        if half_motion:
            c["flow"] = c["flow"].astype(np.float16); c["mask"] = c["mask"].astype(np.float16)
        c["ref"] = apply64(c["p0"], c["p1"], c["flow"], c["mask"], ext)
        c["extent"] = ext; c["seed"] = seed
        if kind == "dense" and is_int(sample) and (sample, maxval) != DENSE_WIDE:
            c["boundary_frac"] = float(boundary(c["ref"]).mean())
            if c["boundary_frac"] >= CAP:
                continue
        _CACHE[key] = c
        return c
    raise AssertionError("no seed below %d gives a dense case under the cap at %s" % (MAX_SEEDS, key))


def exact_in_float32(c):
    """The planted / far claim, in float32 numpy with the kernel's operation order: every intermediate equals its float64 value."""
    p0 = c["p0"].astype(np.float32); p1 = c["p1"].astype(np.float32)
    n, h, w = p0.shape
    wp, hp = c["extent"]
    f = c["flow"].astype(np.float32); m = c["mask"].astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    one = np.float32(1)

    def W(p, dx, dy):
        sx = xs.astype(np.float32) + dx; sy = ys.astype(np.float32) + dy
        x0 = np.floor(sx).astype(np.int64); y0 = np.floor(sy).astype(np.int64)
        x1, y1 = np.clip(x0 + 1, 0, wp - 1), np.clip(y0 + 1, 0, hp - 1)
        x0, y0 = np.clip(x0, 0, wp - 1), np.clip(y0, 0, hp - 1)
        a = sx - x0.astype(np.float32); b = sy - y0.astype(np.float32)
        e = np.zeros((n, hp, wp), np.float32); e[:, :h, :w] = p
        r0 = e[:, y0, x0] * (one - a) + e[:, y0, x1] * a
        r1 = e[:, y1, x0] * (one - a) + e[:, y1, x1] * a
        return r0 * (one - b) + r1 * b
    v = W(p0, f[..., 0], f[..., 1]) * m + W(p1, f[..., 2], f[..., 3]) * (one - m)
    assert v.dtype == np.float32
    return np.array_equal(v.astype(np.float64), c["ref"]["v"])
