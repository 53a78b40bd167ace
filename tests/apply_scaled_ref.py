"""Apply motion at another resolution (include/rife_hip.h rife_hip_apply_set_t) restated for the tests (no GPU): the RESAMPLED motion in numpy float32 with exactly
the header's operation order, and the case builders of tests/test_gpu_apply_scaled.py.  The result of a set is the apply definition, unchanged, on the resampled
motion, so everything after resample() is tests/apply_ref.py: apply64, holds, boundary, expected_exact, exact_in_float32, the cap and the bars derived there - nothing
new is measured or bounded here.

resample() is exact, not approximate: every step of the definition is ONE correctly rounded fp32 operation (a sum, or a product by 0.25, 0.5, 0.75 or 2), numpy's
float32 arithmetic rounds each of them the same way, and no step is fused.  F16 motion is widened first, exactly.

Case kinds on a motion of mw x mh with planes of ws x hs (cached per process; do not modify the arrays):
  planted  integer-valued samples of at most 1023; down shifts: flows on the 2^-2 grid with |d| <= 3 and masks k / 4 - the box sum of four puts the resampled flow on
           the 2^-5 grid and the mask on k / 16, 10 + 5 + 5 + 4 = 24 significant bits at most; up shift: flows on the 2^-1 grid and masks 0 or 1 - two lerps with
           weights k / 4 and the doubling put the flow on the 2^-4 grid and the mask on k / 16, 10 + 4 + 4 + 4 = 22 bits.  Resampled motion and fp32 apply are then
           exact whatever the evaluation order (tests/test_apply_scaled_host.py checks both with apply_ref.exact_in_float32), and the output is BYTE FOR BYTE
           apply_ref.expected_exact in all four sample types.
  dense    apply_ref's smooth fields on the motion grid, the flow amplitude doubled for the down shifts so that the resampled flow still exceeds 2 px; random
           samples.  Judged by apply_ref.holds on the resampled motion.  A dense integer case that claims equality (apply_ref.DENSE_KINDS[:3]) whose boundary set
           exceeds apply_ref.CAP gets the next seed, never a wider cap; below 33 x 47 one boundary sample of a 3 x 3 plane is 11 %, so the tiny sizes get planted
           cases only.  The strips (planes of 2 to 4 rows) cannot meet the cap either - a flow of a few pixels leaves a 3-row extent almost everywhere, beta
           extrapolates and tau grows with its square - so a strip gets planted cases in all four sample types, dense cases in the float types
           (DENSE_STRIP_KINDS), whose bar is a distance and claims no equality, and dense cases in the integer types for the launch-against-launch identity
           alone (cached(capped=False)), which needs no cap."""
import numpy as np

import apply_ref as ar

SHIFT_420, SHIFT_422, SHIFT_UP = (-1, -1), (-1, 0), (1, 1)
SHIFTS = [SHIFT_420, SHIFT_422, SHIFT_UP]
SHIFT_ID = {SHIFT_420: "420", SHIFT_422: "422", SHIFT_UP: "up", (0, 0): "same"}
TINY = [(1, 1), (2, 2), (3, 3)]                      # planted only
SIZES = [(33, 47), (100, 60), (257, 130)]            # planted and dense
DENSE_STRIP_KINDS = ar.DENSE_KINDS[3:]                 # half and float
STRIP = {SHIFT_420: (2050, 3), SHIFT_422: (2050, 3), SHIFT_UP: (513, 2)}      # runs per plane row exceed 256: a second workgroup across


def plane_sizes(shift, mw, mh):
    """the plane sizes (ws, hs) a shift admits on a motion of mw x mh: one, or for the up shift 2 m and 2 m - 1 on both axes"""
    if shift == (0, 0):
        return [(mw, mh)]
    if shift == SHIFT_420:
        return [((mw + 1) // 2, (mh + 1) // 2)]
    if shift == SHIFT_422:
        return [((mw + 1) // 2, mh)]
    return [(2 * mw, 2 * mh), (2 * mw - 1, 2 * mh - 1)]


def frame_extent(shift, mw, mh, pad=32):
    """frame semantics in plane pixels: (wp / 2, hp / 2) of the motion's padded size on chroma (4:2:2: hp), (2 wp, 2 hp) of the proxy's for the up shift"""
    wp, hp = ar.padded(mw, mh, pad)
    fx = {0: lambda v: v, -1: lambda v: v // 2, 1: lambda v: 2 * v}
    return fx[shift[0]](wp), fx[shift[1]](hp)


def extents(shift, mw, mh, ws, hs):
    """0, 0 (the plane size), the frame extent, a 64-padded extent"""
    return [(ws, hs), frame_extent(shift, mw, mh), ar.padded(ws, hs, 64)]


def resample(flow, mask, shift, ws, hs):
    """flow (mh, mw, 4), mask (mh, mw), float32 or float16 -> (flow' (hs, ws, 4), mask' (hs, ws)) float32: the header's definition, operation by operation."""
    f = np.asarray(flow).astype(np.float32); m = np.asarray(mask).astype(np.float32)
    mh, mw = m.shape
    fits = {0: lambda v, n: v == n, -1: lambda v, n: v == (n + 1) // 2, 1: lambda v, n: v in (2 * n - 1, 2 * n)}
    assert f.shape == (mh, mw, 4) and fits[shift[0]](ws, mw) and fits[shift[1]](hs, mh)
    if tuple(shift) == (0, 0):
        return f, m
    M = np.concatenate([f, m[..., None]], axis=-1)      # dx0, dy0, dx1, dy1, m
    q, hf, tq, two = np.float32(0.25), np.float32(0.5), np.float32(0.75), np.float32(2)
    xs, ys = np.arange(ws), np.arange(hs)
    if shift[0] == -1:
        c0, c1 = 2 * xs, np.minimum(2 * xs + 1, mw - 1)
        if shift[1] == -1:
            r0, r1 = 2 * ys, np.minimum(2 * ys + 1, mh - 1)
            s = ((M[r0][:, c0] + M[r0][:, c1]) + (M[r1][:, c0] + M[r1][:, c1])) * q
            scaled = (0, 1, 2, 3)
        else:
            s = (M[:, c0] + M[:, c1]) * hf
            scaled = (0, 2)
        k = hf
    else:
        j = xs >> 1; jn = np.where(xs & 1, np.minimum(j + 1, mw - 1), np.maximum(j - 1, 0))
        i = ys >> 1; inn = np.where(ys & 1, np.minimum(i + 1, mh - 1), np.maximum(i - 1, 0))
        H = M[:, j] * tq + M[:, jn] * q
        s = H[i] * tq + H[inn] * q
        scaled, k = (0, 1, 2, 3), two
    assert s.dtype == np.float32 and s.shape == (hs, ws, 5)
    out = s.copy()
    for ch in scaled:
        out[..., ch] = s[..., ch] * k
    assert out.dtype == np.float32
    return out[..., :4].copy(), out[..., 4].copy()      # copies: a 1 x 1 slice passes for contiguous with the strides of the five-component array


def resample64(flow, mask, shift, ws, hs):
    """the same in float64, from the float32 (or widened float16) motion: what the planted cases must reproduce exactly"""
    f = np.asarray(flow).astype(np.float32).astype(np.float64); m = np.asarray(mask).astype(np.float32).astype(np.float64)
    mh, mw = m.shape
    M = np.concatenate([f, m[..., None]], axis=-1)
    xs, ys = np.arange(ws), np.arange(hs)
    if shift[0] == -1:
        c0, c1 = 2 * xs, np.minimum(2 * xs + 1, mw - 1)
        if shift[1] == -1:
            r0, r1 = 2 * ys, np.minimum(2 * ys + 1, mh - 1)
            s = (M[r0][:, c0] + M[r0][:, c1] + M[r1][:, c0] + M[r1][:, c1]) / 4
            s[..., :4] /= 2
        else:
            s = (M[:, c0] + M[:, c1]) / 2
            s[..., (0, 2)] /= 2
    else:
        j = xs >> 1; jn = np.where(xs & 1, np.minimum(j + 1, mw - 1), np.maximum(j - 1, 0))
        i = ys >> 1; inn = np.where(ys & 1, np.minimum(i + 1, mh - 1), np.maximum(i - 1, 0))
        H = M[:, j] * 0.75 + M[:, jn] * 0.25
        s = H[i] * 0.75 + H[inn] * 0.25
        s[..., :4] *= 2
    return s[..., :4], s[..., 4]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
def _planted_motion(rng, shift, mh, mw):
    if shift[0] < 0:
        flow = (rng.integers(-12, 13, (mh, mw, 4)) * 0.25).astype(np.float32)      # 2^-2 grid, |d| <= 3 px
        mask = (rng.integers(0, 5, (mh, mw)) / 4.0).astype(np.float32)             # k / 4, 0 and 1 included
    else:
        flow = (rng.integers(-6, 7, (mh, mw, 4)) * 0.5).astype(np.float32)         # 2^-1 grid, |d| <= 3 px
        mask = rng.integers(0, 2, (mh, mw)).astype(np.float32)                     # 0 or 1
    return flow, mask


def planted_case(shift, mw, mh, ws, hs, n, sample, maxval, seed=0):
    rng = np.random.default_rng([21, shift[0] + 1, shift[1] + 1, mw, mh, ws, n, sample, maxval, seed])
    top = min(ar._top(sample, maxval), 1023)
    p = rng.integers(0, top + 1, (2, n, hs, ws)).astype(ar.DTYPE[sample])
    flow, mask = _planted_motion(rng, shift, mh, mw)
    return dict(p0=p[0], p1=p[1], mflow=flow, mmask=mask, sample=sample, maxval=maxval, kind="planted")


def dense_case(shift, mw, mh, ws, hs, n, sample, maxval, seed=0):
    rng = np.random.default_rng([23, shift[0] + 1, shift[1] + 1, mw, mh, ws, n, sample, maxval, seed])
    p = ar._planes(rng, n, hs, ws, sample, maxval, False)
    amp = 7.4 if shift[0] < 0 else 3.7
    flow = np.stack([ar._smooth(rng, mh, mw, amp) + rng.random((mh, mw)) * 1e-3 for _ in range(4)], axis=-1).astype(np.float32)
    mask = (0.5 + 0.45 * ar._smooth(rng, mh, mw, 1.0)).astype(np.float32)
    return dict(p0=p[0], p1=p[1], mflow=flow, mmask=mask, sample=sample, maxval=maxval, kind="dense")


_CACHE = {}


def cached(kind, shift, mw, mh, ws, hs, n, sample, maxval, extent=None, half_motion=False, capped=True):
    """The case and its reference: p0, p1 (n, hs, ws); mflow, mmask the motion of mw x mh (float16 when half_motion: rounded FIRST, the reference is that of the
    rounded motion); flow, mask its resample() (float32, ws x hs); ref = apply_ref.apply64 on the resampled motion with `extent`.  Computed once per process and
    shared - do not modify the arrays.  The seed search is apply_ref.cached's: a dense integer case that claims equality and exceeds the cap gets the next seed.
    capped=False: seed 0 as it comes, for a test that compares two launches with each other and claims nothing against the reference."""
    shift = tuple(shift)
    ext = tuple(extent) if extent else (ws, hs)
    key = (kind, shift, mw, mh, ws, hs, n, sample, maxval, ext, bool(half_motion), bool(capped))
    if key in _CACHE:
        return _CACHE[key]
    for seed in range(ar.MAX_SEEDS):
        c = (planted_case if kind == "planted" else dense_case)(shift, mw, mh, ws, hs, n, sample, maxval, seed)
        if half_motion:
            c["mflow"] = c["mflow"].astype(np.float16); c["mmask"] = c["mmask"].astype(np.float16)
        c["flow"], c["mask"] = resample(c["mflow"], c["mmask"], shift, ws, hs)
        c["ref"] = ar.apply64(c["p0"], c["p1"], c["flow"], c["mask"], ext)
        c["extent"] = ext; c["seed"] = seed; c["shift"] = shift
        if capped and kind == "dense" and ar.is_int(sample) and (sample, maxval) != ar.DENSE_WIDE:
            c["boundary_frac"] = float(ar.boundary(c["ref"]).mean())
            if c["boundary_frac"] >= ar.CAP:
                continue
        _CACHE[key] = c
        return c
    raise AssertionError("no seed below %d gives a dense case under the cap at %s" % (ar.MAX_SEEDS, key))
