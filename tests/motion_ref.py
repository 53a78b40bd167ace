"""The motion export of rife-v4.6 restated in float64 (no GPU): what the kernels that finish a frame also store (include/rife_hip.h "motion export"), built on
tests/tail_ref.py - its tail(), warp, boundary and allowed_range, its case table.

  flow = F + d[:4]                   the graph's final flow (blob 327): pixel (x, y) was sampled from frame 0 at (x + flow[0], y + flow[1]), from frame 1 at
                                     (x + flow[2], y + flow[3])
  mask = 1 / (1 + exp(-(M + d[4])))  the Sigmoid output (blob 332): the weight of frame 0's warp
both cropped to w x h.  Half samples are the float32 sample rounded to nearest even: numpy's float16 cast.

Bars of the single-launch tests (tests/test_gpu_motion.py), derived, not measured:
  flow, planted and far cases   byte for byte.  F and d are on the 2^-10 grid and small, so F + d is exact in fp32 and in float64: the F32 bits are the float64
                                value's, and the F16 sample is the RNE half of them.
  flow, dense cases             4e-6 max|d| + 1e-6 px: the bar tail_ref states for deltas that are not exact (the head's dense bar).
  mask, F32                     2^-20 of the float64 value: expf to 2 ulp, an add and a divide give under 4e-7; 2^-20 is 2.6 times that.
  mask, F16                     the RNE half of SOME value within 2^-20 of the reference: at most two admissible halves per sample.

reconstruct() rebuilds the frame values from exported motion and the input codes, so a frame can be held against the motion that came with it."""
import numpy as np

import tail_ref as tr

MOTION_F32, MOTION_F16 = 0, 1      # include/rife_hip.h RIFE_HIP_MOTION_*
DTYPE = {MOTION_F32: np.float32, MOTION_F16: np.float16}
MASK_TOL = 2.0 ** -20
DENSE_FLOW_TOL = lambda dmax: 4e-6 * dmax + 1e-6


def expected(case, w, h):
    """(flow (h, w, 4), mask (h, w)) in float64 of a tail_ref case (its d, F, M)."""
    d = np.asarray(case["d"], np.float64)
    flow = np.asarray(case["F"], np.float64) + np.moveaxis(d[:4], 0, -1)
    mask = 1.0 / (1.0 + np.exp(-(np.asarray(case["M"], np.float64) + d[4])))
    return np.ascontiguousarray(flow[:h, :w]), np.ascontiguousarray(mask[:h, :w])


def half(a):
    """round to nearest even, as the kernels' conversion"""
    return np.asarray(a, np.float32).astype(np.float16)


def mask_half_ok(got_half, want64, tol=MASK_TOL):
    """bool array: got is the RNE half of some value in [want - tol, want + tol].  Rounding is monotone, so that is half(want - tol) <= got <= half(want + tol)."""
    g = np.asarray(got_half, np.float16).astype(np.float64)
    lo = np.asarray(want64 - tol, np.float64).astype(np.float16).astype(np.float64)      # float64 -> float16 directly: one rounding, to nearest even
    hi = np.asarray(want64 + tol, np.float64).astype(np.float16).astype(np.float64)
    return (g >= lo) & (g <= hi)


def reconstruct(flow, mask, p0, p1, depth):
    """flow (h, w, 4), mask (h, w) as exported; p0 / p1 (n, hp, wp) integer codes of the padded resident frames -> (val (h, w, n) = v top + 0.5 unquantised, amax (h, w)):
    tail_ref.tail() from the final flow and mask on, with the frame's own clamp-then-alpha warps over the PADDED frames."""
    h, w = mask.shape
    n, hp, wp = p0.shape
    t = float(tr.top_of(depth))
    f = np.zeros((hp, wp, 4)); f[:h, :w] = np.asarray(flow, np.float64)
    m = np.zeros((hp, wp)); m[:h, :w] = np.asarray(mask, np.float64)
    w0, a0, b0, _ = tr.warp(p0 / t, f[..., 0], f[..., 1])
    w1, a1, b1, _ = tr.warp(p1 / t, f[..., 2], f[..., 3])
    val = (w0 * m + w1 * (1.0 - m)) * t + 0.5
    amax = np.maximum.reduce([np.ones_like(a0), np.abs(a0), np.abs(b0), np.abs(a1), np.abs(b1)])
    return np.ascontiguousarray(np.moveaxis(val, 0, -1)[:h, :w]), amax[:h, :w]


def frame_matches(codes, val, amax, depth, extra_tau=0.0):
    """(ok, boundary_fraction): the quantised codes (h, w, n) against rebuilt values - equal outside the boundary set tau = 2^-6 amax (+ extra_tau), within the
    allowed range inside it."""
    ref = dict(val=val)
    tau = 2.0 ** -6 * amax + extra_tau
    bnd = tr.boundary(ref, tau)
    t = tr.top_of(depth)
    want = np.clip(np.floor(val), 0, t).astype(np.int64)
    lo, hi = tr.allowed_range(ref, tau, depth)
    c = np.asarray(codes, np.int64)
    ok = np.array_equal(c[~bnd], want[~bnd]) and bool(np.all((c >= lo) & (c <= hi)))
    return ok, float(bnd.mean())


def resident_planes(frame, depth, pad=32):
    """A frame at the C boundary -> the integer code planes (3, hp, wp) of the zero-padded resident frame: (h, w, 3) uint8 (depth 8) or (h, w, 3) uint16 codes (depth 10)."""
    a = np.asarray(frame)
    h, w = a.shape[:2]
    hp, wp = (h + pad - 1) // pad * pad, (w + pad - 1) // pad * pad
    p = np.zeros((3, hp, wp), np.int64)
    p[:, :h, :w] = np.moveaxis(np.minimum(a[..., :3].astype(np.int64), tr.top_of(depth)), -1, 0)
    return p


# ---- end to end: the inputs of tests/test_gpu_motion.py and the oracle's blobs for them (CPU; computed once per process and shared - do not modify) --------------
# name -> (frame generator of tools/gen_frames.py, w, h, flow scale, seed).  "rs": a frame on which the test build forces the row-streaming tail.  A case whose
# boundary set exceeds tail_ref.CAP gets another seed here, never a wider cap (tests/test_motion_host.py checks every one against the oracle alone).
E2E = {"smooth": ("smooth", 96, 64, 1, 77), "noise": ("noise", 96, 64, 1, 7), "ragged": ("smooth", 100, 60, 1, 78), "rs": ("smooth", 257, 130, 1, 79),
       "scale2": ("smooth", 64, 48, 2, 80)}
E2E_FLOW_TOL = 1e-3      # px: the project's bound for stage flows (tests/test_gpu_v4.py)
E2E_MASK_TOL = 1e-3      # the sigmoid's slope is at most 1/4 of the same logit error
_E2E_CACHE = {}


def e2e_pair(name):
    from tools import gen_frames
    kind, w, h, _, seed = E2E[name]
    a, b = (gen_frames.smooth_pair if kind == "smooth" else gen_frames.noise_pair)(w, h, seed)
    return np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)


def oracle_motion(name, modeldir, tmpdir):
    """dict(flow (h, w, 4) float32, mask (h, w) float32, frame (h, w, 3) uint8 = the oracle's quantised out0, a, b, pad) of input `name` at timestep 0.5: the blobs the
    last two rife.Warp layers and the last Sigmoid name in the graph the oracle runs (the stock one, or the one rewritten for flow scale 2)."""
    if name in _E2E_CACHE:
        return _E2E_CACHE[name]
    import os

    import deep_ref
    import flowscale_ref
    from oracle import pyoracle
    _, w, h, scale, _ = E2E[name]
    a, b = e2e_pair(name)
    d = modeldir if scale == 1 else flowscale_ref.scaled_modeldir(modeldir, os.path.join(os.fspath(tmpdir), "motion_scale2"))
    flow_blob, mask_blob = motion_blobs(open(os.path.join(d, "flownet.param")).read())
    o = pyoracle.OracleRIFE(rife_v4=True)
    o.load(d)
    ex = (lambda blob: deep_ref.extract(o, a, b, 0.5, 8, blob)) if scale == 1 else (lambda blob: flowscale_ref.extract(o, a, b, 0.5, 8, blob))
    f, m, out0 = ex(flow_blob), ex(mask_blob), ex("out0")
    assert f.shape[0] == 4 and m.shape[0] == 1
    r = dict(flow=np.ascontiguousarray(np.moveaxis(f, 0, -1)[:h, :w]), mask=np.ascontiguousarray(m[0, :h, :w]), frame=deep_ref.quantise(out0, w, h, 8), a=a, b=b,
             pad=32 * scale, blobs=(flow_blob, mask_blob))
    _E2E_CACHE[name] = r
    return r


def rebuilt(name_or_pair, flow, mask, pad):
    """reconstruct() on the 8-bit input frames of an end-to-end case: (val, amax)."""
    a, b = name_or_pair
    return reconstruct(flow, mask, resident_planes(a, 8, pad), resident_planes(b, 8, pad), 8)


# ---- the graph's blobs, found structurally in the .param text (so the same code serves the graph rewritten by tests/flowscale_ref.py) -----------------------
def motion_blobs(param_text):
    """(flow_blob, mask_blob): the 4-channel blob both of the last two rife.Warp layers take their flow from (each through a Split copy and a Crop of two
    channels), and the output of the last Sigmoid."""
    producer, warps, sig = {}, [], None
    for line in param_text.splitlines():
        t = line.split()
        if len(t) < 4 or not t[2].isdigit() or not t[3].isdigit():
            continue
        nin, nout = int(t[2]), int(t[3])
        ins, outs = t[4:4 + nin], t[4 + nin:4 + nin + nout]
        for o in outs:
            producer[o] = (t[0], ins)
        if t[0] == "rife.Warp":
            warps.append(ins)
        elif t[0] == "Sigmoid":
            sig = outs[0]
    assert len(warps) >= 2 and sig is not None, "no tail in this graph"

    def source(blob):      # back through the copies and the channel crop
        while blob in producer and producer[blob][0] in ("Crop", "Split"):
            blob = producer[blob][1][0]
        return blob
    a, b = source(warps[-2][1]), source(warps[-1][1])
    assert a == b, "the last two warps read different flow tensors (%s, %s)" % (a, b)
    return a, sig
