"""Apply motion at another resolution (include/rife_hip.h rife_hip_apply_set_t) on the GPU: planes at half (4:2:0 / 4:2:2 chroma) or twice (proxy upscaling) the motion's size.

  A  the resampling identity, the sharp test: ONE launch of k_apply_motion_scaled through rife_hip_op_apply_scaled equals, byte for byte, one launch of the existing
     rife_hip_op_apply on the same planes with apply_scaled_ref.resample()'s float32 motion - dense and planted cases, all four sample types, the vector and the forced
     one-pixel form, extents 0, 0 / frame / 64-padded, F32 and F16 input motion (F16 is widened and resampled first; the comparison motion is F32).  On the strips
     the dense cases of the integer types run A alone: no seed brings their boundary set under the cap, and the identity needs no cap.
  B  the reference: planted cases byte for byte apply_ref.expected_exact, dense cases within apply_ref.holds on the resampled motion (the bars derived in
     tests/apply_ref.py; nothing new is measured).
     Every launch of A and B hands the motion over as a pitched window inside a larger array filled with NaN - a read outside mw x mh poisons the output - with the
     mask window 16-byte aligned (the wide mask loads) or one element off (element loads), each of them with F32 AND with F16 motion, and writes into planes inside a sentinel-filled array whose row padding
     must keep its bytes.
  C  bounds: output and input planes one element off their alignment, so that the one-pixel form runs for real; surroundings keep their bytes.
  D  the contract of the sets calls: process_apply_sets is process_motion (F32) plus the single apply calls; one shift-0 set is process_apply; the device forms
     likewise; timestep 0 / 1; the frame not wanted; fast precision; apply_motion_sets without a model and on a rife-v2.3 engine.
  E  refusals: other families and -x / -z get -ENOSYS with the words "apply motion" and leave the outputs untouched; a bad shift pair, a plane size that does not
     fit and 0 or 5 sets get -EINVAL by their words."""
import ctypes
import importlib

import numpy as np
import pytest

import apply_ref as ar
import apply_scaled_ref as asr
import motion_ref as mr

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")
amd = pkg.test_build()

_S = {ar.SAMPLE_U8: "u8", ar.SAMPLE_U16: "u16", ar.SAMPLE_F16: "f16", ar.SAMPLE_F32: "f32"}
FILL = 0x5a
KINDS = [(ar.SAMPLE_U8, 255), (ar.SAMPLE_U16, 4095), (ar.SAMPLE_F16, 0), (ar.SAMPLE_F32, 0)]      # all of them among apply_ref.DENSE_KINDS
N = 2
_kid = lambda k: "%s-%d" % (_S[k[0]], k[1])
_sid = lambda s: "%dx%d" % s
_hid = lambda s: asr.SHIFT_ID[tuple(s)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _out(c, off=0):
    """n output planes of the case's size inside one sentinel-filled array with padded rows, `off` elements into each row: (planes, the array).  off = 0: row length
    and numpy's 16-byte base keep every plane store-aligned, so force_scalar = 0 is the vector form; off = 1: no store is aligned and the host picks the one-pixel form."""
    n, h, w = c["p0"].shape
    W = w + (-w) % 8 + 8
    big = np.frombuffer(np.full(n * h * W * c["p0"].itemsize, FILL, np.uint8), c["p0"].dtype).reshape(n, h, W).copy()
    assert big.ctypes.data % 16 == 0
    return tuple(big[k, :, off:off + w] for k in range(n)), big


def _window(c, aligned):
    """the case's motion as pitched windows inside larger arrays filled with NaN: the flow one pixel and one row in, the mask one row and 8 elements (16-byte aligned:
    the wide loads) or 1 element (the element loads) in; both row lengths are multiples of 8 elements"""
    f, m = c["mflow"], c["mmask"]
    mh, mw = m.shape
    W = mw + (-mw) % 8 + 16
    bf = np.full((mh + 2, W, 4), np.nan, f.dtype); bm = np.full((mh + 2, W), np.nan, m.dtype)
    assert bf.ctypes.data % 16 == 0 and bm.ctypes.data % 16 == 0
    co = 8 if aligned else 1
    bf[1:1 + mh, 1:1 + mw] = f; bm[1:1 + mh, co:co + mw] = m
    wf, wm = bf[1:1 + mh, 1:1 + mw], bm[1:1 + mh, co:co + mw]
    assert (wm.ctypes.data % 16 == 0 and wm.strides[0] % 16 == 0) == aligned
    return wf, wm


def _check_rest(c, big, off):
    n, h, w = c["p0"].shape
    rest = np.ones(big.shape, bool); rest[:, :, off:off + w] = False
    assert (_bits(big).reshape(big.shape + (-1,))[rest] == FILL).all(), "bytes outside the output samples were written"


def _scaled(c, fs, aligned=True, off=0):
    planes, big = _out(c, off)
    wf, wm = _window(c, aligned)
    ext = None if c["extent"] == c["p0"].shape[:0:-1] else c["extent"]      # the plane size goes in as 0, 0; the unscaled launch it is compared with gets it spelled out
    amd.op_apply_scaled(c["p0"], c["p1"], wf, wm, planes, c["shift"], maxval=c["maxval"] or None, extent=ext, force_scalar=fs)
    _check_rest(c, big, off)
    w = c["p0"].shape[2]
    return np.ascontiguousarray(big[:, :, off:off + w])


def _plain(c, fs, off=0):
    """the existing launch on the resampled float32 motion"""
    planes, big = _out(c, off)
    amd.op_apply(c["p0"], c["p1"], c["flow"], c["mask"], planes, maxval=c["maxval"] or None, extent=c["extent"], force_scalar=fs)
    w = c["p0"].shape[2]
    return np.ascontiguousarray(big[:, :, off:off + w])


def _what(c, mw, mh, half, fs):
    return "%s %s %s/%d motion %dx%d planes %dx%d extent %s %s motion, %s form" % (
        c["kind"], _hid(c["shift"]), _S[c["sample"]], c["maxval"], mw, mh, c["p0"].shape[2], c["p0"].shape[1], c["extent"], "f16" if half else "f32", "scalar" if fs else "vector")


def _identity_and_reference(kind, shift, mw, mh, sample, maxval, reference=True):
    """A and B for every plane size the shift admits, both forms: the three extents with F32 motion, and the frame and the 64-padded extent with F16 motion.  The mask
    window's alignment is a column of its own: each motion format meets the 16-byte-aligned window (the wide mask loads) AND the window one element off (element
    loads).  reference=False: A alone, for a dense case whose boundary set no seed brings under the cap (no equality with the reference is claimed then)."""
    for ws, hs in asr.plane_sizes(shift, mw, mh):
        exts = asr.extents(shift, mw, mh, ws, hs)
        for ext, half, aligned in [(exts[0], False, True), (exts[1], False, False), (exts[2], False, True), (exts[1], True, False), (exts[2], True, True)]:
            c = asr.cached(kind, shift, mw, mh, ws, hs, N, sample, maxval, ext, half, capped=reference)
            got = {}
            for fs in (0, 1):
                got[fs] = _scaled(c, fs, aligned=aligned)
                want = _plain(c, fs)
                bad = _bits(got[fs]) != _bits(want)
                assert not bad.any(), "%s, mask window %s: %d of %d bytes differ from the unscaled launch on the resampled motion; first sample %s" % (
                    _what(c, mw, mh, half, fs), "aligned" if aligned else "one element off", int(bad.sum()), bad.size,
                    tuple(np.argwhere(got[fs] != want)[0]) if (got[fs] != want).any() else "(nan bits)")
            if not reference:
                continue
            if kind == "planted":
                exp = ar.expected_exact(c["ref"], sample, maxval)
                assert np.array_equal(_bits(got[0]), _bits(exp)), "%s: %d samples differ from the exact reference" % (_what(c, mw, mh, half, 0), int((got[0] != exp).sum()))
            else:
                ok, fig = ar.holds(got[0], c["ref"], sample, maxval)
                print("apply_scaled %s: %s" % (_what(c, mw, mh, half, 0), fig))
                assert ok, (_what(c, mw, mh, half, 0), fig)


# ---- A, B: single launches ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=_kid)
@pytest.mark.parametrize("size", asr.SIZES, ids=_sid)
@pytest.mark.parametrize("shift", asr.SHIFTS, ids=_hid)
def test_single_launch_is_the_unscaled_launch_on_the_resampled_motion(shift, size, kind):
    for k in ("planted", "dense"):
        _identity_and_reference(k, shift, size[0], size[1], *kind)


@pytest.mark.parametrize("kind", KINDS, ids=_kid)
@pytest.mark.parametrize("shift", asr.SHIFTS, ids=_hid)
def test_tiny_motions_planted(shift, kind):
    """1x1, 2x2, 3x3: at 3x3 the last chroma column and row have one sample; planes of one column take the four-single-loads form"""
    for mw, mh in asr.TINY:
        _identity_and_reference("planted", shift, mw, mh, *kind)


@pytest.mark.parametrize("kind", KINDS, ids=_kid)
@pytest.mark.parametrize("shift", asr.SHIFTS, ids=_hid)
def test_strip_with_a_second_workgroup_across(shift, kind):
    """2050x3 (down: 1025 plane pixels a row, 257 runs at R = 4 and 513 at R = 2) and 513x2 (up: 1026 / 1025): more than 256 runs per row"""
    mw, mh = asr.STRIP[shift]
    _identity_and_reference("planted", shift, mw, mh, *kind)
    _identity_and_reference("dense", shift, mw, mh, *kind, reference=kind in asr.DENSE_STRIP_KINDS)      # the integer types: the identity alone (apply_scaled_ref's docstring)


# ---- C: pointers off by one element ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=_kid)
@pytest.mark.parametrize("shift", asr.SHIFTS, ids=_hid)
def test_planes_off_by_one_element_take_the_scalar_form(shift, kind):
    sample, maxval = kind
    for mw, mh in ((3, 3), (100, 60), asr.STRIP[shift]):
        for ws, hs in asr.plane_sizes(shift, mw, mh):
            c = dict(asr.cached("planted", shift, mw, mh, ws, hs, N, sample, maxval, asr.frame_extent(shift, mw, mh)))
            exp = ar.expected_exact(c["ref"], sample, maxval)
            # input planes one element into padded rows too
            pad = lambda p: np.concatenate([np.zeros((N, hs, 1), p.dtype), p, np.zeros((N, hs, 2), p.dtype)], axis=2)
            c["p0"], c["p1"] = pad(c["p0"])[:, :, 1:1 + ws], pad(c["p1"])[:, :, 1:1 + ws]
            for half in (False, True):      # the planted grids are exact in half, so the F16 motion has the same expected output
                ch = dict(c, mflow=c["mflow"].astype(np.float16), mmask=c["mmask"].astype(np.float16)) if half else c
                assert np.array_equal(ch["mflow"].astype(np.float32), c["mflow"]) and np.array_equal(ch["mmask"].astype(np.float32), c["mmask"])
                for aligned in (True, False):
                    got = _scaled(ch, 0, aligned=aligned, off=1)
                    assert np.array_equal(_bits(got), _bits(exp)), "motion %dx%d (%s) planes %dx%d: %d samples differ" % (mw, mh, "f16" if half else "f32", ws, hs, int((got != exp).sum()))


def test_single_launch_refusals():
    c = asr.cached("planted", asr.SHIFT_420, 33, 47, 17, 24, N, ar.SAMPLE_U16, 4095)
    planes, _ = _out(c)
    call = lambda **kw: amd.op_apply_scaled(c["p0"], c["p1"], kw.pop("flow", c["mflow"]), kw.pop("mask", c["mmask"]), planes, kw.pop("shift", c["shift"]), maxval=4095, **kw)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 0: the extent"):
        call(extent=(16, 24))
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 0: the shift pair \(1, 0\)"):
        call(shift=(1, 0))
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 0: the plane size \(17 x 24\) does not fit a motion of 33 x 47 at shift \(-1, 0\)"):
        call(shift=(-1, 0))
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*force_scalar"):
        call(force_scalar=2)
    # a set of shift 0, 0 is the launch of op_apply
    c0 = ar.cached("planted", 33, 47, 3, ar.SAMPLE_U16, 1023)
    o1 = np.zeros_like(c0["p0"]); o2 = np.zeros_like(c0["p0"])
    amd.op_apply_scaled(c0["p0"], c0["p1"], c0["flow"], c0["mask"], o1, (0, 0), maxval=1023)
    amd.op_apply(c0["p0"], c0["p1"], c0["flow"], c0["mask"], o2, maxval=1023)
    assert np.array_equal(o1, o2) and np.array_equal(o1, ar.expected_exact(c0["ref"], ar.SAMPLE_U16, 1023))


# ---- D: the contract of the sets calls ----------------------------------------------------------------------------------------------------------------------------
_ENG = {}


def _engine(modeldirs, scale=1, precision="full"):
    key = (scale, precision)
    if key not in _ENG:
        g = pkg.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
        if scale == 2:
            g.set_flow_scale(2)
        g.set_precision(precision)
        _ENG[key] = g
    return _ENG[key]


@pytest.fixture(scope="module")
def bare():
    """an engine that has loaded no model: the apply calls need only its device"""
    return pkg.RIFE(0, rife_v4=True)


def _yuv_like(name):
    """planes of a deep 4:2:0 picture next to the 8-bit pair of `name`: u16 luma (n 1) and chroma (n 2) with samples up to 65535 (above the maxval of 4095: read as
    stored, only the output is clamped), and one float plane"""
    a, b = mr.e2e_pair(name)
    h, w = a.shape[:2]
    rng = np.random.default_rng([31, w, h])
    cw, ch = (w + 1) // 2, (h + 1) // 2
    Y = rng.integers(0, 65536, (2, 1, h, w)).astype(np.uint16)
    C = rng.integers(0, 65536, (2, 2, ch, cw)).astype(np.uint16)
    F = (rng.random((2, 1, h, w)) * 4 - 1).astype(np.float32)
    return a, b, Y, C, F


def _sets(g, w, h, Y, C, F, outs=(None, None, None)):
    wp, hp = g.padded_size(w, h)
    return [pkg.apply_set(Y[0], Y[1], (0, 0), 4095, (wp, hp), outs[0]), pkg.apply_set(C[0], C[1], (-1, -1), 4095, (wp // 2, hp // 2), outs[1]),
            pkg.apply_set(F[0], F[1], (0, 0), None, None, outs[2])]


@pytest.mark.parametrize("name,scale,precision", [("smooth", 1, "full"), ("ragged", 1, "full"), ("smooth", 2, "full"), ("ragged", 2, "full"), ("ragged", 1, "fast")],
                         ids=["96x64-scale1", "100x60-scale1", "96x64-scale2", "100x60-scale2", "100x60-fast"])
def test_process_apply_sets_is_process_motion_then_the_single_calls(name, scale, precision, modeldirs):
    g = _engine(modeldirs, scale, precision)
    a, b, Y, C, F = _yuv_like(name)
    h, w = a.shape[:2]
    wp, hp = g.padded_size(w, h)
    assert (wp, hp) == ar.padded(w, h, 32 * scale) and wp % 2 == 0 and hp % 2 == 0
    frame, flow, mask = g.process_motion(a, b, 0.5)
    want = [g.apply_motion(Y[0], Y[1], flow, mask, maxval=4095, extent=(wp, hp)),
            g.apply_motion_sets([pkg.apply_set(C[0], C[1], (-1, -1), 4095, (wp // 2, hp // 2))], flow, mask)[0],
            g.apply_motion(F[0], F[1], flow, mask)]
    # the single chroma call is the single launch of part A on the same motion
    one = np.zeros_like(C[0]); amd.op_apply_scaled(C[0], C[1], flow, mask, one, (-1, -1), maxval=4095, extent=(wp // 2, hp // 2))
    assert np.array_equal(np.stack(want[1]), one) and int(one.max()) <= 4095
    ok, fig = ar.holds(one, ar.apply64(C[0], C[1], *asr.resample(flow, mask, (-1, -1), C.shape[3], C.shape[2]), (wp // 2, hp // 2)), ar.SAMPLE_U16, 4095, equality=False)
    assert ok, fig
    fr, got = g.process_apply_sets(a, b, 0.5, _sets(g, w, h, Y, C, F))
    assert np.array_equal(fr, frame), "the frame of process_apply_sets is not process_motion's"
    for k in range(3):
        assert np.array_equal(_bits(np.stack(got[k])), _bits(np.stack(want[k]))), "set %d: %d bytes differ" % (k, int((_bits(np.stack(got[k])) != _bits(np.stack(want[k]))).sum()))
    # all three in one apply call on the exported motion
    got = g.apply_motion_sets(_sets(g, w, h, Y, C, F), flow, mask)
    assert all(np.array_equal(_bits(np.stack(got[k])), _bits(np.stack(want[k]))) for k in range(3))
    # the frame not wanted; output planes with padded rows, written in place
    big = [np.frombuffer(np.full(p[0].size * p.itemsize // p.shape[-1] * (p.shape[-1] + 5), FILL, np.uint8), p.dtype).reshape(p.shape[1:-1] + (p.shape[-1] + 5,)).copy() for p in (Y, C, F)]
    none, got = g.process_apply_sets(a, b, 0.5, _sets(g, w, h, Y, C, F, [x[..., :-5] for x in big]), want_frame=False)
    assert none is None
    for k in range(3):
        assert np.array_equal(_bits(big[k][..., :-5]), _bits(np.stack(want[k]))) and (_bits(big[k][..., -5:]) == FILL).all()
    # timestep 0 / 1: copies, integer samples clamped to maxval
    for t, i, fsrc in ((0.0, 0, a), (1.0, 1, b)):
        fr, got = g.process_apply_sets(a, b, t, _sets(g, w, h, Y, C, F))
        assert np.array_equal(fr, fsrc)
        assert np.array_equal(np.stack(got[0]), np.minimum(Y[i], 4095)) and np.array_equal(np.stack(got[1]), np.minimum(C[i], 4095)) and np.array_equal(_bits(np.stack(got[2])), _bits(F[i]))
    # a sets call with one shift-0 set is process_apply
    fr1, p1 = g.process_apply(a, b, 0.5, Y[0], Y[1], maxval=4095, extent=(wp, hp))
    fr2, p2 = g.process_apply_sets(a, b, 0.5, [pkg.apply_set(Y[0], Y[1], (0, 0), 4095, (wp, hp))])
    assert np.array_equal(fr1, fr2) and np.array_equal(np.stack(p1), np.stack(p2[0]))
    assert np.array_equal(g.process(a, b, 0.5), frame)      # a plain call afterwards returns its usual bytes


@pytest.mark.parametrize("name", ["smooth", "ragged"])
def test_device_sets_calls_are_the_single_device_calls(name, modeldirs):
    import torch
    g = _engine(modeldirs)
    a, b, Y, C, F = _yuv_like(name)
    h, w = a.shape[:2]
    wp, hp = g.padded_size(w, h)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dev = lambda p: torch.from_numpy(_bits(p).reshape(p.shape[:-1] + (-1,))).cuda()
    dY, dC, dF = dev(Y), dev(C), dev(F)

    def desc(t, like, maxval):      # t: (n, h, row bytes) uint8 on the device
        return pkg.planes_desc(like.shape[-1], like.shape[-2], pkg._SAMPLE_OF[like.dtype], [(t[k].data_ptr(), t.stride(1)) for k in range(t.shape[0])], maxval)

    def sets(oY, oC, oF):
        return [pkg.apply_set_desc(desc(dY[0], Y, 4095), desc(dY[1], Y, 4095), desc(oY, Y, 4095), (0, 0), (wp, hp)),
                pkg.apply_set_desc(desc(dC[0], C, 4095), desc(dC[1], C, 4095), desc(oC, C, 4095), (-1, -1), (wp // 2, hp // 2)),
                pkg.apply_set_desc(desc(dF[0], F, None), desc(dF[1], F, None), desc(oF, F, None), (0, 0), None)]

    blank = lambda t: torch.full(t.shape[1:], FILL, dtype=torch.uint8, device="cuda")
    for t in (0.5, 0.0, 1.0):
        for stream in (None, torch.cuda.Stream()):
            st = stream.cuda_stream if stream else None
            do1 = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda"); do2 = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda")
            df = torch.zeros((h, w * 16), dtype=torch.uint8, device="cuda"); dm = torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda")
            o1 = [blank(dY), blank(dC), blank(dF)]; o2 = [blank(dY), blank(dC), blank(dF)]
            torch.cuda.synchronize()
            mo = pkg.motion_desc(df.data_ptr(), dm.data_ptr(), 0, w * 16, w * 4)
            g.process_device_motion(da.data_ptr(), db.data_ptr(), w, h, t, do1.data_ptr(), mo, stream=st)
            s1 = sets(*o1)
            g.apply_device_motion(s1[0]._keep[0], s1[0]._keep[1], mo, s1[0]._keep[2], extent=(wp, hp), stream=st)      # the shift-0 sets through the existing call
            g.apply_device_motion_sets([s1[1]], mo, w, h, stream=st)
            g.apply_device_motion(s1[2]._keep[0], s1[2]._keep[1], mo, s1[2]._keep[2], stream=st)
            g.process_device_apply_sets(da.data_ptr(), db.data_ptr(), w, h, t, do2.data_ptr(), sets(*o2), stream=st)
            torch.cuda.synchronize()
            assert torch.equal(do1, do2), "timestep %s: the frames differ" % t
            if t == 0.5:
                for k in range(3):
                    assert torch.equal(o1[k], o2[k]), "set %d: the planes differ in %d bytes" % (k, int((o1[k] != o2[k]).sum().item()))
                host = g.apply_motion_sets([pkg.apply_set(C[0], C[1], (-1, -1), 4095, (wp // 2, hp // 2))], df.cpu().numpy().view(np.float32).reshape(h, w, 4), dm.cpu().numpy().view(np.float32).reshape(h, w))[0]
                assert np.array_equal(o2[1].cpu().numpy(), _bits(np.stack(host)).reshape(o2[1].shape)), "the device chroma planes are not the host call's"
            else:
                i = 0 if t == 0.0 else 1
                for o, src, clamp in ((o2[0], Y[i], True), (o2[1], C[i], True), (o2[2], F[i], False)):
                    want = np.minimum(src, 4095) if clamp else src
                    assert np.array_equal(o.cpu().numpy(), _bits(want).reshape(o.shape))


def test_apply_motion_sets_needs_no_model_and_serves_every_family(bare, modeldirs):
    v23 = pkg.RIFE(0, rife_v2=True); v23.load(modeldirs["rife-v2.3"])
    for e in (bare, v23):
        sets, want = [], []
        for shift, (sample, maxval) in zip(asr.SHIFTS, ((ar.SAMPLE_U16, 4095), (ar.SAMPLE_F16, 0), (ar.SAMPLE_U8, 255))):
            ws, hs = asr.plane_sizes(shift, 100, 60)[-1]
            ext = asr.frame_extent(shift, 100, 60)
            c = asr.cached("planted", shift, 100, 60, ws, hs, N, sample, maxval, ext)
            got = e.apply_motion_sets([pkg.apply_set(c["p0"], c["p1"], shift, maxval or None, ext)], c["mflow"], c["mmask"])[0]
            assert np.array_equal(_bits(np.stack(got)), _bits(ar.expected_exact(c["ref"], sample, maxval))), (shift, sample)
        # 4:2:0 and 4:2:2 chroma and a full-size plane of ONE motion in one call: each set is its own single call
        c = asr.cached("planted", asr.SHIFT_420, 100, 60, 50, 30, N, ar.SAMPLE_U16, 4095, (64, 32))
        c2 = asr.cached("planted", asr.SHIFT_422, 100, 60, 50, 60, N, ar.SAMPLE_F32, 0)
        c0 = ar.cached("planted", 100, 60, 3, ar.SAMPLE_U8, 255)
        mk = lambda: [pkg.apply_set(c["p0"], c["p1"], asr.SHIFT_420, 4095, (64, 32)), pkg.apply_set(c2["p0"], c2["p1"], asr.SHIFT_422), pkg.apply_set(c0["p0"], c0["p1"])]
        got = e.apply_motion_sets(mk(), c["mflow"], c["mmask"])
        for k, s in enumerate(mk()):
            single = e.apply_motion_sets([s], c["mflow"], c["mmask"])[0]
            assert np.array_equal(_bits(np.stack(got[k])), _bits(np.stack(single))), k
        assert np.array_equal(np.stack(got[0]), ar.expected_exact(c["ref"], ar.SAMPLE_U16, 4095))
    a = np.zeros((60, 100, 3), np.uint8)
    with pytest.raises(pkg.RifeError, match="before load"):
        bare.process_apply_sets(a, a, 0.5, [pkg.apply_set(c["p0"], c["p1"], asr.SHIFT_420, 4095)])


# ---- E: refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife-v3.1", {}, "rife-v3"), ("rife", {}, "rife (v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = pkg.RIFE(0, **fl); e.load(modeldirs[fam])
    w, h = 64, 64
    a = np.zeros((h, w, 3), np.uint8)
    q = np.zeros((2, h // 2, w // 2), np.uint16)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for t in (0.5, 0.0):
        out = np.full((h, w, 3), FILL, np.uint8); po = np.full(q.shape, FILL * 257, np.uint16)
        n, arr = pkg._set_array([pkg.apply_set(q, q, (-1, -1), out=po)])
        rc = e._L.rife_hip_process_apply_sets(e._h, p(a), p(a), w, h, t, p(out), 0, n, arr)
        msg = e._L.rife_hip_last_error().decode()
        assert rc == -pkg.ENOSYS and word in msg and "apply motion" in msg, (rc, msg)
        assert (out == FILL).all() and (po == FILL * 257).all(), "a refused call wrote into an output buffer"
        da = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"); dq = torch.zeros((2, h // 2, w), dtype=torch.uint8, device="cuda")
        dout = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda"); dpo = torch.full((2, h // 2, w), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        planes = lambda tt: pkg.planes_desc(w // 2, h // 2, ar.SAMPLE_U16, [(tt[k].data_ptr(), w) for k in range(2)])
        with pytest.raises(pkg.RifeError) as ex:
            e.process_device_apply_sets(da.data_ptr(), da.data_ptr(), w, h, t, dout.data_ptr(), [pkg.apply_set_desc(planes(dq), planes(dq), planes(dpo), (-1, -1))])
        assert "(-6)" in str(ex.value) and word in str(ex.value) and "apply motion" in str(ex.value), str(ex.value)
        torch.cuda.synchronize()
        assert (dout == FILL).all().item() and (dpo == FILL).all().item()


def test_bad_sets_are_refused_with_einval(bare, modeldirs):
    g = _engine(modeldirs)
    c = asr.cached("planted", asr.SHIFT_420, 100, 60, 50, 30, N, ar.SAMPLE_U16, 4095)
    a = np.zeros((60, 100, 3), np.uint8)
    mk = lambda shift=asr.SHIFT_420: pkg.apply_set(c["p0"], c["p1"], shift, 4095)
    for call in (lambda ss: bare.apply_motion_sets(ss, c["mflow"], c["mmask"]), lambda ss: g.process_apply_sets(a, a, 0.5, ss)):
        with pytest.raises(pkg.RifeError, match=r"\(-1\).*the set count \(0\) is not in 1\.\.4"):
            call([])
        with pytest.raises(pkg.RifeError, match=r"\(-1\).*the set count \(5\) is not in 1\.\.4"):
            call([mk()] * 5)
        with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 1: the shift pair \(0, -1\) is not one of"):
            call([mk(), mk((0, -1))])
        with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 2: the plane size \(50 x 30\) does not fit a motion of 100 x 60 at shift \(1, 1\)"):
            call([mk(), mk(), mk((1, 1))])
        with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 0: the plane size \(50 x 30\) does not fit"):
            call([mk((0, 0))])
    assert len(bare.apply_motion_sets([mk()] * 4, c["mflow"], c["mmask"])) == 4
