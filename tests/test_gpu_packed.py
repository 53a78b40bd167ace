"""16-bit packed RGB and RGBA (include/rife_hip.h "16-bit packed RGB and RGBA") on the GPU.  Every assertion is byte equality against code that existed before the
packed path did.

  A  the pre-processing kernel alone: ONE launch of k_preproc_packed / _vec through rife_hip_op_packed_to_rgb10 equals, dword for dword with the padding, the existing
     rife_hip_op_hbd_to_rgb10 on the de-interleaved colour planes in RGBP10 - 3 and 4 channels, depths 10, 12 and 16, samples above maxval among them; sizes from 1 x 1
     to a second workgroup across, the vector form (64 x 32, 72 x 34 with padded rows, and wide enough for a second workgroup of vector lanes), the scalar form forced
     and for real (one element off with an odd pitch); the call says which form ran.
  B  the blend alone: ONE launch of k_apply_packed through rife_hip_op_apply_packed equals the existing rife_hip_op_apply on the de-interleaved u16 planes (n = channels),
     re-interleaved, byte for byte with the sentinels around the rows - motions 1 x 1 .. 1030 x 5, F32 and F16 motion, the mask 16-byte aligned and one element off,
     maxval 4095 and 65535 on full-range random samples, zero / integer-shift / clamping random fields; vector form, forced scalar, and an output one element off.
  C  the calls: process_hbd_packed (3 channels) equals the interleaved planes of the existing process_hbd(..., PIX_RGBP10); with 4 channels the existing
     rife_hip_process_apply_sets on the numpy proxy with one four-plane set (packed_ref.expected); sizes 1 x 1 .. 256 x 192, depths 10, 12, 16, timesteps 0, 0.37, 0.5, 1,
     tight, row-padded and misaligned frames, flow scale 2, fast precision, the device call on pitched device frames; bytes around the output are kept; opaque alpha in
     gives maxval everywhere; the profiler shows one preproc_packed per input and one apply_packed per call.
  D  refusals by name on a rife-v2.3 engine and on -x / -z / -u engines, host and device, with the outputs untouched."""
import ctypes
import importlib

import numpy as np
import pytest

import packed_ref as pr

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")
amd = pkg.test_build()
hr = pr.hr

DEPTHS = (10, 12, 16)
CHS = (3, 4)
_ENG = {}


# ---- A: the pre-processing launch --------------------------------------------------------------------------------------------------------------------------------------
def _preproc_case(ch, w, h, depth, seed, pitch=None, offset=0, force_scalar=0, vector=None):
    a = pr.frames(w, h, ch, depth, seed, pitch, offset)[0]
    assert int(a[:, :, :3].max()) > (1 << depth) - 1 or depth == 16 or w * h < 2048, "no sample above maxval"
    got, vec = amd.op_packed_to_rgb10(a, depth, force_scalar)
    planes = tuple(pr.deinterleave(a)[:3])
    want = amd.op_hbd_to_rgb10(pkg.planes_image(planes, w, h, pkg.PIX_RGBP10), depth)
    what = "ch %d %dx%d depth %d pitch %s off %d forced %d" % (ch, w, h, depth, pitch, offset, force_scalar)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d dwords differ" % (what, int((got != want).sum()))
    assert not got[h:].any() and not got[:, w:].any(), what + ": the padding is not zero"
    if vector is not None:
        assert vec == vector, what + ": vector form %s" % vec


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (17, 9), (64, 32), (258, 130), (2056, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ch", CHS)
def test_preproc_is_the_planar_preproc_on_the_deinterleaved_planes(ch, size):
    w, h = size
    vector = w % (4 if ch == 4 else 8) == 0      # tight rows on a 64-byte-aligned base: the pitch is a multiple of 16 bytes whenever w allows the vector form
    for depth in DEPTHS:
        _preproc_case(ch, w, h, depth, 13 * depth + w, vector=vector)
        if size == (64, 32):
            _preproc_case(ch, w, h, depth, 13 * depth + w, force_scalar=1, vector=False)


@pytest.mark.parametrize("ch", CHS)
def test_preproc_forms_on_72x34(ch):
    for depth in DEPTHS:
        _preproc_case(ch, 72, 34, depth, 5 + depth, pitch=72 * ch + 8, vector=True)                       # aligned, padded rows
        _preproc_case(ch, 72, 34, depth, 5 + depth, pitch=72 * ch + 8, force_scalar=1, vector=False)
        _preproc_case(ch, 72, 34, depth, 5 + depth, pitch=72 * ch + 3, offset=1, vector=False)            # one element off, an odd pitch: the scalar form for real


def test_preproc_refusals():
    a = pr.frames(16, 8, 4, 12, 1)[0]
    d = pkg.packed_of(a, 12)
    L = amd.lib()
    out = np.zeros((32, 32), np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    bad = pkg.packed_of(a, 9)
    assert L.rife_hip_op_packed_to_rgb10(0, ctypes.byref(bad), p, 0) == -pkg.EINVAL and "the depth (9)" in L.rife_hip_last_error().decode()
    assert L.rife_hip_op_packed_to_rgb10(0, ctypes.byref(d), None, 0) == -pkg.EINVAL
    assert L.rife_hip_op_packed_to_rgb10(0, ctypes.byref(d), p, 2) == -pkg.EINVAL
    assert not out.any()


# ---- B: the blend launch -------------------------------------------------------------------------------------------------------------------------------------------------
def _aligned(rows, cols, dtype, fill, offset=0):
    """a (rows, cols) view, `offset` elements into a 64-byte-aligned array whose pitch is a multiple of 16 bytes, `fill` everywhere else"""
    es = np.dtype(dtype).itemsize
    pitch = (cols + offset + 15) // 16 * 16
    raw = np.full(rows * pitch + 64, fill, dtype)
    lead = (-raw.ctypes.data % 64) // es
    return raw[lead:lead + rows * pitch].reshape(rows, pitch)[:, offset:offset + cols]


def _motion(kind, mw, mh, dt, mask_off, rng):
    """flow (mh, mw, 4) and mask (mh, mw) of dtype dt as pitched windows inside NaN-filled arrays; the mask 16-byte aligned (mask_off 0) or one element off"""
    if kind == "zero":
        f = np.zeros((mh, mw, 4), np.float32)
    elif kind == "shift":
        f = np.broadcast_to(np.array([2, -1, -3, 1], np.float32), (mh, mw, 4)).copy()
    else:      # displacements up to 1.5 times the plane size: taps clamp on every side
        f = (rng.uniform(-1.5, 1.5, (mh, mw, 4)) * np.array([mw, mh, mw, mh])).astype(np.float32)
    m = rng.uniform(0.0, 1.0, (mh, mw)).astype(np.float32)
    fw = _aligned(mh, mw * 4, dt, np.nan).reshape(mh, mw, 4)
    mk = _aligned(mh, mw, dt, np.nan, mask_off)
    fw[...] = f.astype(dt); mk[...] = m.astype(dt)
    assert (mk.ctypes.data % 16 == 0) == (mask_off == 0)
    return fw, mk


@pytest.mark.parametrize("ch", CHS)
@pytest.mark.parametrize("size", [(1, 1), (2, 1), (1, 2), (3, 3), (5, 4), (33, 17), (130, 66), (1030, 5)], ids=lambda s: "%dx%d" % s)
def test_packed_blend_is_the_planar_blend_on_the_deinterleaved_planes(size, ch):
    w, h = size
    rng = np.random.default_rng(1000 * w + h + ch)
    geoms = [(pr.tight_pitch(w, ch, 8, pad=4), 0, 0, True),                   # rows padded to 16 bytes on an aligned base: the vector form
             (pr.tight_pitch(w, ch, 8, pad=4), 0, 1, False),                  # the same frames, forced scalar
             (pr.tight_pitch(w, ch, 1, pad=2, offset=1) | 1, 1, 0, False)]    # one element off, an odd pitch: the scalar form for real
    for pitch, offset, forced, vector in geoms:
        in0, in1 = pr.random_frames(w, h, ch, rng, pitch, offset)
        p0, p1 = pr.deinterleave(in0), pr.deinterleave(in1)
        for dt in (np.float32, np.float16):
            for mask_off in (0, 1):
                for depth in (12, 16):
                    maxval = (1 << depth) - 1
                    for kind in ("zero", "shift", "random"):
                        flow, mask = _motion(kind, w, h, dt, mask_off, rng)
                        planes = tuple(np.full((h, w), pr.SENTINEL, np.uint16) for _ in range(ch))
                        amd.op_apply(tuple(p0), tuple(p1), flow, mask, planes, maxval)
                        want = pr.blank_like(in0)
                        want[...] = pr.interleave(planes)
                        got = pr.blank_like(in0)
                        vec = amd.op_apply_packed(in0, in1, flow, mask, got, depth, forced)
                        what = "ch %d %dx%d pitch %d off %d forced %d %s mask_off %d maxval %d %s" % (ch, w, h, pitch, offset, forced, np.dtype(dt).name, mask_off, maxval, kind)
                        d = pkg.packed_of(got, depth)                            # the host's rule on what it is given (a one-row array has no row stride of its own)
                        unit = 8 if ch == 4 else 4
                        assert vec == (not forced and d.data % unit == 0 and d.pitch % unit == 0), what + ": vector form %s" % vec
                        assert h == 1 or vec == vector, what + ": vector form %s" % vec
                        assert np.array_equal(pr.big(got), pr.big(want)), what + ": %d samples differ" % int((pr.big(got) != pr.big(want)).sum())      # row padding included
                        assert pr.untouched(got), what + ": sentinel samples changed"
                        if kind == "random" and w * h > 64:
                            assert (got != np.minimum(in0, maxval)).any(), "a case without motion checks nothing"


def test_blend_refusals():
    rng = np.random.default_rng(3)
    in0, in1 = pr.random_frames(16, 8, 4, rng, 64)
    flow, mask = _motion("zero", 16, 8, np.float32, 0, rng)
    out = pr.blank_like(in0)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 1: the depth \(17\)"):
        L = amd.lib()
        a, b, o = pkg.packed_of(in0, 16), pkg.packed_of(in1, 17), pkg.packed_of(out, 16)
        m = pkg._motion_in(16, 8, flow, mask)
        pkg._check(L.rife_hip_op_apply_packed(0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o), ctypes.byref(m), 0), "op_apply_packed", L)
    three = pr.random_frames(16, 8, 3, rng, 48)[0]
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*differ in channels"):
        amd.op_apply_packed(in0, three, flow, mask, out, 16)
    assert (out == pr.SENTINEL).all()


# ---- C: the calls --------------------------------------------------------------------------------------------------------------------------------------------------------
def _engine(modeldirs, scale=1, precision="full"):
    key = (scale, precision)
    if key not in _ENG:
        g = pkg.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
        if scale == 2:
            g.set_flow_scale(2)
        g.set_precision(precision)
        _ENG[key] = g
    return _ENG[key]


def _want(g, in0, in1, t, depth):
    """3 channels: the existing hbd call on the de-interleaved planes; 4 channels: the existing sets call on the numpy proxy with one four-plane set"""
    if in0.shape[2] == 3:
        return pr.interleave(g.process_hbd(tuple(pr.deinterleave(in0)), tuple(pr.deinterleave(in1)), t, depth, pkg.PIX_RGBP10))
    return pr.expected(g, in0, in1, t, depth)


class _Dev:
    """a frame of packed_ref.view() in device memory with its geometry: the whole (rows, pitch) array goes up, the descriptor names the frame inside it"""

    def __init__(self, a, depth):
        import torch
        self.a = a
        parent, self.off = hr._GEOM[a.ctypes.data]
        self.t = torch.from_numpy(parent.view(np.int16)).cuda()
        self.img = pkg.packed_desc(a.shape[1], a.shape[0], a.shape[2], depth, self.t.data_ptr() + 2 * self.off, self.t.stride(0) * 2)

    def frame(self):
        """the frame as a host array; the array behind `a` takes everything that came back, so packed_ref.untouched() speaks about the device bytes"""
        parent = hr._GEOM[self.a.ctypes.data][0]
        parent[...] = self.t.cpu().numpy().view(np.uint16)
        return self.a


def _host_and_device(g, in0, in1, t, depth, what, stream=False):
    import torch
    want = _want(g, in0, in1, t, depth)
    out = pr.blank_like(in0)
    got = g.process_hbd_packed(in0, in1, t, depth, out=out)
    assert got is out and np.array_equal(got, want), "%s host: %d samples differ" % (what, int((got != want).sum()))
    assert pr.untouched(out), what + " host: bytes around the output changed"
    d0, d1, do = _Dev(in0, depth), _Dev(in1, depth), _Dev(pr.blank_like(in0), depth)
    st = torch.cuda.Stream() if stream else None
    torch.cuda.synchronize()
    g.process_device_hbd_packed(d0.img, d1.img, t, do.img, stream=st.cuda_stream if st else None)
    torch.cuda.synchronize()
    dgot = do.frame()
    assert np.array_equal(dgot, want), "%s device: %d samples differ" % (what, int((dgot != want).sum()))
    assert pr.untouched(dgot), what + " device: bytes around the output changed"
    return want


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("ch", CHS)
def test_packed_calls_are_the_planar_calls_on_the_deinterleaved_planes(ch, depth, modeldirs):
    g = _engine(modeldirs)
    maxval = (1 << depth) - 1
    for i, (w, h) in enumerate(((1, 1), (33, 17), (96, 64), (256, 192))):
        in0, in1 = pr.frames(w, h, ch, depth, 100 * depth + i)
        want = _host_and_device(g, in0, in1, 0.37, depth, "ch %d depth %d %dx%d tight" % (ch, depth, w, h), stream=(i % 2 == 1))
        if (w, h) == (96, 64):
            assert (want != np.minimum(in0, maxval)).any(), "a case without motion checks nothing"
    # row-padded frames; frames one element off their alignment with an odd pitch (every launch takes its scalar form); all four timesteps
    for pitch, off in ((96 * ch + 8, 0), (96 * ch + 5, 1)):
        in0, in1 = pr.frames(96, 64, ch, depth, 7 + depth, pitch, off)
        for t in (0.0, 0.37, 0.5, 1.0):
            want = _host_and_device(g, in0, in1, t, depth, "ch %d depth %d 96x64 pitch %d off %d t %s" % (ch, depth, pitch, off, t))
            if t in (0.0, 1.0):      # samples copied and clamped to maxval
                assert np.array_equal(want, np.minimum(in0 if t == 0.0 else in1, maxval)), "timestep %s" % t


@pytest.mark.parametrize("scale,precision", [(2, "full"), (1, "fast"), (2, "fast")])
@pytest.mark.parametrize("ch", CHS)
def test_packed_calls_at_flow_scale_2_and_fast_precision(ch, scale, precision, modeldirs):
    g = _engine(modeldirs, scale, precision)
    full = _engine(modeldirs)
    in0, in1 = pr.frames(100, 60, ch, 12, 31, 100 * ch + 4)
    want = _host_and_device(g, in0, in1, 0.5, 12, "ch %d scale %d %s" % (ch, scale, precision))
    if scale == 2:
        assert (want != _want(full, in0, in1, 0.5, 12)).any(), "flow scale 2 gave the frame of flow scale 1: the engine setting was not in force"


def test_opaque_alpha_stays_opaque(modeldirs):
    g = _engine(modeldirs)
    for depth in DEPTHS:
        in0, in1 = pr.frames(96, 64, 4, depth, 3 + depth, over=False, opaque=True)
        out = g.process_hbd_packed(in0, in1, 0.5, depth)
        assert (out[:, :, 3] == (1 << depth) - 1).all(), "depth %d: %d alpha samples are not maxval" % (depth, int((out[:, :, 3] != (1 << depth) - 1).sum()))
        assert np.array_equal(out, _want(g, in0, in1, 0.5, depth))


@pytest.mark.parametrize("ch", CHS)
def test_profiler_classes_of_a_packed_call(ch, modeldirs):
    import torch
    g = _engine(modeldirs)
    in0, in1 = pr.frames(100, 60, ch, 16, 41, 100 * ch + 4)
    for device in (False, True):
        if device:
            d0, d1, do = _Dev(in0, 16), _Dev(in1, 16), _Dev(pr.blank_like(in0), 16)
            torch.cuda.synchronize()
        g.profile_enable(True)
        if device:
            g.process_device_hbd_packed(d0.img, d1.img, 0.5, do.img)
        else:
            g.process_hbd_packed(in0, in1, 0.5, 16)
        prof = g.profile_read()
        g.profile_enable(False)
        assert prof["preproc_packed"]["launches"] == 2 and prof["apply_packed"]["launches"] == 1, prof
        assert not any(v["launches"] for k, v in prof.items() if k in ("preproc", "apply_motion", "apply_yuv")), "a planar launch ran in a packed call"


# ---- D: refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw,word", [("rife-v2.3", {}, "rife-v2"), ("rife-v4", {}, "rife-v4 (4.0)"), ("rife-v4.6", dict(tta_mode=True), "TTA mode (-x)"),
                                         ("rife-v4.6", dict(tta_temporal_mode=True), "temporal TTA mode (-z)"), ("rife-v4.6", dict(uhd_mode=True), "UHD mode (-u)")])
def test_other_families_and_modes_are_refused_by_name(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = pkg.RIFE(0, **fl); e.load(modeldirs[fam])
    for ch in CHS:
        in0, in1 = pr.frames(64, 64, ch, 12, 3, 64 * ch + 2)
        for t in (0.5, 0.0):
            out = pr.blank_like(in0)
            with pytest.raises(pkg.RifeError) as ex:
                e.process_hbd_packed(in0, in1, t, 12, out=out)
            assert "(-6)" in str(ex.value) and word in str(ex.value) and "high bit depth" in str(ex.value), str(ex.value)
            assert (out == pr.SENTINEL).all() and pr.untouched(out), "a refused call wrote into the output"
            d0, d1, do = _Dev(in0, 12), _Dev(in1, 12), _Dev(pr.blank_like(in0), 12)
            torch.cuda.synchronize()
            with pytest.raises(pkg.RifeError) as ex:
                e.process_device_hbd_packed(d0.img, d1.img, t, do.img)
            assert "(-6)" in str(ex.value) and word in str(ex.value) and "high bit depth" in str(ex.value), str(ex.value)
            torch.cuda.synchronize()
            back = do.frame()
            assert (back == pr.SENTINEL).all() and pr.untouched(back)


def test_bad_arguments_and_an_unloaded_engine(modeldirs):
    g = _engine(modeldirs)
    in0, in1 = pr.frames(32, 16, 4, 12, 9)
    out = pr.blank_like(in0)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 0: the depth \(17\) is not in 10\.\.16"):
        g.process_hbd_packed(in0, in1, 0.5, 17, out=out)
    wider = pr.frames(34, 16, 4, 12, 9)[0]
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 0 and image 1 differ in size"):
        g.process_hbd_packed(in0, wider, 0.5, 12, out=out)
    bare = pkg.RIFE(0, rife_v4=True)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*before load"):
        bare.process_hbd_packed(in0, in1, 0.5, 12, out=out)
    assert (out == pr.SENTINEL).all()
