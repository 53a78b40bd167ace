"""Semi-planar high bit depth (include/rife_hip.h "semi-planar high bit depth") on the GPU.  Every assertion is byte equality against code that existed before the
semi-planar path did, on split(img) (tests/semiplanar_ref.py), joined back.

  A  the pre-processing kernel alone: ONE launch of k_preproc_sp / _vec through rife_hip_op_sp_to_rgb10 equals, dword for dword with the padding, the existing
     rife_hip_op_hbd_to_rgb10 on split(img) - 4:2:0 and 4:2:2, depths 10, 12 and 16, BT.709 and BT.2020, random low bits under the code; sizes 1 x 1, 3 x 3, 33 x 17,
     72 x 34 on aligned planes with padded rows (the vector form, and forced scalar) and one element off (the scalar form for real), 1030 x 5 (a second workgroup
     across in the scalar form); the call says which form ran.
  B  the blend alone: ONE launch of k_apply_sp through rife_hip_op_apply_sp equals join(op_apply_yuv(split(...)) << s), byte for byte with the sentinels in the row
     padding and around the planes - motions 1 x 1 .. 1030 x 5, F32 and F16 motion, the mask 16-byte aligned and one element off, depths 10, 12, 16, both chroma
     modes, zero / integer-shift / clamping / few-pixel random fields on full-range random samples; vector form, forced scalar, and an output one element off.
  C  the calls: process_hbd_semiplanar and process_device_hbd_semiplanar equal the existing process_hbd on split, joined back - sizes 1 x 1 .. 256 x 192, depths 10,
     12, 16, timesteps 0, 0.25, 0.5, 1, flow scale 2, fast precision, pitched device planes; bytes around the output are kept; the profiler shows one preproc_sp per
     input and one apply_sp per call.
  D  refusals by name on a rife-v2.3 engine and on a -x engine, host and device, with the outputs untouched."""
import ctypes
import importlib

import numpy as np
import pytest

import semiplanar_ref as sr

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")
amd = pkg.test_build()
hr = sr.hr

DEPTHS = (10, 12, 16)
CHROMAS = (1, 2)
_ENG = {}


# ---- A: the pre-processing launch --------------------------------------------------------------------------------------------------------------------------------------
def _preproc_case(chroma, w, h, depth, csp, seed, pad=0, offset=0, multiple=1, odd=False, force_scalar=0, vector=None):
    sf = sr.surfaces(w, h, chroma, depth, seed, pad, offset, multiple, odd)[0]
    assert depth == 16 or any((p & ((1 << (16 - depth)) - 1)).any() for p in sf), "no garbage in the low bits"
    got, vec = amd.op_sp_to_rgb10(sf[0], sf[1], depth, chroma, csp, force_scalar)
    want = amd.op_hbd_to_rgb10(pkg.planes_image(tuple(sr.split(sf, depth)), w, h, sr.pixfmt(chroma, csp)), depth)
    what = "chroma %d %dx%d depth %d csp %d pad %d off %d forced %d" % (chroma, w, h, depth, csp, pad, offset, force_scalar)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d dwords differ" % (what, int((got != want).sum()))
    assert not got[h:].any() and not got[:, w:].any(), what + ": the padding is not zero"
    if w * h > 64:
        assert len(np.unique(got[:h, :w])) > 8, what + ": a flat frame checks nothing"
    if vector is not None:
        assert vec == vector, what + ": vector form %s" % vec


@pytest.mark.parametrize("size", [(1, 1), (3, 3), (33, 17), (1030, 5)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("chroma", CHROMAS)
def test_preproc_is_the_planar_preproc_on_split(chroma, size):
    w, h = size
    for depth in DEPTHS:
        for csp in (pkg.CSP_BT709, pkg.CSP_BT2020NCL):
            _preproc_case(chroma, w, h, depth, csp, 13 * depth + w, vector=False)      # no width here is a multiple of 8


@pytest.mark.parametrize("chroma", CHROMAS)
def test_preproc_forms_on_72x34(chroma):
    for depth in DEPTHS:
        for csp in (pkg.CSP_BT709, pkg.CSP_BT2020NCL):
            _preproc_case(chroma, 72, 34, depth, csp, 5 + depth, pad=8, multiple=8, vector=True)                       # aligned planes, padded rows
            _preproc_case(chroma, 72, 34, depth, csp, 5 + depth, pad=8, multiple=8, force_scalar=1, vector=False)
            _preproc_case(chroma, 72, 34, depth, csp, 5 + depth, pad=2, offset=1, odd=True, vector=False)             # one element off, an odd pitch: the scalar form for real


def test_preproc_refusals():
    y, c = sr.surfaces(16, 8, 1, 12, 1)[0]
    d = pkg.semiplanar_of(y, c, 12, 1)
    L = amd.lib()
    out = np.zeros((32, 32), np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    bad = pkg.semiplanar_of(y, c, 9, 1)
    assert L.rife_hip_op_sp_to_rgb10(0, ctypes.byref(bad), p, 0) == -pkg.EINVAL and "the depth (9)" in L.rife_hip_last_error().decode()
    assert L.rife_hip_op_sp_to_rgb10(0, ctypes.byref(d), None, 0) == -pkg.EINVAL
    assert L.rife_hip_op_sp_to_rgb10(0, ctypes.byref(d), p, 2) == -pkg.EINVAL
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
    elif kind == "small":      # a few pixels, fractional
        f = rng.uniform(-3.0, 3.0, (mh, mw, 4)).astype(np.float32)
    else:                      # displacements up to 1.5 times the plane size: taps clamp on every side
        f = (rng.uniform(-1.5, 1.5, (mh, mw, 4)) * np.array([mw, mh, mw, mh])).astype(np.float32)
    m = rng.uniform(0.0, 1.0, (mh, mw)).astype(np.float32)
    fw = _aligned(mh, mw * 4, dt, np.nan).reshape(mh, mw, 4)
    mk = _aligned(mh, mw, dt, np.nan, mask_off)
    fw[...] = f.astype(dt); mk[...] = m.astype(dt)
    assert (mk.ctypes.data % 16 == 0) == (mask_off == 0)
    return fw, mk


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 3), (4, 4), (33, 17), (1030, 5)], ids=lambda s: "%dx%d" % s)
def test_sp_blend_is_the_planar_blend_on_split(size, chroma):
    w, h = size
    rng = np.random.default_rng(1000 * w + h + chroma)
    shift = (-1, -1) if chroma == 1 else (-1, 0)
    geoms = [(dict(pad=4, multiple=8), 0, True),                      # rows padded to 16 bytes on an aligned base: the vector form where w >= 4
             (dict(pad=4, multiple=8), 1, False),                     # the same surfaces, forced scalar
             (dict(pad=2, offset=1, odd=True), 0, False)]             # one element off, an odd pitch: the scalar form for real
    moved = False
    for geom, forced, vector in geoms:
        in0, in1 = sr.random_surfaces(w, h, chroma, rng, **geom)
        for depth in DEPTHS:
            s, maxval = 16 - depth, (1 << depth) - 1
            p0, p1 = sr.split(in0, depth), sr.split(in1, depth)
            for dt in (np.float32, np.float16):
                for mask_off in (0, 1):
                    for kind in ("zero", "shift", "small", "random"):
                        flow, mask = _motion(kind, w, h, dt, mask_off, rng)
                        planes = [np.full(p.shape, 0x5a5a, np.uint16) for p in p0]
                        amd.op_apply_yuv(p0[:1], p1[:1], p0[1:], p1[1:], flow, mask, planes[:1], planes[1:], shift, maxval)
                        assert all(int(p.max()) <= maxval for p in planes)
                        want = sr.blank_like(in0)
                        sr.fill(want, planes, depth)
                        got = sr.blank_like(in0)
                        vec = amd.op_apply_sp(in0, in1, flow, mask, got, depth, chroma, forced)
                        what = "chroma %d %dx%d %s forced %d %s mask_off %d depth %d %s" % (chroma, w, h, geom, forced, np.dtype(dt).name, mask_off, depth, kind)
                        d = pkg.semiplanar_of(got[0], got[1], depth, chroma)      # the host's rule on what it is given (a one-row array has no row stride of its own)
                        assert vec == (not forced and w >= 4 and (d.y | d.cbcr | d.pitch_y | d.pitch_c) % 8 == 0), what + ": vector form %s" % vec
                        assert h == 1 or vec == (vector and w >= 4), what + ": vector form %s" % vec
                        for g, w_ in zip(got, want):
                            assert np.array_equal(sr.big(g), sr.big(w_)), what + ": %d samples differ" % int((sr.big(g) != sr.big(w_)).sum())      # row padding included
                        assert sr.untouched(got), what + ": sentinel samples changed"
                        if s:
                            assert not any((g & ((1 << s) - 1)).any() for g in got), what + ": low bits written"
                        if kind in ("small", "random") and w * h > 64:
                            moved = moved or (got[0] != (in0[0] >> s) << s).any()
    assert moved or w * h <= 64, "no case with motion"


def test_blend_refusals():
    rng = np.random.default_rng(3)
    in0, in1 = sr.random_surfaces(16, 8, 1, rng)
    flow, mask = _motion("zero", 16, 8, np.float32, 0, rng)
    out = sr.blank_like(in0)
    L = amd.lib()
    a, b, o = pkg.semiplanar_of(*in0, 16, 1), pkg.semiplanar_of(*in1, 17, 1), pkg.semiplanar_of(*out, 16, 1)
    m = pkg._motion_in(16, 8, flow, mask)
    assert L.rife_hip_op_apply_sp(0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o), ctypes.byref(m), 16, 8, 0) == -pkg.EINVAL
    assert "image 1: the depth (17)" in L.rife_hip_last_error().decode()
    b = pkg.semiplanar_of(*in1, 16, 1)
    assert L.rife_hip_op_apply_sp(0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o), ctypes.byref(m), 8, 8, 0) == -pkg.EINVAL
    assert "the motion has the luma size" in L.rife_hip_last_error().decode()
    two = sr.random_surfaces(16, 8, 2, rng)[0]
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*differ in chroma"):
        c2 = pkg.semiplanar_of(*two, 16, 2)
        pkg._check(L.rife_hip_op_apply_sp(0, ctypes.byref(a), ctypes.byref(c2), ctypes.byref(o), ctypes.byref(m), 16, 8, 0), "op_apply_sp", L)
    assert all((p == sr.SENTINEL).all() for p in out)


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


class _Dev:
    """a surface of semiplanar_ref.surface() in device memory with its geometry: the whole (rows, pitch) array behind each plane goes up, the descriptor names the
    planes inside them"""

    def __init__(self, sf, depth, chroma, csp=0):
        import torch
        self.sf = sf
        self.t = []
        ptr = []
        for p in sf:
            parent, off = hr._GEOM[p.ctypes.data]
            t = torch.from_numpy(parent.view(np.int16)).cuda()
            self.t.append(t)
            ptr.append((t.data_ptr() + 2 * off, t.stride(0) * 2))
        self.img = pkg.semiplanar_desc(sf[0].shape[1], sf[0].shape[0], chroma, depth, ptr[0][0], ptr[0][1], ptr[1][0], ptr[1][1], csp)

    def surface(self):
        """the surface as host arrays; the arrays behind it take everything that came back, so semiplanar_ref.untouched() speaks about the device bytes"""
        for p, t in zip(self.sf, self.t):
            hr._GEOM[p.ctypes.data][0][...] = t.cpu().numpy().view(np.uint16)
        return self.sf


def _differ(got, want):
    return sum(int((g != w_).sum()) for g, w_ in zip(got, want))


def _host_and_device(g, in0, in1, t, depth, chroma, what, csp=0, stream=False):
    import torch
    want = sr.expected(g, in0, in1, t, depth, chroma, csp)
    out = sr.blank_like(in0)
    got = g.process_hbd_semiplanar(in0, in1, t, depth, chroma, csp, out=out)
    assert got[0] is out[0] and got[1] is out[1] and _differ(got, want) == 0, "%s host: %d samples differ" % (what, _differ(got, want))
    assert sr.untouched(out), what + " host: bytes around the output changed"
    d0, d1, do = _Dev(in0, depth, chroma, csp), _Dev(in1, depth, chroma, csp), _Dev(sr.blank_like(in0), depth, chroma, csp)
    st = torch.cuda.Stream() if stream else None
    torch.cuda.synchronize()
    g.process_device_hbd_semiplanar(d0.img, d1.img, t, do.img, stream=st.cuda_stream if st else None)
    torch.cuda.synchronize()
    dgot = do.surface()
    assert _differ(dgot, want) == 0, "%s device: %d samples differ" % (what, _differ(dgot, want))
    assert sr.untouched(dgot), what + " device: bytes around the output changed"
    return want


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("chroma", CHROMAS)
def test_sp_calls_are_the_planar_calls_on_split(chroma, depth, modeldirs):
    g = _engine(modeldirs)
    s = 16 - depth
    for i, (w, h) in enumerate(((1, 1), (33, 17), (96, 64), (256, 192))):
        in0, in1 = sr.surfaces(w, h, chroma, depth, 100 * depth + i)
        want = _host_and_device(g, in0, in1, 0.25, depth, chroma, "chroma %d depth %d %dx%d tight" % (chroma, depth, w, h), stream=(i % 2 == 1))
        if (w, h) == (96, 64):
            assert (want[0] != (in0[0] >> s) << s).any(), "a case without motion checks nothing"
    # row-padded aligned planes (pitched device planes too), and planes one element off with an odd pitch (every launch takes its scalar form); all four timesteps
    for geom in (dict(pad=8, multiple=8), dict(pad=3, offset=1, odd=True)):
        in0, in1 = sr.surfaces(96, 64, chroma, depth, 7 + depth, **geom)
        for t in (0.0, 0.25, 0.5, 1.0):
            want = _host_and_device(g, in0, in1, t, depth, chroma, "chroma %d depth %d 96x64 %s t %s" % (chroma, depth, geom, t), csp=pkg.CSP_BT2020NCL)
            if t in (0.0, 1.0):      # the samples of one frame, the low bits cleared
                src = in0 if t == 0.0 else in1
                assert all(np.array_equal(w_, (p >> s) << s) for w_, p in zip(want, src)), "timestep %s" % t
                assert depth == 16 or any((p != w_).any() for w_, p in zip(want, src)), "no low bits to clear"


@pytest.mark.parametrize("scale,precision", [(2, "full"), (1, "fast")])
@pytest.mark.parametrize("chroma", CHROMAS)
def test_sp_calls_at_flow_scale_2_and_fast_precision(chroma, scale, precision, modeldirs):
    g = _engine(modeldirs, scale, precision)
    full = _engine(modeldirs)
    in0, in1 = sr.surfaces(100, 60, chroma, 12, 31, pad=4)
    want = _host_and_device(g, in0, in1, 0.5, 12, chroma, "chroma %d scale %d %s" % (chroma, scale, precision))
    if scale == 2:
        assert _differ(want, sr.expected(full, in0, in1, 0.5, 12, chroma)) > 0, "flow scale 2 gave the frame of flow scale 1: the engine setting was not in force"


@pytest.mark.parametrize("chroma", CHROMAS)
def test_profiler_classes_of_a_semiplanar_call(chroma, modeldirs):
    import torch
    g = _engine(modeldirs)
    in0, in1 = sr.surfaces(100, 60, chroma, 16, 41, pad=4)
    for device in (False, True):
        if device:
            d0, d1, do = _Dev(in0, 16, chroma), _Dev(in1, 16, chroma), _Dev(sr.blank_like(in0), 16, chroma)
            torch.cuda.synchronize()
        g.profile_enable(True)
        if device:
            g.process_device_hbd_semiplanar(d0.img, d1.img, 0.5, do.img)
        else:
            g.process_hbd_semiplanar(in0, in1, 0.5, 16, chroma)
        prof = g.profile_read()
        g.profile_enable(False)
        assert prof["preproc_sp"]["launches"] == 2 and prof["apply_sp"]["launches"] == 1, prof
        assert not any(v["launches"] for k, v in prof.items() if k in ("preproc", "preproc_packed", "apply_motion", "apply_yuv", "apply_packed")), "a planar launch ran in a semi-planar call"


# ---- D: refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw,word", [("rife-v2.3", {}, "rife-v2"), ("rife-v4.6", dict(tta_mode=True), "TTA mode (-x)")])
def test_other_families_and_modes_are_refused_by_name(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = pkg.RIFE(0, **fl); e.load(modeldirs[fam])
    for chroma in CHROMAS:
        in0, in1 = sr.surfaces(64, 64, chroma, 12, 3, pad=2)
        for t in (0.5, 0.0):
            out = sr.blank_like(in0)
            with pytest.raises(pkg.RifeError) as ex:
                e.process_hbd_semiplanar(in0, in1, t, 12, chroma, out=out)
            assert "(-6)" in str(ex.value) and word in str(ex.value) and "high bit depth" in str(ex.value), str(ex.value)
            assert all((p == sr.SENTINEL).all() for p in out) and sr.untouched(out), "a refused call wrote into the output"
            d0, d1, do = _Dev(in0, 12, chroma), _Dev(in1, 12, chroma), _Dev(sr.blank_like(in0), 12, chroma)
            torch.cuda.synchronize()
            with pytest.raises(pkg.RifeError) as ex:
                e.process_device_hbd_semiplanar(d0.img, d1.img, t, do.img)
            assert "(-6)" in str(ex.value) and word in str(ex.value) and "high bit depth" in str(ex.value), str(ex.value)
            torch.cuda.synchronize()
            back = do.surface()
            assert all((p == sr.SENTINEL).all() for p in back) and sr.untouched(back)


def test_bad_arguments_and_an_unloaded_engine(modeldirs):
    g = _engine(modeldirs)
    in0, in1 = sr.surfaces(32, 16, 1, 12, 9)
    out = sr.blank_like(in0)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 0: the depth \(17\) is not in 10\.\.16"):
        g.process_hbd_semiplanar(in0, in1, 0.5, 17, 1, out=out)
    wider = sr.surfaces(34, 16, 1, 12, 9)[0]
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 0 and image 1 differ in size"):
        g.process_hbd_semiplanar(in0, wider, 0.5, 12, 1, out=out)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 0: RIFE_HIP_CSP_FULL"):
        g.process_hbd_semiplanar(in0, in1, 0.5, 12, 1, pkg.CSP_FULL, out=out)
    bare = pkg.RIFE(0, rife_v4=True)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*before load"):
        bare.process_hbd_semiplanar(in0, in1, 0.5, 12, 1, out=out)
    assert all((p == sr.SENTINEL).all() for p in out)
