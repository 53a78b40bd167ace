"""High bit depth (include/rife_hip.h "high bit depth") on the GPU.  Every assertion is byte equality against something that is not the code under test.

  A  the pre-processing kernel alone: ONE launch of k_preproc_hbd / k_preproc_hbd_rgb through rife_hip_op_hbd_to_rgb10 equals, dword for dword (padding included),
     the existing rife_hip_op_image_to_resident on the numpy-reduced planes (tests/hbd_ref.py reduce10) in the ten-bit format - all four layouts, depths 10, 12 and 16,
     BT.709 and BT.2020, samples above maxval among them; sizes from 1 x 1 to more than one workgroup across, the x8 form (64 x 32, 72 x 34 on aligned planes) and the
     scalar form (forced, and for real on planes one element off their alignment with odd pitches).
  B  the call: process_hbd and process_device_hbd equal the composition of reduce10 and the EXISTING rife_hip_process_apply_sets /
     rife_hip_process_device_apply_sets (hbd_ref.expected) - four layouts by three depths, sizes 1 x 1 .. 256 x 192, tight, row-padded and misaligned planes, timesteps
     0, 0.37, 0.5 and 1, flow scale 2, fast precision; the bytes around the output planes keep their values.  The profiler's classes show the fused launch on aligned
     planes, the two launches on misaligned ones and with RIFE_HIP_APPLY_YUV=0 (test build), and the same planes either way.
  A2 the fused apply launch alone: rife_hip_op_apply_yuv equals rife_hip_op_apply on the luma set plus rife_hip_op_apply_scaled on the chroma set, byte for byte with the
     row padding - motions 1 x 1 .. 1030 x 5 (a second workgroup across a chroma row), 4:2:0 and 4:2:2, F32 and F16 motion, the mask 16-byte aligned and one element
     off, maxval 4095 and 65535, zero / integer-shift / clamping random fields; the call says whether it was one launch (w >= 4, aligned stores) or the two.
  C  refusals by name on a rife-v2.3 engine and on -x / -z / -u engines, host and device, with the outputs untouched."""
import ctypes
import importlib

import numpy as np
import pytest

import hbd_ref as hr

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")
amd = pkg.test_build()

DEPTHS = (10, 12, 16)
_fid = lambda p: hr.NAME[p]
_ENG = {}


def _csps(pixfmt):
    return (0,) if pixfmt == pkg.PIX_RGBP10 else (pkg.CSP_BT709, pkg.CSP_BT2020NCL)


# ---- A: the pre-processing launch --------------------------------------------------------------------------------------------------------------------------------------
def _preproc_case(pixfmt, w, h, depth, seed, pitch_pad=0, offset=0, force_scalar=0):
    ps = hr.planes(w, h, pixfmt, depth, seed, pitch_pad, offset)[0]
    assert max(int(p.max()) for p in ps) > (1 << depth) - 1 or depth == 16 or w * h < 2048, "no sample above maxval"
    ten = tuple(np.ascontiguousarray(hr.reduce10(p, depth)) for p in ps)
    for csp in _csps(pixfmt):
        got = amd.op_hbd_to_rgb10(pkg.planes_image(tuple(ps), w, h, pixfmt | csp), depth, force_scalar)
        want = amd.op_image_to_resident(pkg.planes_image(ten, w, h, pixfmt | csp))
        assert got.shape == want.shape and np.array_equal(got, want), "%s %dx%d depth %d csp %#x: %d dwords differ" % (hr.NAME[pixfmt], w, h, depth, csp, int((got != want).sum()))
        assert not got[h:].any() and not got[:, w:].any(), "the padding is not zero"


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (17, 9), (64, 32), (258, 130)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pixfmt", hr.BASES, ids=_fid)
def test_preproc_is_the_ten_bit_preproc_on_reduced_planes(pixfmt, size):
    for depth in DEPTHS:
        _preproc_case(pixfmt, size[0], size[1], depth, 11 * depth + size[0])
        if size == (64, 32):      # the x8 form ran above (aligned planes, w % 8 == 0); the scalar form on the same planes
            _preproc_case(pixfmt, size[0], size[1], depth, 11 * depth + size[0], force_scalar=1)


@pytest.mark.parametrize("pixfmt", hr.BASES, ids=_fid)
def test_preproc_forms_on_72x34(pixfmt):
    for depth in DEPTHS:
        _preproc_case(pixfmt, 72, 34, depth, 5 + depth, pitch_pad=8)                      # aligned, padded rows: the x8 form
        _preproc_case(pixfmt, 72, 34, depth, 5 + depth, pitch_pad=8, force_scalar=1)
        _preproc_case(pixfmt, 72, 34, depth, 5 + depth, pitch_pad=2, offset=1)            # one element off, odd pitches: the scalar form for real


def test_preproc_refusals():
    ps = hr.planes(16, 8, pkg.PIX_I420P10, 12, 1)[0]
    im = pkg.planes_image(tuple(ps), 16, 8, pkg.PIX_I420P10)
    L = amd.lib()
    out = np.zeros((32, 32), np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert L.rife_hip_op_hbd_to_rgb10(0, ctypes.byref(im), 9, p, 0) == -pkg.EINVAL and "the depth (9)" in L.rife_hip_last_error().decode()
    assert L.rife_hip_op_hbd_to_rgb10(0, ctypes.byref(im), 12, None, 0) == -pkg.EINVAL
    assert L.rife_hip_op_hbd_to_rgb10(0, ctypes.byref(im), 12, p, 2) == -pkg.EINVAL
    u8 = np.zeros((8, 16), np.uint8)
    i444 = pkg.planes_image((u8, u8, u8), 16, 8, pkg.PIX_I444)
    assert L.rife_hip_op_hbd_to_rgb10(0, ctypes.byref(i444), 12, p, 0) == -pkg.EINVAL and "pixel format 49 is not a high-bit-depth layout" in L.rife_hip_last_error().decode()
    assert not out.any()


# ---- A2: the fused apply launch -----------------------------------------------------------------------------------------------------------------------------------------
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


def _yuv_planes(mw, mh, shift, rng, offset=0):
    """(luma, chroma) planes of two frames: random u16 over the whole range (samples above maxval are read as stored), luma pitches multiples of 8 bytes"""
    cw, ch = (mw + 1) // 2, (mh + 1) // 2 if shift[1] < 0 else mh
    mk = lambda rows, cols: hr._view(rows, cols, (cols + offset + 7) // 8 * 8, offset)
    frames = []
    for f in range(2):
        y = mk(mh, mw); y[...] = rng.integers(0, 65536, (mh, mw), dtype=np.uint32).astype(np.uint16)
        c = [mk(ch, cw), mk(ch, cw)]
        for q in c:
            q[...] = rng.integers(0, 65536, (ch, cw), dtype=np.uint32).astype(np.uint16)
        frames.append(([y], c))
    return frames


_big = lambda p: hr._GEOM[p.ctypes.data][0]


@pytest.mark.parametrize("shift", [(-1, -1), (-1, 0)], ids=["420", "422"])
@pytest.mark.parametrize("size", [(1, 1), (2, 1), (1, 2), (3, 3), (5, 4), (8, 8), (33, 17), (130, 66), (1030, 5)], ids=lambda s: "%dx%d" % s)
def test_fused_apply_is_the_luma_launch_then_the_chroma_launch(size, shift):
    mw, mh = size
    rng = np.random.default_rng(1000 * mw + mh)
    for offset in (0, 1):                                   # 1: every output plane one element off its alignment - the two-launch fallback
        (y0, c0), (y1, c1) = _yuv_planes(mw, mh, shift, rng, offset)
        for dt in (np.float32, np.float16):
            for mask_off in (0, 1):
                for maxval in (4095, 65535):
                    for kind in ("zero", "shift", "random"):
                        flow, mask = _motion(kind, mw, mh, dt, mask_off, rng)
                        wy, wc = hr.blank_like(y0), hr.blank_like(c0)
                        amd.op_apply(y0, y1, flow, mask, wy, maxval)
                        amd.op_apply_scaled(c0, c1, flow, mask, wc, shift, maxval)
                        gy, gc = hr.blank_like(y0), hr.blank_like(c0)
                        fused = amd.op_apply_yuv(y0, y1, c0, c1, flow, mask, gy, gc, shift, maxval)
                        what = "%dx%d %s off %d %s mask_off %d maxval %d %s" % (mw, mh, shift, offset, np.dtype(dt).name, mask_off, maxval, kind)
                        assert fused == (mw >= 4 and offset == 0), what + ": fused %s" % fused
                        for g, w_ in zip(gy + gc, wy + wc):
                            assert np.array_equal(_big(g), _big(w_)), what + ": %d samples differ" % int((_big(g) != _big(w_)).sum())      # row padding included
                            assert hr.untouched(g), what + ": sentinel bytes changed"
                        if kind == "random" and mw * mh > 64:
                            assert (gy[0] != np.minimum(y0[0], maxval)).any(), "a case without motion checks nothing"


def test_fused_apply_refusals():
    rng = np.random.default_rng(3)
    (y0, c0), (y1, c1) = _yuv_planes(16, 8, (-1, -1), rng)
    flow, mask = _motion("zero", 16, 8, np.float32, 0, rng)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*a luma set of shift \(0, 0\) and a chroma set of shift"):
        amd.op_apply_yuv(y0, y1, y0, y1, flow, mask, hr.blank_like(y0), hr.blank_like(y0), (0, 0))
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*set 1: the plane size"):
        amd.op_apply_yuv(y0, y1, c0, c1, flow, mask, hr.blank_like(y0), hr.blank_like(c0), (-1, 0))


# ---- B: the call -------------------------------------------------------------------------------------------------------------------------------------------------------
def _engine(modeldirs, scale=1, precision="full"):
    key = (scale, precision)
    if key not in _ENG:
        g = pkg.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
        if scale == 2:
            g.set_flow_scale(2)
        g.set_precision(precision)
        _ENG[key] = g
    return _ENG[key]


def _same(got, want, what):
    for k in range(3):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: plane %d differs in %d samples" % (what, k, int((got[k] != want[k]).sum()))


class _Dev:
    """planes of hbd_ref.planes() / blank_like() in device memory with their geometry: the whole (rows, pitch) array goes up, the descriptor names the plane inside it"""

    def __init__(self, ps, w, h, pixfmt):
        import torch
        self.ps = ps
        self.t = [torch.from_numpy(hr._GEOM[p.ctypes.data][0].view(np.int16)).cuda() for p in ps]
        self.off = [hr._GEOM[p.ctypes.data][1] for p in ps]
        self.img = pkg.device_image(w, h, pixfmt, [(t.data_ptr() + 2 * o, t.stride(0) * 2) for t, o in zip(self.t, self.off)])

    def planes(self):
        """the planes as host arrays; the arrays behind `ps` take everything that came back, so hbd_ref.untouched() speaks about the device bytes"""
        out = []
        for p, t, o in zip(self.ps, self.t, self.off):
            big = hr._GEOM[p.ctypes.data][0]
            big[...] = t.cpu().numpy().view(np.uint16)
            out.append(big[:, o:o + p.shape[1]])
        return out


def _host_and_device(g, p0, p1, t, depth, pixfmt, what, stream=False):
    import torch
    h, w = p0[0].shape
    want = hr.expected(g, p0, p1, t, depth, pixfmt)
    out = hr.blank_like(p0)
    got = g.process_hbd(tuple(p0), tuple(p1), t, depth, pixfmt, out=tuple(out))
    _same(got, want, what + " host")
    assert all(hr.untouched(o) for o in out), what + " host: bytes around the output planes changed"
    d0, d1, do = _Dev(p0, w, h, pixfmt), _Dev(p1, w, h, pixfmt), _Dev(hr.blank_like(p0), w, h, pixfmt)
    st = torch.cuda.Stream() if stream else None
    torch.cuda.synchronize()
    g.process_device_hbd(d0.img, d1.img, t, do.img, depth, stream=st.cuda_stream if st else None)
    torch.cuda.synchronize()
    dgot = do.planes()
    _same(dgot, want, what + " device")
    assert all(hr.untouched(o) for o in dgot), what + " device: bytes around the output planes changed"
    return want


def _device_composition(g, p0, p1, t, depth, pixfmt):
    """rife_hip_process_device_apply_sets on device proxies and device planes: the device form of the definition"""
    import torch
    h, w = p0[0].shape
    maxval = (1 << depth) - 1
    f0 = torch.from_numpy(hr.proxy_frame(p0, depth).view(np.int16)).cuda(); f1 = torch.from_numpy(hr.proxy_frame(p1, depth).view(np.int16)).cuda()
    fo = torch.zeros_like(f0)
    d0, d1, do = _Dev(p0, w, h, pixfmt), _Dev(p1, w, h, pixfmt), _Dev(hr.blank_like(p0), w, h, pixfmt)

    def desc(d, first, n):
        return pkg.planes_desc(d.ps[first].shape[1], d.ps[first].shape[0], pkg.SAMPLE_U16, [(d.img.plane[k], d.img.pitch[k]) for k in range(first, first + n)], maxval)

    if (pixfmt & 0xff) in hr.SHIFT:
        sets = [pkg.apply_set_desc(desc(d0, 0, 1), desc(d1, 0, 1), desc(do, 0, 1), (0, 0)), pkg.apply_set_desc(desc(d0, 1, 2), desc(d1, 1, 2), desc(do, 1, 2), hr.SHIFT[pixfmt & 0xff])]
    else:
        sets = [pkg.apply_set_desc(desc(d0, 0, 3), desc(d1, 0, 3), desc(do, 0, 3), (0, 0))]
    torch.cuda.synchronize()
    g.process_device_apply_sets(f0.data_ptr(), f1.data_ptr(), w, h, t, fo.data_ptr(), sets, pixfmt=pixfmt)
    torch.cuda.synchronize()
    return do.planes()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("pixfmt", hr.BASES, ids=_fid)
def test_hbd_calls_are_reduce10_then_the_sets_calls(pixfmt, depth, modeldirs):
    g = _engine(modeldirs)
    px = pixfmt | _csps(pixfmt)[-1 if depth == 12 else 0]
    for i, (w, h) in enumerate(((1, 1), (2, 2), (17, 9), (96, 64), (100, 60), (256, 192))):
        p0, p1 = hr.planes(w, h, px, depth, 100 * depth + i)
        want = _host_and_device(g, p0, p1, 0.37, depth, px, "%s depth %d %dx%d tight" % (hr.NAME[pixfmt], depth, w, h), stream=(i % 2 == 1))
        if (w, h) == (100, 60):
            _same(_device_composition(g, p0, p1, 0.37, depth, px), want, "the device composition")
            assert any((want[k] != np.minimum(p0[k], (1 << depth) - 1)).any() for k in range(3)), "a case without motion checks nothing"
    # row-padded planes; planes one element off their alignment with odd pitches (every launch takes its scalar form); all four timesteps
    for pad, off in ((8, 0), (3, 1)):
        p0, p1 = hr.planes(96, 64, px, depth, 7 + depth, pitch_pad=pad, offset=off)
        for t in (0.0, 0.37, 0.5, 1.0):
            want = _host_and_device(g, p0, p1, t, depth, px, "%s depth %d 96x64 pad %d off %d t %s" % (hr.NAME[pixfmt], depth, pad, off, t))
            if t in (0.0, 1.0):      # planes copied and clamped to maxval
                _same(want, [np.minimum(p, (1 << depth) - 1) for p in (p0 if t == 0.0 else p1)], "timestep %s" % t)


@pytest.mark.parametrize("scale,precision", [(2, "full"), (1, "fast"), (2, "fast")])
@pytest.mark.parametrize("pixfmt", hr.BASES, ids=_fid)
def test_hbd_calls_at_flow_scale_2_and_fast_precision(pixfmt, scale, precision, modeldirs):
    g = _engine(modeldirs, scale, precision)
    full = _engine(modeldirs)
    p0, p1 = hr.planes(100, 60, pixfmt, 12, 31, pitch_pad=4)
    want = _host_and_device(g, p0, p1, 0.5, 12, pixfmt, "%s scale %d %s" % (hr.NAME[pixfmt], scale, precision))
    if scale == 2:
        assert any((want[k] != hr.expected(full, p0, p1, 0.5, 12, pixfmt)[k]).any() for k in range(3)), "flow scale 2 gave the planes of flow scale 1: the engine setting was not in force"


def _apply_classes(g, p0, p1, depth, pixfmt, device=False):
    """the profiler's apply classes of one hbd call; device: on the planes where they lie, with their pitch and alignment (the host call stages them tight)"""
    import torch
    h, w = p0[0].shape
    if device:
        d0, d1, do = _Dev(p0, w, h, pixfmt), _Dev(p1, w, h, pixfmt), _Dev(hr.blank_like(p0), w, h, pixfmt)
        torch.cuda.synchronize()
    g.profile_enable(True)
    if device:
        g.process_device_hbd(d0.img, d1.img, 0.5, do.img, depth)
    else:
        g.process_hbd(tuple(p0), tuple(p1), 0.5, depth, pixfmt)
    prof = g.profile_read()
    g.profile_enable(False)
    return sorted(k for k, v in prof.items() if k.startswith("apply") and v["launches"])


@pytest.mark.parametrize("pixfmt", [pkg.PIX_I420P10, pkg.PIX_I422P10], ids=_fid)
def test_fused_launch_where_aligned_two_launches_elsewhere_and_with_the_switch_off(pixfmt, modeldirs, monkeypatch):
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])      # the test build reads RIFE_HIP_APPLY_YUV, per call
    p0, p1 = hr.planes(100, 60, pixfmt, 12, 41, pitch_pad=4)
    q0, q1 = hr.planes(100, 60, pixfmt, 12, 41, pitch_pad=3, offset=1)
    monkeypatch.delenv("RIFE_HIP_APPLY_YUV", raising=False)
    fused = _host_and_device(g, p0, p1, 0.5, 12, pixfmt, "fused")
    assert _apply_classes(g, p0, p1, 12, pixfmt) == ["apply_yuv"] and _apply_classes(g, p0, p1, 12, pixfmt, device=True) == ["apply_yuv"]
    assert _apply_classes(g, q0, q1, 12, pixfmt, device=True) == ["apply_motion", "apply_motion_down"], "misaligned device planes must take the two launches"
    assert _apply_classes(g, q0, q1, 12, pixfmt) == ["apply_yuv"], "host planes are staged tight: their own alignment does not matter"
    _host_and_device(g, q0, q1, 0.5, 12, pixfmt, "misaligned")
    monkeypatch.setenv("RIFE_HIP_APPLY_YUV", "0")
    assert _apply_classes(g, p0, p1, 12, pixfmt) == ["apply_motion", "apply_motion_down"]
    _same(_host_and_device(g, p0, p1, 0.5, 12, pixfmt, "switch off"), fused, "the switch changed the planes")
    assert _apply_classes(_engine(modeldirs), p0, p1, 12, pixfmt) == ["apply_yuv"], "the product ignores the switch"


# ---- C: refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw,word", [("rife-v2.3", {}, "rife-v2"), ("rife-v4", {}, "rife-v4 (4.0)"), ("rife-v4.6", dict(tta_mode=True), "TTA mode (-x)"),
                                         ("rife-v4.6", dict(tta_temporal_mode=True), "temporal TTA mode (-z)"), ("rife-v4.6", dict(uhd_mode=True), "UHD mode (-u)")])
def test_other_families_and_modes_are_refused_by_name(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = pkg.RIFE(0, **fl); e.load(modeldirs[fam])
    for pixfmt in (pkg.PIX_I420P10, pkg.PIX_RGBP10):
        p0, p1 = hr.planes(64, 64, pixfmt, 12, 3, pitch_pad=2)
        for t in (0.5, 0.0):
            out = hr.blank_like(p0)
            with pytest.raises(pkg.RifeError) as ex:
                e.process_hbd(tuple(p0), tuple(p1), t, 12, pixfmt, out=tuple(out))
            assert "(-6)" in str(ex.value) and word in str(ex.value) and "high bit depth" in str(ex.value), str(ex.value)
            assert all((o == hr.SENTINEL).all() and hr.untouched(o) for o in out), "a refused call wrote into an output plane"
            d0, d1, do = _Dev(p0, 64, 64, pixfmt), _Dev(p1, 64, 64, pixfmt), _Dev(hr.blank_like(p0), 64, 64, pixfmt)
            torch.cuda.synchronize()
            with pytest.raises(pkg.RifeError) as ex:
                e.process_device_hbd(d0.img, d1.img, t, do.img, 12)
            assert "(-6)" in str(ex.value) and word in str(ex.value) and "high bit depth" in str(ex.value), str(ex.value)
            torch.cuda.synchronize()
            assert all((o == hr.SENTINEL).all() and hr.untouched(o) for o in do.planes())


def test_bad_arguments_and_an_unloaded_engine(modeldirs):
    g = _engine(modeldirs)
    p0, p1 = hr.planes(32, 16, pkg.PIX_I422P10, 12, 9)
    out = hr.blank_like(p0)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*image 0: the depth \(17\) is not in 10\.\.16"):
        g.process_hbd(tuple(p0), tuple(p1), 0.5, 17, pkg.PIX_I422P10, out=tuple(out))
    q0, _ = hr.planes(34, 16, pkg.PIX_I422P10, 12, 9)
    a, b, o = (pkg.planes_image(tuple(x), x[0].shape[1], 16, pkg.PIX_I422P10) for x in (p0, q0, out))
    assert g._L.rife_hip_process_hbd(g._h, ctypes.byref(a), ctypes.byref(b), 0.5, ctypes.byref(o), 12) == -pkg.EINVAL
    assert "the images of one call differ in size" in g._L.rife_hip_last_error().decode()
    bare = pkg.RIFE(0, rife_v4=True)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*before load"):
        bare.process_hbd(tuple(p0), tuple(p1), 0.5, 12, pkg.PIX_I422P10, out=tuple(out))
    assert all((x == hr.SENTINEL).all() for x in out)
