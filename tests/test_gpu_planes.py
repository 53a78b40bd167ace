"""Strided frames and separate planes (include/rife_hip.h rife_hip_image_t) through the rife-v4.6 engine, on the GPU.

The contract, checked in its words: an image call is byte for byte the _px call on the same samples repacked tight, with the result unpacked into `out`; it writes
the first row-bytes bytes of each row of each output plane and nothing else (tests/planes_ref.py surrounds every window with canaries).
  1  the pitched kernels alone (csrc/planes.h) against the tight kernels of the _px path on the repacked frame, exact, both forms
  2  the device image call against the _px call, on a caller stream and on the NULL stream
  3  timestep 0 / 1: the canonical samples
  4  the host path: process_image, frame_upload_image + process_frames_image, the Python mirror
  5  refusals"""
import ctypes
import importlib

import numpy as np
import pytest

import deep_ref
import planes_ref as pr
import yuv_ref as yr
from tools import gen_frames

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
RGB8, RGB10, PACKED, RGBA8 = amd.PIX_RGB8, amd.PIX_RGB10_U16, amd.PIX_A2B10G10R10, amd.PIX_RGBA8
NV12, I420, P010, I420P10 = amd.PIX_NV12, amd.PIX_I420, amd.PIX_P010, amd.PIX_I420P10
KERNEL_SIZES = [(1, 1), (2, 2), (3, 5), (8, 6), (33, 47), (64, 34), (72, 40)]


def _id(px):
    return pr.FMT_NAME[px & 0xff]


@pytest.fixture(scope="module")
def engine(modeldirs):
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    return g


# ---- frames, as the tight BYTES of the _px calls ------------------------------------------------------------------------------------------------

_SCENES = {}
_PX = {}


def pair_bytes(w, h, px, seed=60):
    """Two frames of one moving 10-bit scene (tests/deep_ref.py) in format px, as uint8 arrays of frame_bytes(w, h, px) bytes."""
    key = (w, h, seed)
    if key not in _SCENES:
        _SCENES[key] = deep_ref.deep_pair_uncached(w, h, seed + w)
    out = []
    for i, c10 in enumerate(_SCENES[key]):
        b = px & 0xff
        if b == RGB8:
            f = deep_ref.to_depth8(c10).astype(np.uint8)
        elif b == RGB10:
            f = c10.astype(np.uint16)
        elif b == PACKED:
            f = amd.pack_a2b10g10r10(c10)
        elif b == RGBA8:
            alpha = np.random.default_rng(seed + i).integers(0, 256, (h, w, 1), dtype=np.uint8)
            f = np.concatenate([deep_ref.to_depth8(c10).astype(np.uint8), alpha], axis=-1)
        else:
            f = yr.rgb10_to_yuv(c10, px)
            if b == P010:
                f = f | np.uint16(0x2a >> i)                 # low bits set on input: ignored, and cleared on output
        out.append(np.frombuffer(np.ascontiguousarray(f).tobytes(), np.uint8).copy())
    return out


def px_call(g, a, b, w, h, t, px):
    """The _px call on tight frames (bytes in, bytes out); computed once per case and shared."""
    key = (a.tobytes(), b.tobytes(), w, h, t, px)
    if key not in _PX:
        out = np.full(a.size, 0x5a, np.uint8)
        rc = g._L.rife_hip_process_px(g._h, a.ctypes.data, b.ctypes.data, w, h, ctypes.c_float(t), out.ctypes.data, px)
        assert rc == 0, g._L.rife_hip_last_error().decode()
        _PX[key] = out
    return _PX[key]


def random_bytes(w, h, px, seed):
    return np.random.default_rng(seed).integers(0, 256, pr.frame_bytes(w, h, px), dtype=np.uint8)


class DeviceImage:
    """The buffers of a planes_ref.StridedImage in device memory, at the host buffers' alignment modulo 64."""

    def __init__(self, im):
        import torch
        self.im, self.t, self.off = im, [], []
        for buf in im.bufs:
            t = torch.empty(buf.size + 64, dtype=torch.uint8, device="cuda")
            off = (buf.ctypes.data - t.data_ptr()) % 64
            t[off:off + buf.size] = torch.from_numpy(buf)
            self.t.append(t); self.off.append(off)
        self.desc = im.rebased([t.data_ptr() + off for t, off in zip(self.t, self.off)])

    def fetch(self):
        """Copy the device buffers back into the StridedImage (canaries and all)."""
        for buf, t, off in zip(self.im.bufs, self.t, self.off):
            buf[:] = t[off:off + buf.size].cpu().numpy()
        return self.im


def expect_for(layout, tight_result, w, h, px):
    """What from_image() returns for a call whose tight result is tight_result: for `separate` the descriptor lists Cr before Cb (planes_ref.seen_by_call)."""
    return pr.swap_chroma(tight_result, w, h, px) if layout == "separate" else tight_result


# ---- 1. the kernels alone, exact -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_pitched_input_kernels_equal_the_tight_kernels(px):
    pxc = px | (amd.CSP_BT601 if pr.is_yuv(px) else 0)
    for (w, h) in KERNEL_SIZES:
        tight = random_bytes(w, h, px, 11 + w)
        for layout in pr.LAYOUTS:
            seen = pr.seen_by_call(tight, w, h, px, layout)
            want = amd.op_image_to_resident(pr.to_image(seen, w, h, pxc, "tight").desc, 2)      # the kernels of launch_preproc on the repacked frame
            im = pr.to_image(tight, w, h, pxc, layout)
            got = amd.op_image_to_resident(im.desc, 0)
            assert np.array_equal(got, want), "%s %dx%d %s: %d dwords differ" % (_id(px), w, h, layout, int((got != want).sum()))
            if layout == "a64" and w % 8 == 0:                                                   # the wide form ran above: the scalar form on the same planes
                assert np.array_equal(amd.op_image_to_resident(im.desc, 1), got), "%s %dx%d: the two forms differ" % (_id(px), w, h)
            assert im.canaries_intact() and np.array_equal(pr.from_image(im), tight)
        if pr.is_yuv(px):                                                                        # and the tight kernels are those of the YUV tests
            flat = tight.view(yr.dtype(px))
            assert np.array_equal(amd.op_image_to_resident(pr.to_image(tight, w, h, pxc, "tight").desc, 2), amd.op_yuv_to_rgb10(flat, w, h, pxc))


@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_pitched_output_kernels_equal_the_tight_kernels_and_keep_the_canaries(px):
    pxc = px | (amd.CSP_BT601 if pr.is_yuv(px) else 0)
    for (w, h) in KERNEL_SIZES:
        rng = np.random.default_rng(23 + h)
        if pr.is_yuv(px):
            src = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)                             # the alpha bits are ignored
            want = np.frombuffer(amd.op_rgb10_to_yuv(src, pxc).tobytes(), np.uint8)             # k_postproc_yuv on the tight frame
        else:
            src = random_bytes(w, h, px, 29 + w)                                                 # an RGB-format frame is stored as it is
            want = src
        for layout in pr.LAYOUTS:
            for force in ((0, 1) if (layout == "a64" and w % 8 == 0) else (0,)):
                im = pr.to_image(np.full(want.size, 0x3c, np.uint8), w, h, pxc, layout)
                amd.op_resident_to_image(src, im.desc, force)
                got = pr.from_image(im)
                exp = expect_for(layout, want, w, h, px)
                assert np.array_equal(got, exp), "%s %dx%d %s form %d: %d bytes differ" % (_id(px), w, h, layout, force, int((got != exp).sum()))
                assert im.canaries_intact(), "%s %dx%d %s form %d: bytes outside the windows were written" % (_id(px), w, h, layout, force)


# ---- 2. end to end: the device image call is the _px call ------------------------------------------------------------------------------------------

def device_call(g, a, b, w, h, t, px, layout, stream, layout_in=None):
    import torch
    ia, ib = DeviceImage(pr.to_image(a, w, h, px, layout_in or layout)), DeviceImage(pr.to_image(b, w, h, px, layout_in or layout))
    io = DeviceImage(pr.to_image(np.full(a.size, 0x3c, np.uint8), w, h, px, layout))
    torch.cuda.synchronize()
    g.process_device_image(ia.desc, ib.desc, t, io.desc, stream)
    torch.cuda.synchronize()
    for x, src in ((ia, a), (ib, b)):                                                           # the inputs are read only
        assert np.array_equal(pr.from_image(x.fetch()), src) and x.im.canaries_intact()
    return io.fetch()


@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_device_image_call_equals_the_px_call(engine, px):
    import torch
    g = engine
    pxc = px | (amd.CSP_BT601 if pr.is_yuv(px) else 0)
    user = torch.cuda.Stream()
    for (w, h) in [(33, 47), (64, 34)]:
        a, b = pair_bytes(w, h, pxc)
        for stream in (None, user.cuda_stream):
            for layout in ("elem", "a64", "window"):
                for t in (0.5, 0.3):
                    want = px_call(g, a, b, w, h, t, pxc)
                    im = device_call(g, a, b, w, h, t, pxc, layout, stream)
                    got = pr.from_image(im)
                    assert np.array_equal(got, want), "%s %dx%d %s t=%g stream %s: %d bytes differ" % (_id(px), w, h, layout, t, stream, int((got != want).sum()))
                    assert im.canaries_intact(), "%s %dx%d %s: bytes outside the windows were written" % (_id(px), w, h, layout)


@pytest.mark.parametrize("px", [RGB8, I420, P010], ids=_id)
def test_separate_allocations_in_yv12_order_and_mixed_pitches(engine, px):
    """Planes in allocations of their own, Cr before Cb: the call on the frame with its chroma planes exchanged.  Inputs and output of one call may have
    different pitches, and one engine serves calls of different pitches one after the other from one workspace."""
    g = engine
    w, h = 33, 47
    a, b = pair_bytes(w, h, px)
    want = px_call(g, pr.swap_chroma(a, w, h, px), pr.swap_chroma(b, w, h, px), w, h, 0.5, px)
    im = device_call(g, a, b, w, h, 0.5, px, "separate", None)
    assert np.array_equal(pr.from_image(im), pr.swap_chroma(want, w, h, px)) and im.canaries_intact()
    want = px_call(g, a, b, w, h, 0.5, px)
    first = pr.from_image(device_call(g, a, b, w, h, 0.5, px, "a64", None, layout_in="window"))
    second = pr.from_image(device_call(g, a, b, w, h, 0.5, px, "elem", None, layout_in="tight"))
    third = pr.from_image(device_call(g, a, b, w, h, 0.5, px, "a64", None, layout_in="window"))
    assert np.array_equal(first, want) and np.array_equal(second, want) and np.array_equal(third, want)
    a2, b2 = pair_bytes(64, 34, px)                                                             # another size in between: the workspace is rebuilt
    assert np.array_equal(pr.from_image(device_call(g, a2, b2, 64, 34, 0.5, px, "a64", None)), px_call(g, a2, b2, 64, 34, 0.5, px))
    assert np.array_equal(pr.from_image(device_call(g, a, b, w, h, 0.5, px, "window", None)), want)
    # an image whose planes are all tight IS the _px call
    tight = device_call(g, a, b, w, h, 0.5, px, "tight", None)
    assert np.array_equal(pr.from_image(tight), want)


# ---- 3. timestep 0 / 1 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_timestep_endpoints_return_the_canonical_samples(engine, px):
    g = engine
    w, h = 33, 47
    pxc = px | (amd.CSP_BT601 if pr.is_yuv(px) else 0)
    a, b = pair_bytes(w, h, pxc)
    if px in (RGB10, I420P10):
        a = a.copy(); a.view(np.uint16)[::7] = 0xffff                                           # samples above 1023: clamped on output
    if px == PACKED:
        a = a.copy(); a.view(np.uint32)[::5] &= np.uint32(0x3fffffff)                           # alpha bits clear on input: 3 on output
    for t, src in ((0.0, a), (1.0, b)):
        want = px_call(g, a, b, w, h, t, pxc)
        if pr.is_yuv(px):
            canon = np.frombuffer(yr.canonical(src.view(yr.dtype(px)), w, h, pxc).tobytes(), np.uint8)
            assert np.array_equal(want, canon)
            if px == P010:
                assert not (want.view(np.uint16) & 63).any() and (src.view(np.uint16) & 63).any()
        for layout in ("elem", "a64", "window"):
            im = device_call(g, a, b, w, h, t, pxc, layout, None)
            assert np.array_equal(pr.from_image(im), want), (_id(px), layout, t)
            assert im.canaries_intact()
            out = pr.to_image(np.full(a.size, 0x3c, np.uint8), w, h, pxc, layout)              # the host path
            _check_rc(g, g._L.rife_hip_process_image(g._h, ctypes.byref(pr.to_image(a, w, h, pxc, layout).desc), ctypes.byref(pr.to_image(b, w, h, pxc, "a64").desc),
                                                    ctypes.c_float(t), ctypes.byref(out.desc)))
            assert np.array_equal(pr.from_image(out), want) and out.canaries_intact()
    assert not np.array_equal(px_call(g, a, b, w, h, 0.0, pxc), px_call(g, a, b, w, h, 1.0, pxc))


def _check_rc(g, rc):
    assert rc == 0, (rc, g._L.rife_hip_last_error().decode())


# ---- 4. the host path --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", [RGB8, RGBA8, I420, P010], ids=_id)
@pytest.mark.parametrize("w,h", [(33, 47), (100, 60)])
def test_host_image_calls_equal_process_px(engine, px, w, h):
    g = engine
    L = g._L
    pxc = px | (amd.CSP_BT601 if pr.is_yuv(px) else 0)
    a, b = pair_bytes(w, h, pxc)
    for t in (0.5, 1.0):
        want = px_call(g, a, b, w, h, t, pxc)
        for layout in ("elem", "window"):
            ia, ib = pr.to_image(a, w, h, pxc, layout), pr.to_image(b, w, h, pxc, layout)
            out = pr.to_image(np.full(a.size, 0x3c, np.uint8), w, h, pxc, layout)
            _check_rc(g, L.rife_hip_process_image(g._h, ctypes.byref(ia.desc), ctypes.byref(ib.desc), ctypes.c_float(t), ctypes.byref(out.desc)))
            assert np.array_equal(pr.from_image(out), want), (_id(px), layout, t)
            assert out.canaries_intact() and ia.canaries_intact() and np.array_equal(pr.from_image(ia), a)
            # stream mode: upload the strided planes once, write a strided result
            f0, f1 = ctypes.c_void_p(), ctypes.c_void_p()
            _check_rc(g, L.rife_hip_frame_upload_image(g._h, ctypes.byref(ia.desc), ctypes.byref(f0)))
            _check_rc(g, L.rife_hip_frame_upload_image(g._h, ctypes.byref(ib.desc), ctypes.byref(f1)))
            out = pr.to_image(np.full(a.size, 0x3c, np.uint8), w, h, pxc, layout)
            _check_rc(g, L.rife_hip_process_frames_image(g._h, f0, f1, ctypes.c_float(t), ctypes.byref(out.desc)))
            assert np.array_equal(pr.from_image(out), want) and out.canaries_intact()
            tight = np.full(a.size, 0x3c, np.uint8)                                             # a frame of upload_image is a frame like any other
            _check_rc(g, L.rife_hip_process_frames(g._h, f0, f1, ctypes.c_float(t), tight.ctypes.data))
            assert np.array_equal(tight, want)
            L.rife_hip_frame_release(f0); L.rife_hip_frame_release(f1)


def test_python_mirror_takes_views_and_planes(engine):
    g = engine
    w, h = 33, 47
    a8, b8 = gen_frames.smooth_pair(120, 100, 3)
    big0, big1 = a8.copy(), b8.copy()
    va, vb = big0[3:3 + h, 5:5 + w], big1[3:3 + h, 5:5 + w]
    assert amd.image_of(va) is not None and not va.flags.c_contiguous
    want = g.process(np.ascontiguousarray(va), np.ascontiguousarray(vb), 0.5)
    assert np.array_equal(g.process(va, vb, 0.5), want)
    canvas = np.full((100, 120, 3), 0x3c, np.uint8)                                             # into a window of a larger picture
    g.process(va, vb, 0.5, outimage=canvas[10:10 + h, 20:20 + w])
    assert np.array_equal(canvas[10:10 + h, 20:20 + w], want)
    canvas[10:10 + h, 20:20 + w] = 0x3c
    assert (canvas == 0x3c).all()
    assert np.array_equal(big0, a8) and np.array_equal(big1, b8)
    f0, f1 = g.upload(va), g.upload(vb)
    assert np.array_equal(g.process_frames(f0, f1, 0.5), want)
    f0.release(); f1.release()
    assert np.array_equal(g.process(big0[:, ::2], big1[:, ::2], 0.5), g.process(np.ascontiguousarray(big0[:, ::2]), np.ascontiguousarray(big1[:, ::2]), 0.5))      # today's path
    # three separately allocated plane arrays with rows padded to 64 bytes == process_yuv on the packed frame
    px = I420 | amd.CSP_BT601
    a, b = pair_bytes(w, h, px)
    want = g.process_yuv(a, b, w, h, 0.5, px)
    cw, ch = yr.chroma_dims(w, h)

    def planes(flat):
        out = []
        for (rows, rb, off, _) in pr.plane_table(w, h, px):
            p = np.full((rows, 64), 0x3c, np.uint8)[:, :rb]
            p[:] = flat[off:off + rows * rb].reshape(rows, rb)
            out.append(p)
        return tuple(out)
    got = g.process_planes(planes(a), planes(b), 0.5, px)
    assert [p.shape for p in got] == [(h, w), (ch, cw), (ch, cw)]
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in got]), want)
    outp = planes(np.zeros_like(a))
    g.process_planes(planes(a), planes(b), 0.5, px, out=outp)
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in outp]), want)
    assert all((p.base[:, p.shape[1]:] == 0x3c).all() for p in outp)                            # the row padding keeps its bytes
    f0, f1 = g.upload_planes(planes(a), px), g.upload_planes(planes(b), px)
    assert np.array_equal(g.process_frames(f0, f1, 0.5), want)
    f0.release(); f1.release()


@pytest.mark.parametrize("fam,kw", [("rife-v2.3", {}), ("rife-v4.6", dict(tta_mode=True))])
def test_views_on_engines_without_strided_images_take_the_contiguous_copy_as_before(modeldirs, fam, kw):
    """process() / upload() on a cropped view worked on every family and mode before images existed (through a contiguous copy) and still does: where the
    engine refuses strided images the mirror falls back, and the result is that of the contiguous copy."""
    g = amd.RIFE(0, rife_v2=fam.startswith("rife-v2"), rife_v4=fam.startswith("rife-v4"), **kw); g.load(modeldirs[fam])
    w, h = 64, 64
    a8, b8 = gen_frames.smooth_pair(120, 100, 5)
    va, vb = a8[3:3 + h, 5:5 + w], b8[3:3 + h, 5:5 + w]
    assert amd.image_of(va) is not None and not va.flags.c_contiguous
    want = g.process(np.ascontiguousarray(va), np.ascontiguousarray(vb), 0.5)
    assert want.any() and np.array_equal(g.process(va, vb, 0.5), want)
    assert np.array_equal(g.process(va, vb, 0.0), va) and np.array_equal(g.process(va, vb, 1.0), vb)
    f0, f1 = g.upload(va), g.upload(vb)
    assert np.array_equal(g.process_frames(f0, f1, 0.5), want)
    f0.release(); f1.release()
    with pytest.raises(ValueError):                                                             # a strided outimage was never taken there, and is not now
        g.process(va, vb, 0.5, outimage=np.zeros((100, 120, 3), np.uint8)[3:3 + h, 5:5 + w])
    d16 = np.zeros((100, 120, 3), np.uint16)[3:3 + h, 5:5 + w]                                   # a 10-bit view: the refusal of the _px call, as before
    with pytest.raises(amd.RifeError) as e:
        g.process(d16, d16, 0.5)
    assert "(-6)" in str(e.value) and "10-bit" in str(e.value)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------

def test_images_that_disagree_are_einval(engine):
    g = engine
    L = g._L
    a, b = pair_bytes(33, 47, RGB8)
    ia, ib = pr.to_image(a, 33, 47, RGB8, "a64"), pr.to_image(b, 33, 47, RGB8, "a64")
    out = pr.to_image(np.full(a.size, 0x3c, np.uint8), 33, 47, RGB8, "a64")
    narrow = pr.to_image(a[:32 * 47 * 3], 32, 47, RGB8, "a64")
    rgba = pr.to_image(np.zeros(33 * 47 * 4, np.uint8), 33, 47, RGBA8, "a64")
    di, dn, dr, do = DeviceImage(ia), DeviceImage(narrow), DeviceImage(rgba), DeviceImage(out)
    for (x, y, z) in [(narrow, ib, out), (ia, narrow, out), (ia, ib, narrow), (rgba, ib, out), (ia, ib, rgba)]:
        assert L.rife_hip_process_image(g._h, ctypes.byref(x.desc), ctypes.byref(y.desc), ctypes.c_float(0.5), ctypes.byref(z.desc)) == -1
        assert "differ" in L.rife_hip_last_error().decode()
    for (x, y, z) in [(dn, di, do), (di, di, dn), (dr, di, do), (di, di, dr)]:
        assert L.rife_hip_process_device_image(g._h, ctypes.byref(x.desc), ctypes.byref(y.desc), ctypes.c_float(0.5), ctypes.byref(z.desc), None) == -1
        assert "differ" in L.rife_hip_last_error().decode()
    bad = pr.to_image(a, 33, 47, RGB8, "a64"); bad.desc.pitch[0] = 98
    assert L.rife_hip_process_image(g._h, ctypes.byref(bad.desc), ctypes.byref(ib.desc), ctypes.c_float(0.5), ctypes.byref(out.desc)) == -1
    assert "smaller than the row bytes" in L.rife_hip_last_error().decode()
    f0 = ctypes.c_void_p()
    assert L.rife_hip_frame_upload_image(g._h, ctypes.byref(bad.desc), ctypes.byref(f0)) == -1 and not f0.value
    fa, fb = g.upload(a.reshape(47, 33, 3)), g.upload(b.reshape(47, 33, 3))
    assert L.rife_hip_process_frames_image(g._h, fa._f, fb._f, ctypes.c_float(0.5), ctypes.byref(narrow.desc)) == -1
    assert L.rife_hip_process_frames_image(g._h, fa._f, fb._f, ctypes.c_float(0.5), ctypes.byref(rgba.desc)) == -1
    fa.release(); fb.release()
    assert out.canaries_intact() and (pr.from_image(out) == 0x3c).all() and (pr.from_image(do.fetch()) == 0x3c).all()


@pytest.mark.parametrize("fam,kw,word", [("rife-v2.3", {}, "rife-v2"), ("rife-v4.6", dict(tta_mode=True), "TTA")])
def test_strided_images_on_other_families_and_modes_are_enosys(modeldirs, fam, kw, word):
    import torch
    g = amd.RIFE(0, rife_v2=fam.startswith("rife-v2"), rife_v4=fam.startswith("rife-v4"), **kw); g.load(modeldirs[fam])
    L = g._L
    w, h = 64, 64
    a, b = pair_bytes(w, h, RGB8)
    for t in (0.5, 0.0):
        ia, ib, out = pr.to_image(a, w, h, RGB8, "elem"), pr.to_image(b, w, h, RGB8, "elem"), pr.to_image(np.full(a.size, 0x3c, np.uint8), w, h, RGB8, "elem")
        assert L.rife_hip_process_image(g._h, ctypes.byref(ia.desc), ctypes.byref(ib.desc), ctypes.c_float(t), ctypes.byref(out.desc)) == -6
        msg = L.rife_hip_last_error().decode()
        assert word in msg and "strided" in msg, msg
        assert (pr.from_image(out) == 0x3c).all() and out.canaries_intact()
        da, db, do = DeviceImage(ia), DeviceImage(ib), DeviceImage(out)
        torch.cuda.synchronize()
        assert L.rife_hip_process_device_image(g._h, ctypes.byref(da.desc), ctypes.byref(db.desc), ctypes.c_float(t), ctypes.byref(do.desc), None) == -6
        assert word in L.rife_hip_last_error().decode()
        torch.cuda.synchronize()
        assert (pr.from_image(do.fetch()) == 0x3c).all() and out.canaries_intact()
    f = ctypes.c_void_p()
    assert L.rife_hip_frame_upload_image(g._h, ctypes.byref(ia.desc), ctypes.byref(f)) == -6 and not f.value
    if fam == "rife-v2.3":
        # a TIGHT RGB8 image is rife_hip_process_device, served wherever that is
        import torch
        ta, tb, to = DeviceImage(pr.to_image(a, w, h, RGB8, "tight")), DeviceImage(pr.to_image(b, w, h, RGB8, "tight")), DeviceImage(pr.to_image(np.zeros_like(a), w, h, RGB8, "tight"))
        ref = torch.zeros(a.size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.process_device(ta.desc.plane[0], tb.desc.plane[0], w, h, 0.5, ref.data_ptr(), None)
        g.process_device_image(ta.desc, tb.desc, 0.5, to.desc, None)
        torch.cuda.synchronize()
        assert np.array_equal(pr.from_image(to.fetch()), ref.cpu().numpy()) and ref.any().item()
        host = pr.to_image(np.zeros_like(a), w, h, RGB8, "tight")
        _check_rc(g, L.rife_hip_process_image(g._h, ctypes.byref(pr.to_image(a, w, h, RGB8, "tight").desc), ctypes.byref(pr.to_image(b, w, h, RGB8, "tight").desc),
                                                ctypes.c_float(0.5), ctypes.byref(host.desc)))
        assert np.array_equal(pr.from_image(host), ref.cpu().numpy())
