"""4:2:0 Y'CbCr frames (RIFE_HIP_PIX_NV12 / I420 / P010 / I420P10, include/rife_hip.h "video") through the rife-v4.6 engine, on the GPU.

What the header states, checked in its words: the two kernels equal tests/yuv_ref.py bit for bit; a YUV call is byte for byte
rgb10_to_yuv(process(yuv_to_rgb10(a), yuv_to_rgb10(b), t)) through every entry point; against the reference network at most 1 code per sample (the depth-10
bound times the sensitivity pinned in tests/test_yuv_host.py); timestep 0 / 1 return the inputs; everything out of scope is refused before anything is written."""
import ctypes
import importlib

import numpy as np
import pytest

import deep_ref
import yuv_ref as yr
from oracle import pyoracle
from tools import gen_frames

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
NV12, I420, P010, I420P10 = amd.PIX_NV12, amd.PIX_I420, amd.PIX_P010, amd.PIX_I420P10
FMT_IDS = {NV12: "nv12", I420: "i420", P010: "p010", I420P10: "i420p10"}
SIZES = [(1, 1), (2, 2), (3, 5), (31, 33), (33, 47), (100, 60), (256, 192), (640, 360)]
# all four formats at matrix 709, each matrix on NV12, both ranges at 8 bits
KERNEL_CASES = [NV12, I420, P010, I420P10, NV12 | amd.CSP_BT601, NV12 | amd.CSP_BT2020NCL, NV12 | amd.CSP_FULL, I420 | amd.CSP_FULL | amd.CSP_BT601]


def _id(px):
    return "%s-%s-%s" % (FMT_IDS[px & 0xff], {0: "709", 1: "601", 2: "2020"}[(px >> 8) & 15], "full" if px & amd.CSP_FULL else "limited")


@pytest.fixture(scope="module")
def engines(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    return g, o


_SCENES = {}


def scene(w, h, px, seed=40):
    """Two YUV frames of one moving 10-bit scene (tests/deep_ref.py), in format px; the RGB scene is shared by the formats."""
    key = (w, h, seed)
    if key not in _SCENES:
        _SCENES[key] = deep_ref.deep_pair_uncached(w, h, seed + w)
    a, b = _SCENES[key]
    return yr.rgb10_to_yuv(a, px), yr.rgb10_to_yuv(b, px)


def random_frame(w, h, px, seed):
    """Random samples over the whole code range of every plane: most of them out of gamut (P010: with random low bits, which are ignored)."""
    rng = np.random.default_rng(seed)
    n = yr.frame_elems(w, h)
    if yr.depth(px) == 8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if (px & 0xff) == P010:
        return rng.integers(0, 65536, n, dtype=np.uint16)
    return rng.integers(0, 1024, n, dtype=np.uint16)


def unpack_padded(d):
    return np.stack([d & 1023, (d >> 10) & 1023, (d >> 20) & 1023], axis=-1).astype(np.uint16)


def composed(g, a, b, w, h, t, px):
    """The header's composition through the A2B10G10R10 call."""
    mid = g.process(amd.pack_a2b10g10r10(yr.yuv_to_rgb10(a, w, h, px)), amd.pack_a2b10g10r10(yr.yuv_to_rgb10(b, w, h, px)), t)
    return yr.rgb10_to_yuv(amd.unpack_a2b10g10r10(mid), px)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ---- 1. the kernels alone, exact ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", KERNEL_CASES, ids=_id)
def test_kernels_alone_equal_the_specification(px):
    for (w, h) in SIZES:                                     # 256x192 and 640x360: the x8 forms (w % 8 == 0); every other size: the scalar forms
        f = random_frame(w, h, px, 5 + w)
        got = amd.op_yuv_to_rgb10(f, w, h, px)
        want = yr.yuv_to_rgb10(f, w, h, px)
        assert np.array_equal(unpack_padded(got[:h, :w]), want), "in %s %dx%d: %d pixels differ" % (_id(px), w, h, int((unpack_padded(got[:h, :w]) != want).any(axis=-1).sum()))
        assert not got[h:].any() and not got[:, w:].any(), "padding of %dx%d is not zero RGB" % (w, h)
        assert not (got >> 30).any()
        rng = np.random.default_rng(9 + h)
        rgb = rng.integers(0, 1024, (h, w, 3), dtype=np.uint16)
        packed = amd.pack_a2b10g10r10(rgb) & np.uint32(0x3fffffff) | (rng.integers(0, 4, (h, w), dtype=np.uint32) << 30)      # the alpha bits are ignored
        back = amd.op_rgb10_to_yuv(packed, px)
        assert np.array_equal(back, yr.rgb10_to_yuv(rgb, px)), "out %s %dx%d: %d samples differ" % (_id(px), w, h, int((back != yr.rgb10_to_yuv(rgb, px)).sum()))


@pytest.mark.parametrize("px", [NV12, I420, P010, I420P10], ids=_id)
def test_odd_heights_on_the_x8_forms(px):
    """w % 8 == 0 with an odd height: the last chroma row averages two pixels, and the last luma row has no partner."""
    for (w, h) in [(8, 1), (64, 33), (40, 7)]:
        f = random_frame(w, h, px, 77)
        assert np.array_equal(unpack_padded(amd.op_yuv_to_rgb10(f, w, h, px)[:h, :w]), yr.yuv_to_rgb10(f, w, h, px))
        rgb = np.random.default_rng(3).integers(0, 1024, (h, w, 3), dtype=np.uint16)
        assert np.array_equal(amd.op_rgb10_to_yuv(amd.pack_a2b10g10r10(rgb), px), yr.rgb10_to_yuv(rgb, px))


@pytest.mark.parametrize("px", [NV12, I420, P010, I420P10], ids=_id)
def test_device_frames_one_element_off_alignment(engines, px):
    """A w % 8 == 0 frame whose device pointers are offset by one element takes the scalar kernels: same bytes as the aligned call."""
    import torch
    g, _ = engines
    w, h = 256, 192
    a, b = scene(w, h, px)
    want = g.process_yuv(a, b, w, h, 0.5, px)
    esz = a.dtype.itemsize
    n = a.size * esz
    b0 = torch.zeros(n + 32, dtype=torch.uint8, device="cuda"); b1 = torch.zeros(n + 32, dtype=torch.uint8, device="cuda"); out = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    b0[esz:esz + n] = _dev(a); b1[esz:esz + n] = _dev(b)
    torch.cuda.synchronize()
    g.process_device(b0.data_ptr() + esz, b1.data_ptr() + esz, w, h, 0.5, out.data_ptr() + esz, None, pixfmt=px)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out[esz:esz + n], want), want)
    assert not out[:esz].any().item() and not out[esz + n:].any().item(), "bytes outside the frame were written"


# ---- 2. the composition, exact, through every entry point ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES)
def test_a_yuv_call_is_the_packed_10_bit_call_converted(engines, w, h):
    g, _ = engines
    per_format = {}
    for px in (NV12, I420, P010, I420P10, NV12 | amd.CSP_BT601 | amd.CSP_FULL):
        a, b = scene(w, h, px)
        got = g.process_yuv(a, b, w, h, 0.4, px)
        assert got.dtype == a.dtype and got.shape == a.shape
        want = composed(g, a, b, w, h, 0.4, px)
        assert np.array_equal(got, want), "%s %dx%d: %d samples differ" % (_id(px), w, h, int((got != want).sum()))
        per_format[px] = yr.split(got, w, h, px)
    # the two layouts of one depth carry the same samples
    for p, q in ((NV12, I420), (P010, I420P10)):
        assert all(np.array_equal(x, y) for x, y in zip(per_format[p], per_format[q]))


@pytest.mark.parametrize("px", [NV12, I420P10], ids=_id)
@pytest.mark.parametrize("w,h", [(33, 47), (256, 192)])
def test_resident_batch_and_stream_mode_agree_with_the_host_call(engines, w, h, px):
    import torch
    g, _ = engines
    pairs = [scene(w, h, px, seed) for seed in (40, 41, 42)]
    ts = [0.5, 0.25, 0.7]
    want = [g.process_yuv(a, b, w, h, t, px) for (a, b), t in zip(pairs, ts)]
    for (a, b), t, x in zip(pairs[:1], ts, want):
        assert np.array_equal(x, composed(g, a, b, w, h, t, px))
    d0 = [_dev(a) for a, _ in pairs]; d1 = [_dev(b) for _, b in pairs]
    # process_device_px
    outs = [torch.zeros_like(x) for x in d0]
    torch.cuda.synchronize()
    for i in range(3):
        g.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], outs[i].data_ptr(), None, pixfmt=px)
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(_host(outs[i], want[i]), want[i]), "process_device pair %d" % i
    # process_device_batch_px: two pairs in lockstep plus one, on a caller stream and without one
    st = torch.cuda.Stream()
    for stream in (st.cuda_stream, None):
        outs = [torch.zeros_like(x) for x in d0]
        torch.cuda.synchronize()
        g.process_device_batch([x.data_ptr() for x in d0], [x.data_ptr() for x in d1], w, h, ts, [o.data_ptr() for o in outs], stream, pixfmt=px)
        torch.cuda.synchronize()
        for i in range(3):
            assert np.array_equal(_host(outs[i], want[i]), want[i]), "process_device_batch pair %d" % i
    # frame_upload_px + process_frames: a frame serves both sides and several timesteps
    f = [g.upload_yuv(pairs[0][0], w, h, px), g.upload_yuv(pairs[0][1], w, h, px)]
    for t in (0.5, 0.25):
        assert np.array_equal(g.process_frames(f[0], f[1], t), g.process_yuv(pairs[0][0], pairs[0][1], w, h, t, px))
    assert np.array_equal(g.process_frames(f[1], f[0], 0.5), g.process_yuv(pairs[0][1], pairs[0][0], w, h, 0.5, px))
    for x in f:
        x.release()


# ---- 3. against the reference network ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", [NV12, I420P10, P010 | amd.CSP_BT2020NCL, I420 | amd.CSP_FULL | amd.CSP_BT601], ids=_id)
@pytest.mark.parametrize("w,h", [(33, 47), (100, 60), (256, 192)])
def test_against_the_reference_network_within_one_code(engines, w, h, px):
    g, o = engines
    a, b = scene(w, h, px)
    t = 0.5
    got = g.process_yuv(a, b, w, h, t, px)
    want = yr.rgb10_to_yuv(deep_ref.expected_frame(o, yr.yuv_to_rgb10(a, w, h, px), yr.yuv_to_rgb10(b, w, h, px), t), px)
    sh = 6 if (px & 0xff) == P010 else 0
    d = np.abs((got.astype(np.int32) >> sh) - (want.astype(np.int32) >> sh))
    print("%s %dx%d: exact %.6f, off by one %.6f, max %d" % (_id(px), w, h, (d == 0).mean(), (d == 1).mean(), d.max()))
    assert d.max() <= 1


# ---- 4. timestep 0 / 1 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", [NV12, I420, P010, I420P10], ids=_id)
def test_timestep_endpoints_return_the_inputs(engines, px):
    import torch
    g, _ = engines
    w, h = 33, 47
    a, b = scene(w, h, px)
    if (px & 0xff) == P010:
        a = a | np.uint16(0x2a); b = b | np.uint16(0x15)              # low bits set on input: cleared on output
    ca, cb = yr.canonical(a, w, h, px), yr.canonical(b, w, h, px)
    if (px & 0xff) == P010:
        assert not np.array_equal(ca, a) and not (ca & 63).any()
    else:
        assert np.array_equal(ca, a)
    assert np.array_equal(g.process_yuv(a, b, w, h, 0.0, px), ca)
    assert np.array_equal(g.process_yuv(a, b, w, h, 1.0, px), cb)
    d0, d1 = _dev(a), _dev(b); out = torch.zeros_like(d0)
    torch.cuda.synchronize()
    g.process_device(d0.data_ptr(), d1.data_ptr(), w, h, 1.0, out.data_ptr(), None, pixfmt=px)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out, cb), cb)
    g.process_device_batch([d0.data_ptr()], [d1.data_ptr()], w, h, [0.0], [out.data_ptr()], None, pixfmt=px)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out, ca), ca)
    f0, f1 = g.upload_yuv(a, w, h, px), g.upload_yuv(b, w, h, px)
    assert np.array_equal(g.process_frames(f0, f1, 0.0), ca) and np.array_equal(g.process_frames(f0, f1, 1.0), cb)
    f0.release(); f1.release()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife", {}, "v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal"),
                                         ("rife-v4.6", dict(uhd_mode=True), "UHD")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    g = amd.RIFE(0, **fl); g.load(modeldirs[fam])
    w, h = 64, 64
    for px in (NV12, I420P10):
        a, b = scene(w, h, px)
        out = np.full_like(a, 0x5a)
        keep = out.copy()
        for t in (0.5, 0.0):
            with pytest.raises(amd.RifeError) as e:
                g.process_yuv(a, b, w, h, t, px, out=out)
            assert "(-6)" in str(e.value) and word in str(e.value) and "YUV" in str(e.value), str(e.value)
            assert np.array_equal(out, keep), "the output buffer was written"
        with pytest.raises(amd.RifeError) as e:
            g.upload_yuv(a, w, h, px)
        assert "(-6)" in str(e.value)
        d0, d1, do = _dev(a), _dev(b), _dev(out)
        torch.cuda.synchronize()
        with pytest.raises(amd.RifeError) as e:
            g.process_device(d0.data_ptr(), d1.data_ptr(), w, h, 0.5, do.data_ptr(), None, pixfmt=px)
        assert "(-6)" in str(e.value)
        with pytest.raises(amd.RifeError) as e:
            g.process_device_batch([d0.data_ptr()] * 2, [d1.data_ptr()] * 2, w, h, [0.5, 0.3], [do.data_ptr()] * 2, None, pixfmt=px)
        assert "(-6)" in str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(_host(do, out), keep)
    a8, b8 = gen_frames.smooth_pair(64, 64, 2)
    assert g.process(a8, b8, 0.5).shape == a8.shape           # the 8-bit path of the same engine is untouched by the refusals


def test_bad_colour_descriptions_are_einval(engines):
    import torch
    g, _ = engines
    L = g._L
    w, h = 32, 32
    bad = [(P010 | amd.CSP_FULL, "full"), (I420P10 | amd.CSP_FULL | amd.CSP_BT601, "full"), (NV12 | (3 << 8), "matrix"), (I420 | (15 << 8), "matrix"),
           (amd.PIX_RGB8 | amd.CSP_BT601, "RGB"), (amd.PIX_RGB8 | amd.CSP_FULL, "RGB"), (amd.PIX_A2B10G10R10 | amd.CSP_BT2020NCL, "RGB"), (NV12 | (1 << 13), "unknown"),
           (9, "unknown"), (3, "unknown"), (5, "unknown"), (7, "unknown"), (15, "unknown"), (20, "unknown")]      # 5 .. 15 stay reserved
    for px, word in bad:
        n = 8 * w * h
        a = np.zeros(n, np.uint8); out = np.full(n, 0x5a, np.uint8)
        assert L.rife_hip_process_px(g._h, a.ctypes.data, a.ctypes.data, w, h, ctypes.c_float(0.5), out.ctypes.data, px) == -1, hex(px)
        assert word in L.rife_hip_last_error().decode(), (hex(px), L.rife_hip_last_error().decode())
        assert (out == 0x5a).all()
        f = ctypes.c_void_p()
        assert L.rife_hip_frame_upload_px(g._h, a.ctypes.data, w, h, px, ctypes.byref(f)) == -1 and not f.value
        d = torch.full((n,), 0x5a, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.rife_hip_process_device_px(g._h, d.data_ptr(), d.data_ptr(), w, h, ctypes.c_float(0.5), d.data_ptr(), px, None) == -1
        pa = (ctypes.c_void_p * 1)(d.data_ptr())
        assert L.rife_hip_process_device_batch_px(g._h, 1, pa, pa, (ctypes.c_float * 1)(0.5), pa, w, h, px, None) == -1
        torch.cuda.synchronize()
        assert (d == 0x5a).all().item()
    assert amd.frame_bytes(33, 47, NV12 | amd.CSP_BT601) == yr.frame_bytes(33, 47, NV12) == amd.yuv_frame_bytes(33, 47, NV12)
    assert amd.frame_bytes(33, 47, P010) == yr.frame_bytes(33, 47, P010) == amd.yuv_frame_bytes(33, 47, I420P10)
    assert amd.frame_bytes(33, 47, 9) == 0


def test_frames_that_differ_in_colour_description_are_refused(engines):
    g, _ = engines
    w, h = 32, 32
    a, b = scene(w, h, NV12)
    f0 = g.upload_yuv(a, w, h, NV12); f1 = g.upload_yuv(b, w, h, NV12 | amd.CSP_BT601); f2 = g.upload_yuv(b, w, h, I420)
    out = np.full_like(a, 0x5a)
    for x in (f1, f2):
        assert g._L.rife_hip_process_frames(g._h, f0._f, x._f, ctypes.c_float(0.5), out.ctypes.data) == -1
        assert "differ" in g._L.rife_hip_last_error().decode()
    assert (out == 0x5a).all()
    for x in (f0, f1, f2):
        x.release()


# ---- 6. no bleed between formats on one engine ----------------------------------------------------------------------------------------------------

def test_rgb8_calls_around_a_yuv_call_are_identical(modeldirs):
    import torch
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    w, h = 100, 60
    a8, b8 = gen_frames.smooth_pair(w, h, 5)
    ya, yb = scene(w, h, I420)
    d0, d1 = _dev(a8), _dev(b8); y0, y1 = _dev(ya), _dev(yb)
    o1 = torch.zeros_like(d0); o2 = torch.zeros_like(d0); oy = torch.zeros_like(y0)
    torch.cuda.synchronize()
    first = g.process(a8, b8, 0.5)
    g.process_device(d0.data_ptr(), d1.data_ptr(), w, h, 0.5, o1.data_ptr(), None)             # one workspace (the NULL stream's) serves all three
    yuv = g.process_yuv(ya, yb, w, h, 0.5, I420)
    g.process_device(y0.data_ptr(), y1.data_ptr(), w, h, 0.5, oy.data_ptr(), None, pixfmt=I420)
    g.process_device(d0.data_ptr(), d1.data_ptr(), w, h, 0.5, o2.data_ptr(), None)
    again = g.process(a8, b8, 0.5)
    torch.cuda.synchronize()
    assert np.array_equal(first, again)
    assert np.array_equal(_host(o1, first), first) and np.array_equal(_host(o2, first), first)
    assert np.array_equal(_host(oy, yuv), yuv)
    assert np.array_equal(g.process_yuv(ya, yb, w, h, 0.5, I420), yuv)
