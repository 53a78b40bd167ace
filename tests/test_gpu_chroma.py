"""4:2:2 / 4:4:4 Y'CbCr frames (RIFE_HIP_PIX_I422 / I422P10 / I444 / I444P10, include/rife_hip.h "video") through the rife-v4.6 engine, on the GPU.

  1  the kernels alone (csrc/yuv.h k_preproc_yuvc / k_postproc_yuvc, both forms) equal tests/chroma_ref.py bit for bit
  2  the same kernels on pitched planes in separate buffers: the host's choice, the scalar form and the tight frame agree; nothing outside the rows is written
  3  a call is byte for byte rgb10_to_yuv(process(yuv_to_rgb10(a), yuv_to_rgb10(b), t)) through every _px and image entry point
  4  against the reference network at most 1 code per sample (the depth-10 bound times the sensitivity pinned in tests/test_yuv_host.py)
  5  timestep 0 / 1 return the canonical inputs
  6  everything out of scope is refused before anything is written"""
import ctypes
import importlib

import numpy as np
import pytest

import chroma_ref as cr
import deep_ref
from oracle import pyoracle

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
I422, I422P10, I444, I444P10 = amd.PIX_I422, amd.PIX_I422P10, amd.PIX_I444, amd.PIX_I444P10
FORMATS = (I422, I422P10, I444, I444P10)
FMT_IDS = {I422: "i422", I422P10: "i422p10", I444: "i444", I444P10: "i444p10"}
# w % 8 == 0: the x8 forms (8x1, 40x7, 64x33: with odd heights; 256x192: more than one block of 256 lanes x 8 columns would need w > 2048, so several rows of
# blocks stand in); every other size: the scalar forms
KERNEL_SIZES = [(1, 1), (2, 1), (3, 5), (31, 33), (33, 47), (8, 1), (40, 7), (64, 33), (256, 192)]
# all four formats at matrix 709, each matrix on one format, full range at 8 bits
KERNEL_CASES = [I422, I422P10, I444, I444P10, I422 | amd.CSP_BT601, I444P10 | amd.CSP_BT2020NCL, I422 | amd.CSP_FULL, I444 | amd.CSP_FULL | amd.CSP_BT601]


def _id(px):
    return "%s-%s-%s" % (FMT_IDS[px & 0xff], {0: "709", 1: "601", 2: "2020"}[(px >> 8) & 15], "full" if px & amd.CSP_FULL else "limited")


@pytest.fixture(scope="module")
def engines(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    return g, o


_SCENES = {}
_COMPOSED = {}


def scene(w, h, px, seed=40):
    """Two frames of one moving 10-bit scene (tests/deep_ref.py), in format px; the RGB scene is shared by the formats."""
    key = (w, h, seed)
    if key not in _SCENES:
        _SCENES[key] = deep_ref.deep_pair_uncached(w, h, seed + w)
    a, b = _SCENES[key]
    return cr.rgb10_to_yuv(a, px), cr.rgb10_to_yuv(b, px)


def random_frame(w, h, px, seed, top=None):
    """Random samples over the whole code range of every plane: most of them out of gamut."""
    return np.random.default_rng(seed).integers(0, top or (1024 if cr.depth(px) == 10 else 256), cr.frame_elems(w, h, px)).astype(cr.dtype(px))


def unpack_padded(d):
    return np.stack([d & 1023, (d >> 10) & 1023, (d >> 20) & 1023], axis=-1).astype(np.uint16)


def composed(g, a, b, w, h, t, px):
    """The header's composition through the A2B10G10R10 call; computed once per case and shared."""
    key = (a.tobytes(), b.tobytes(), w, h, t, px)
    if key not in _COMPOSED:
        mid = g.process(amd.pack_a2b10g10r10(cr.yuv_to_rgb10(a, w, h, px)), amd.pack_a2b10g10r10(cr.yuv_to_rgb10(b, w, h, px)), t)
        _COMPOSED[key] = cr.rgb10_to_yuv(amd.unpack_a2b10g10r10(mid), px)
    return _COMPOSED[key]


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ---- planes in separate buffers with gaps -------------------------------------------------------------------------------------------------------

FILL = 0xC5
MARGIN = 64


class Planes:
    """Y, Cb, Cr in three buffers of their own, FILL everywhere outside the rows' own bytes.  layout (a = the luma access of the x8 forms, 8 elements; ac = the
    chroma access, 4 elements for 4:2:2 and 8 for 4:4:4):
      a64     bases and pitches multiples of 64: the x8 forms where w % 8 == 0
      exact   luma base and pitch multiples of a but not of 2a, chroma of ac but not of 2ac: the x8 forms still qualify, with nothing to spare
      elem    bases one element past a 64-byte boundary, pitch = row bytes + one element: the scalar forms
      luma    luma as in a64, chroma as in elem: luma alone would qualify
      chroma  the other way round"""

    def __init__(self, w, h, px, layout, flat=None):
        self.w, self.h, self.px, self.es = w, h, px, 2 if cr.depth(px) == 10 else 1
        cw, _ = cr.chroma_dims(w, h, px)
        self.rb = [w * self.es, cw * self.es, cw * self.es]
        acc = [8 * self.es, 8 // cr.subx(px) * self.es, 8 // cr.subx(px) * self.es]
        self.bufs, self.off, self.pitch = [], [], []
        for p in range(3):
            wide = layout in ("a64", "exact") or (layout == "luma" and p == 0) or (layout == "chroma" and p > 0)
            if layout == "exact":
                pitch = (self.rb[p] + acc[p] - 1) // acc[p] * acc[p]
                pitch += acc[p] if pitch % (2 * acc[p]) == 0 else 0
                mis = acc[p]
            elif wide:
                pitch, mis = (self.rb[p] + 63) // 64 * 64, 0
            else:
                pitch, mis = self.rb[p] + self.es, self.es
            raw = np.full(2 * MARGIN + h * pitch + 128, FILL, np.uint8)
            start = (-raw.ctypes.data) % 64 + MARGIN + mis
            self.bufs.append(raw); self.off.append(start); self.pitch.append(pitch)
        self.desc = amd.device_image(w, h, px, [(self.bufs[p].ctypes.data + self.off[p], self.pitch[p]) for p in range(3)])
        self.desc._keep = self
        if flat is not None:
            src = np.ascontiguousarray(flat).view(np.uint8).reshape(-1)
            for p, o in enumerate(cr.plane_offsets(w, h, px)):
                for y in range(h):
                    s = self.off[p] + y * self.pitch[p]
                    self.bufs[p][s:s + self.rb[p]] = src[o * self.es + y * self.rb[p]: o * self.es + (y + 1) * self.rb[p]]

    def mask(self, p):
        m = np.zeros(self.bufs[p].size, bool)
        for y in range(self.h):
            m[self.off[p] + y * self.pitch[p]: self.off[p] + y * self.pitch[p] + self.rb[p]] = True
        return m

    def gather(self):
        return np.concatenate([self.bufs[p][self.mask(p)] for p in range(3)]).view(cr.dtype(self.px))

    def intact(self):
        return all(bool((self.bufs[p][~self.mask(p)] == FILL).all()) for p in range(3))


def plane_views(pl):
    """The planes of a Planes object as 2-D arrays of the format's dtype that share its buffers (what process_planes takes)."""
    dt = np.dtype(cr.dtype(pl.px))
    cw, _ = cr.chroma_dims(pl.w, pl.h, pl.px)
    return tuple(np.ndarray((pl.h, n), dt, buffer=pl.bufs[p].data, offset=pl.off[p], strides=(pl.pitch[p], dt.itemsize)) for p, n in enumerate((pl.w, cw, cw)))


class DevicePlanes:
    """The buffers of a Planes object in device memory, at the host buffers' alignment modulo 64."""

    def __init__(self, pl):
        import torch
        self.pl, self.t, self.shift = pl, [], []
        for p in range(3):
            t = torch.empty(pl.bufs[p].size + 64, dtype=torch.uint8, device="cuda")
            shift = (pl.bufs[p].ctypes.data - t.data_ptr()) % 64
            t[shift:shift + pl.bufs[p].size] = torch.from_numpy(pl.bufs[p])
            self.t.append(t); self.shift.append(shift)
        self.desc = amd.device_image(pl.w, pl.h, pl.px, [(self.t[p].data_ptr() + self.shift[p] + pl.off[p], pl.pitch[p]) for p in range(3)])

    def fetch(self):
        for p in range(3):
            self.pl.bufs[p][:] = self.t[p][self.shift[p]:self.shift[p] + self.pl.bufs[p].size].cpu().numpy()
        return self.pl


LAYOUTS = ("a64", "exact", "elem", "luma", "chroma")


# ---- 1. the kernels alone, exact ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", KERNEL_CASES, ids=_id)
def test_kernels_alone_equal_the_specification(px):
    for (w, h) in KERNEL_SIZES:
        f = random_frame(w, h, px, 5 + w)
        got = amd.op_yuv_to_rgb10(f, w, h, px)
        want = cr.yuv_to_rgb10(f, w, h, px)
        assert np.array_equal(unpack_padded(got[:h, :w]), want), "in %s %dx%d: %d pixels differ" % (_id(px), w, h, int((unpack_padded(got[:h, :w]) != want).any(axis=-1).sum()))
        assert not got[h:].any() and not got[:, w:].any(), "padding of %dx%d is not zero RGB" % (w, h)
        assert not (got >> 30).any()
        rng = np.random.default_rng(9 + h)
        rgb = rng.integers(0, 1024, (h, w, 3), dtype=np.uint16)
        packed = amd.pack_a2b10g10r10(rgb) & np.uint32(0x3fffffff) | (rng.integers(0, 4, (h, w), dtype=np.uint32) << 30)      # the alpha bits are ignored
        back = amd.op_rgb10_to_yuv(packed, px)
        assert np.array_equal(back, cr.rgb10_to_yuv(rgb, px)), "out %s %dx%d: %d samples differ" % (_id(px), w, h, int((back != cr.rgb10_to_yuv(rgb, px)).sum()))


@pytest.mark.parametrize("px", [I422P10, I444P10], ids=_id)
def test_ten_bit_samples_above_1023_are_read_as_1023(px):
    for (w, h) in [(33, 47), (40, 7)]:
        f = random_frame(w, h, px, 3, top=65536)
        assert (f > 1023).any()
        assert np.array_equal(unpack_padded(amd.op_yuv_to_rgb10(f, w, h, px)[:h, :w]), cr.yuv_to_rgb10(np.minimum(f, 1023), w, h, px))


# ---- 2. pitched planes ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", [I422 | amd.CSP_BT601, I422P10, I444, I444P10 | amd.CSP_BT2020NCL], ids=_id)
def test_pitched_input_kernels(px):
    for (w, h) in [(1, 1), (3, 5), (33, 47), (8, 1), (40, 7), (64, 33)]:
        f = random_frame(w, h, px, 11 + w)
        want = amd.op_yuv_to_rgb10(f, w, h, px)                                     # the tight frame
        assert np.array_equal(unpack_padded(want[:h, :w]), cr.yuv_to_rgb10(f, w, h, px))
        tight = amd.device_image(w, h, px, [(f.ctypes.data + o * f.itemsize, amd.image_row_bytes(w, px, p)) for p, o in enumerate(cr.plane_offsets(w, h, px))])
        assert np.array_equal(amd.op_image_to_resident(tight, 2), want)
        for layout in LAYOUTS:
            pl = Planes(w, h, px, layout, f)
            for force in (0, 1):
                got = amd.op_image_to_resident(pl.desc, force)
                assert np.array_equal(got, want), "%s %dx%d %s form %d: %d dwords differ" % (_id(px), w, h, layout, force, int((got != want).sum()))
            assert pl.intact() and np.array_equal(pl.gather(), f)


@pytest.mark.parametrize("px", [I422 | amd.CSP_BT601, I422P10, I444, I444P10 | amd.CSP_BT2020NCL], ids=_id)
def test_pitched_output_kernels_write_their_rows_and_nothing_else(px):
    for (w, h) in [(1, 1), (3, 5), (33, 47), (8, 1), (40, 7), (64, 33)]:
        src = np.random.default_rng(23 + h).integers(0, 2 ** 32, (h, w), dtype=np.uint32)      # the alpha bits are ignored
        want = amd.op_rgb10_to_yuv(src, px)                                                   # the tight frame
        assert np.array_equal(want, cr.rgb10_to_yuv(unpack_padded(src), px))
        for layout in LAYOUTS:
            for force in (0, 1):
                pl = Planes(w, h, px, layout)
                amd.op_resident_to_image(src, pl.desc, force)
                assert np.array_equal(pl.gather(), want), "%s %dx%d %s form %d: %d samples differ" % (_id(px), w, h, layout, force, int((pl.gather() != want).sum()))
                assert pl.intact(), "%s %dx%d %s form %d: bytes outside the rows were written" % (_id(px), w, h, layout, force)


# ---- 3. the composition, exact, through every entry point ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (33, 47), (100, 60), (256, 192)])
def test_a_call_is_the_packed_10_bit_call_converted(engines, w, h):
    g, _ = engines
    for px in FORMATS + (I422 | amd.CSP_BT601 | amd.CSP_FULL, I444P10 | amd.CSP_BT2020NCL):
        a, b = scene(w, h, px)
        got = g.process_yuv(a, b, w, h, 0.4, px)
        assert got.dtype == a.dtype and got.shape == a.shape
        want = composed(g, a, b, w, h, 0.4, px)
        assert np.array_equal(got, want), "%s %dx%d: %d samples differ" % (_id(px), w, h, int((got != want).sum()))


@pytest.mark.parametrize("px", FORMATS, ids=_id)
@pytest.mark.parametrize("w,h", [(33, 47), (256, 192)])
def test_resident_batch_and_stream_mode(engines, w, h, px):
    import torch
    g, _ = engines
    pairs = [scene(w, h, px, seed) for seed in (40, 41, 42)]
    ts = [0.5, 0.25, 0.7]
    want = [composed(g, a, b, w, h, t, px) for (a, b), t in zip(pairs, ts)]
    d0 = [_dev(a) for a, _ in pairs]; d1 = [_dev(b) for _, b in pairs]
    outs = [torch.zeros_like(x) for x in d0]
    torch.cuda.synchronize()
    for i in range(3):
        g.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], outs[i].data_ptr(), None, pixfmt=px)
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(_host(outs[i], want[i]), want[i]), "process_device pair %d" % i
    st = torch.cuda.Stream()
    for stream in (st.cuda_stream, None):
        outs = [torch.zeros_like(x) for x in d0]
        torch.cuda.synchronize()
        g.process_device_batch([x.data_ptr() for x in d0], [x.data_ptr() for x in d1], w, h, ts, [o.data_ptr() for o in outs], stream, pixfmt=px)
        torch.cuda.synchronize()
        for i in range(3):
            assert np.array_equal(_host(outs[i], want[i]), want[i]), "process_device_batch pair %d" % i
    # frame_upload_px + process_frames: a frame serves both sides and two timesteps
    f = [g.upload_yuv(pairs[0][0], w, h, px), g.upload_yuv(pairs[0][1], w, h, px)]
    assert np.array_equal(g.process_frames(f[0], f[1], 0.5), want[0])
    assert np.array_equal(g.process_frames(f[0], f[1], 0.25), composed(g, pairs[0][0], pairs[0][1], w, h, 0.25, px))
    assert np.array_equal(g.process_frames(f[1], f[0], 0.5), composed(g, pairs[0][1], pairs[0][0], w, h, 0.5, px))
    for x in f:
        x.release()


@pytest.mark.parametrize("px", FORMATS, ids=_id)
@pytest.mark.parametrize("w,h", [(33, 47), (64, 33)])
def test_image_entry_points(engines, w, h, px):
    import torch
    g, _ = engines
    a, b = scene(w, h, px)
    want = composed(g, a, b, w, h, 0.5, px)
    user = torch.cuda.Stream()
    for layout in ("a64", "elem", "chroma"):
        # host planes: process_planes, upload_planes + process_frames_image
        pa, pb, po = Planes(w, h, px, layout, a), Planes(w, h, px, layout, b), Planes(w, h, px, layout)
        g.process_planes(plane_views(pa), plane_views(pb), 0.5, px, out=plane_views(po))
        assert np.array_equal(po.gather(), want) and po.intact(), "process_planes %s" % layout
        f0, f1 = g.upload_planes(plane_views(pa), px), g.upload_planes(plane_views(pb), px)
        po = Planes(w, h, px, layout)
        g.process_frames_image(f0, f1, 0.5, po.desc)
        assert np.array_equal(po.gather(), want) and po.intact(), "process_frames_image %s" % layout
        f0.release(); f1.release()
        # device planes, read and written in place
        for stream in (None, user.cuda_stream):
            da, db, do = DevicePlanes(pa), DevicePlanes(pb), DevicePlanes(Planes(w, h, px, layout))
            torch.cuda.synchronize()
            g.process_device_image(da.desc, db.desc, 0.5, do.desc, stream)
            torch.cuda.synchronize()
            out = do.fetch()
            assert np.array_equal(out.gather(), want), "process_device_image %s: %d samples differ" % (layout, int((out.gather() != want).sum()))
            assert out.intact(), "process_device_image %s: bytes outside the rows were written" % layout
            assert np.array_equal(da.fetch().gather(), a) and pa.intact()


@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_device_frames_one_element_off_alignment(engines, px):
    """A w % 8 == 0 frame whose device pointers are offset by one element takes the scalar kernels: same bytes, and nothing outside the frame is written."""
    import torch
    g, _ = engines
    w, h = 256, 192
    a, b = scene(w, h, px)
    want = composed(g, a, b, w, h, 0.4, px)
    esz = a.dtype.itemsize
    n = a.size * esz
    b0 = torch.zeros(n + 32, dtype=torch.uint8, device="cuda"); b1 = torch.zeros(n + 32, dtype=torch.uint8, device="cuda"); out = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    b0[esz:esz + n] = _dev(a); b1[esz:esz + n] = _dev(b)
    torch.cuda.synchronize()
    g.process_device(b0.data_ptr() + esz, b1.data_ptr() + esz, w, h, 0.4, out.data_ptr() + esz, None, pixfmt=px)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out[esz:esz + n], want), want)
    assert not out[:esz].any().item() and not out[esz + n:].any().item(), "bytes outside the frame were written"


# ---- 4. against the reference network ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", [I422, I422P10 | amd.CSP_BT2020NCL, I444 | amd.CSP_FULL | amd.CSP_BT601, I444P10], ids=_id)
@pytest.mark.parametrize("w,h", [(33, 47), (100, 60), (256, 192)])
def test_against_the_reference_network_within_one_code(engines, w, h, px):
    g, o = engines
    a, b = scene(w, h, px)
    t = 0.5
    got = g.process_yuv(a, b, w, h, t, px)
    want = cr.rgb10_to_yuv(deep_ref.expected_frame(o, cr.yuv_to_rgb10(a, w, h, px), cr.yuv_to_rgb10(b, w, h, px), t), px)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s %dx%d: exact %.6f, off by one %.6f, max %d" % (_id(px), w, h, (d == 0).mean(), (d == 1).mean(), d.max()))
    assert d.max() <= 1


# ---- 5. timestep 0 / 1 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_timestep_endpoints_return_the_canonical_inputs(engines, px):
    import torch
    g, _ = engines
    w, h = 33, 47
    a, b = scene(w, h, px)
    if cr.depth(px) == 10:                                              # values above 1023 on input: read, and returned, as 1023
        a = a.copy(); b = b.copy()
        a[::5] |= np.uint16(0x8400); b[::7] |= np.uint16(0x0c00)
    ca, cb = cr.canonical(a, w, h, px), cr.canonical(b, w, h, px)
    if cr.depth(px) == 10:
        assert not np.array_equal(ca, a) and ca.max() == 1023 and np.array_equal(ca, np.minimum(a, 1023))
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
    # images: host planes, resident frames into host planes, device planes
    pa, pb = Planes(w, h, px, "elem", a), Planes(w, h, px, "elem", b)
    po = Planes(w, h, px, "elem")
    g.process_planes(plane_views(pa), plane_views(pb), 1.0, px, out=plane_views(po))
    assert np.array_equal(po.gather(), cb) and po.intact()
    po = Planes(w, h, px, "a64")
    g.process_frames_image(f0, f1, 0.0, po.desc)
    assert np.array_equal(po.gather(), ca) and po.intact()
    da, db, do = DevicePlanes(pa), DevicePlanes(pb), DevicePlanes(Planes(w, h, px, "a64"))
    torch.cuda.synchronize()
    g.process_device_image(da.desc, db.desc, 0.0, do.desc, None)
    torch.cuda.synchronize()
    assert np.array_equal(do.fetch().gather(), ca) and do.pl.intact()
    f0.release(); f1.release()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife", {}, "v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal"),
                                         ("rife-v4.6", dict(uhd_mode=True), "UHD")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    g = amd.RIFE(0, **fl); g.load(modeldirs[fam])
    w, h = 64, 64
    for px in (I422, I444P10):
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
        pa, pb, po = Planes(w, h, px, "a64", a), Planes(w, h, px, "a64", b), Planes(w, h, px, "a64")
        with pytest.raises(amd.RifeError) as e:
            g.process_planes(plane_views(pa), plane_views(pb), 0.5, px, out=plane_views(po))
        assert "(-6)" in str(e.value) and word in str(e.value), str(e.value)
        assert po.intact() and (po.gather().view(np.uint8) == FILL).all()


def test_bad_formats_and_colour_descriptions_are_einval(engines):
    import torch
    g, _ = engines
    L = g._L
    w, h = 32, 32
    bad = [(I422P10 | amd.CSP_FULL, "full"), (I444P10 | amd.CSP_FULL | amd.CSP_BT601, "full"), (I422 | (3 << 8), "matrix"), (I444 | (15 << 8), "matrix"),
           (I444 | (1 << 13), "unknown"), (32, "unknown"), (34, "unknown"), (48, "unknown"), (50, "unknown"), (52, "unknown"), (20, "unknown")]
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
        im = amd.device_image(w, h, px, [(d.data_ptr(), 64), (d.data_ptr() + 2048, 64), (d.data_ptr() + 4096, 64)])
        assert L.rife_hip_process_device_image(g._h, ctypes.byref(im), ctypes.byref(im), ctypes.c_float(0.5), ctypes.byref(im), None) == -1
        torch.cuda.synchronize()
        assert (d == 0x5a).all().item()


def test_frames_that_differ_in_class_or_colour_description_are_refused(engines):
    g, _ = engines
    w, h = 32, 32
    a, b = scene(w, h, I444)
    a2, _ = scene(w, h, I422)
    f0 = g.upload_yuv(a, w, h, I444); f1 = g.upload_yuv(b, w, h, I444 | amd.CSP_BT601); f2 = g.upload_yuv(a2, w, h, I422)
    f3 = g.upload_yuv(np.zeros(amd.yuv_frame_bytes(w, h, amd.PIX_I420), np.uint8), w, h, amd.PIX_I420)
    out = np.full_like(a, 0x5a)
    for x in (f1, f2, f3):
        assert g._L.rife_hip_process_frames(g._h, f0._f, x._f, ctypes.c_float(0.5), out.ctypes.data) == -1
        assert "differ" in g._L.rife_hip_last_error().decode()
    assert (out == 0x5a).all()
    for x in (f0, f1, f2, f3):
        x.release()
