"""Planar RGB frames (RIFE_HIP_PIX_RGBP8 / RGBP10 / RGBPH / RGBPF, include/rife_hip.h "planar RGB") through the rife-v4.6 engine, on the GPU.

Every expected value is tests/planar_ref.py applied around the engine's own A2B10G10R10 call - the separately tested depth-10 path, not the new kernels -
and every comparison is byte-exact:
    out = from10(process_px(to10(in0), to10(in1), t, A2B10G10R10))
  1  the tight _px call, odd sizes to several blocks
  2  the kernels alone (csrc/planar_rgb.h), wide form against the forced scalar form against the specification
  3  host and device image calls on planes in three allocations with row padding: nothing outside the rows is written
  4  timestep 0 / 1 return the canonical samples
  5  stream mode, the resident batch, flow scale 2
  6  everything out of scope is refused before anything is written
  7  against the reference network: at most one ten-bit code per sample (RGBP8: one eight-bit code) - the engine's standing contract, here to guard the wiring"""
import ctypes
import importlib

import numpy as np
import pytest

import deep_ref
import planar_ref as pr
from oracle import pyoracle

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
P8, P10, PH, PF = amd.PIX_RGBP8, amd.PIX_RGBP10, amd.PIX_RGBPH, amd.PIX_RGBPF
FORMATS = (P8, P10, PH, PF)
_id = pr.NAMES.get


@pytest.fixture(scope="module")
def g(modeldirs):
    e = amd.RIFE(0, rife_v4=True); e.load(modeldirs["rife-v4.6"])
    return e


_SCENES = {}
_COMPOSED = {}


def frames(w, h, px, seed=60):
    """Two (3, h, w) frames of one moving scene (tests/deep_ref.py) in format px, with the values the specification singles out spread over them: codes 0 and
    max; RGBP10: values above 1023; half / float: samples between the codes, NaN, both infinities, negatives, values above 1 and the half-code boundaries."""
    key = (w, h, seed)
    if key not in _SCENES:
        _SCENES[key] = deep_ref.deep_pair_uncached(w, h, seed + w)
    out = []
    for i, codes in enumerate(_SCENES[key]):
        rng = np.random.default_rng(seed + 7 * i + px)
        f = pr.from_rgb10(codes, px)
        flat = f.reshape(-1)
        n = flat.size

        def put(vals):
            vals = np.asarray(vals).astype(f.dtype)
            flat[rng.choice(n, min(n, vals.size), replace=False)] = vals[:min(n, vals.size)]
        if px in (PH, PF):
            flat += (rng.uniform(-0.49, 0.49, n) / 1023.0).astype(f.dtype)           # between the codes
            if n >= 64:
                put(pr.boundary_floats().reshape(-1)[rng.choice(3069, min(n // 4, 3069), replace=False)])
                put([np.nan, -np.nan, np.inf, -np.inf, -1.0, -0.0, -1e-3, 1.0 + 1e-3, 2.0, 60000.0, 1e-8, 1.0, 0.0] * 2)
        elif px == P10:
            if n >= 64:
                put([1024, 1025, 2047, 4095, 32768, 65535, 1023, 0] * 2)
        elif n >= 64:
            put([0, 255, 1, 254] * 2)
        out.append(f)
    return out[0], out[1]


def composed(e, a, b, t, px):
    """The header's composition through the A2B10G10R10 call of engine e; computed once per case and shared."""
    key = (id(e), a.tobytes(), b.tobytes(), a.shape, t, px)
    if key not in _COMPOSED:
        mid = e.process(amd.pack_a2b10g10r10(pr.to_rgb10(a, px)), amd.pack_a2b10g10r10(pr.to_rgb10(b, px)), t)
        _COMPOSED[key] = pr.from_rgb10(amd.unpack_a2b10g10r10(mid), px)
    return _COMPOSED[key]


def same(got, want):
    """Byte for byte (a NaN would compare unequal to itself; none may come out anyway)."""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def process_px(e, a, b, t, px, out=None):
    """rife_hip_process_px on tight frames."""
    _, h, w = a.shape
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    out = np.empty_like(a) if out is None else out
    rc = e._L.rife_hip_process_px(e._h, a.ctypes.data, b.ctypes.data, w, h, ctypes.c_float(t), out.ctypes.data, px)
    return rc, out


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ---- planes in three allocations with gaps ---------------------------------------------------------------------------------------------------------------

FILL = 0xC5
MARGIN = 64


class Planes:
    """R, G, B in three buffers of their own, FILL everywhere outside the rows' own bytes.  layout:
      a64    bases and pitches multiples of 64: the wide form where w % 8 == 0
      exact  bases and pitches multiples of the wide access (16 bytes, u8: 8) but not of twice that: the wide form still qualifies, with nothing to spare
      elem   bases one element past a 64-byte boundary, pitch = row bytes + one element: the scalar form
      off1   pitches multiples of 64, bases one element past a 64-byte boundary: w % 8 == 0 alone does not make the wide form legal
      one    plane 1 as in elem, the others as in a64: one plane that does not qualify sends the whole frame to the scalar form"""

    def __init__(self, w, h, px, layout, frame=None):
        self.w, self.h, self.px, self.es = w, h, px, pr.elem(px)
        self.rb = w * self.es
        acc = 8 if px == P8 else 16
        self.bufs, self.off, self.pitch = [], [], []
        for p in range(3):
            lay = ("elem" if p == 1 else "a64") if layout == "one" else layout
            if lay == "exact":
                pitch = (self.rb + acc - 1) // acc * acc
                pitch += acc if pitch % (2 * acc) == 0 else 0
                mis = acc
            elif lay == "a64":
                pitch, mis = (self.rb + 63) // 64 * 64, 0
            elif lay == "off1":
                pitch, mis = (self.rb + 63) // 64 * 64, self.es
            else:
                pitch, mis = self.rb + self.es, self.es
            raw = np.full(2 * MARGIN + h * pitch + 128, FILL, np.uint8)
            start = (-raw.ctypes.data) % 64 + MARGIN + mis
            self.bufs.append(raw); self.off.append(start); self.pitch.append(pitch)
        self.desc = self.descriptor((0, 1, 2))
        if frame is not None:
            src = np.ascontiguousarray(frame).view(np.uint8).reshape(3, h, self.rb)
            for p in range(3):
                for y in range(h):
                    s = self.off[p] + y * self.pitch[p]
                    self.bufs[p][s:s + self.rb] = src[p, y]

    def descriptor(self, order):
        d = amd.device_image(self.w, self.h, self.px, [(self.bufs[p].ctypes.data + self.off[p], self.pitch[p]) for p in order])
        d._keep = self
        return d

    def mask(self, p):
        m = np.zeros(self.bufs[p].size, bool)
        for y in range(self.h):
            m[self.off[p] + y * self.pitch[p]: self.off[p] + y * self.pitch[p] + self.rb] = True
        return m

    def gather(self):
        return np.concatenate([self.bufs[p][self.mask(p)] for p in range(3)]).view(pr.dtype(self.px)).reshape(3, self.h, self.w)

    def intact(self):
        return all(bool((self.bufs[p][~self.mask(p)] == FILL).all()) for p in range(3))

    def views(self):
        """The planes as 2-D arrays of the format's dtype that share the buffers (what process_planes takes)."""
        dt = np.dtype(pr.dtype(self.px))
        return tuple(np.ndarray((self.h, self.w), dt, buffer=self.bufs[p].data, offset=self.off[p], strides=(self.pitch[p], dt.itemsize)) for p in range(3))


class DevicePlanes:
    """The buffers of a Planes object in device memory, at the host buffers' alignment modulo 64."""

    def __init__(self, pl, order=(0, 1, 2)):
        import torch
        self.pl, self.t, self.shift = pl, [], []
        for p in range(3):
            t = torch.empty(pl.bufs[p].size + 64, dtype=torch.uint8, device="cuda")
            shift = (pl.bufs[p].ctypes.data - t.data_ptr()) % 64
            t[shift:shift + pl.bufs[p].size] = torch.from_numpy(pl.bufs[p])
            self.t.append(t); self.shift.append(shift)
        self.desc = amd.device_image(pl.w, pl.h, pl.px, [(self.t[p].data_ptr() + self.shift[p] + pl.off[p], pl.pitch[p]) for p in order])

    def fetch(self):
        for p in range(3):
            self.pl.bufs[p][:] = self.t[p][self.shift[p]:self.shift[p] + self.pl.bufs[p].size].cpu().numpy()
        return self.pl


def unpack_padded(d):
    return np.stack([d & 1023, (d >> 10) & 1023, (d >> 20) & 1023], axis=-1).astype(np.uint16)


# ---- 1. the tight _px call ----------------------------------------------------------------------------------------------------------------------------------

# 1x1, 7x5, 33x47: the scalar form, its tail and the padding; 64x32: no padding, the wide form; 256x192: several blocks of rows, the wide form
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (33, 47), (64, 32), (256, 192)])
def test_a_tight_call_is_the_packed_10_bit_call_converted(g, w, h):
    for px in FORMATS:
        a, b = frames(w, h, px)
        rc, got = process_px(g, a, b, 0.4, px)
        assert rc == 0, g._L.rife_hip_last_error().decode()
        want = composed(g, a, b, 0.4, px)
        assert same(got, want), "%s %dx%d: %d samples differ" % (_id(px), w, h, int((got.view(np.uint8) != want.view(np.uint8)).sum()))
        # the Python surface: a (3, h, w) array stands for its three planes
        out = g.process_planes(a, b, 0.4, px)
        assert same(np.stack(out), want)


def test_the_test_frames_hold_the_special_values():
    a, _ = frames(33, 47, PF)
    assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and (a < 0).any() and (a > 1).any()
    a, _ = frames(33, 47, PH)
    assert np.isnan(a).any() and np.isinf(a).any() and (a < 0).any() and (a > 1).any()
    a, _ = frames(33, 47, P10)
    assert (a > 1023).any() and (a == 0).any()
    a, _ = frames(33, 47, P8)
    assert (a == 0).any() and (a == 255).any()


# ---- 2. the kernels alone: wide form, forced scalar form, specification ------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_wide_and_scalar_input_kernels(px):
    for (w, h) in [(64, 32), (72, 40), (33, 47), (8, 1)]:
        f, _ = frames(w, h, px, 61)
        codes = pr.to_rgb10(f, px)
        tight = amd.planes_image(f, w, h, px)
        want = amd.op_image_to_resident(tight, 2)                                      # the tight path of the _px calls
        assert np.array_equal(unpack_padded(want[:h, :w]), codes), "%s %dx%d: %d pixels differ from the specification" % (_id(px), w, h, int((unpack_padded(want[:h, :w]) != codes).any(axis=-1).sum()))
        assert not want[h:].any() and not want[:, w:].any(), "padding of %dx%d is not zero RGB" % (w, h)
        assert not (want >> 30).any()
        for layout in ("a64", "exact", "elem", "off1", "one"):
            pl = Planes(w, h, px, layout, f)
            for force in (0, 1):
                got = amd.op_image_to_resident(pl.desc, force)
                assert np.array_equal(got, want), "%s %dx%d %s form %d: %d dwords differ" % (_id(px), w, h, layout, force, int((got != want).sum()))
            assert pl.intact() and same(pl.gather(), f)


@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_wide_and_scalar_output_kernels_write_their_rows_and_nothing_else(px):
    for (w, h) in [(64, 32), (72, 40), (33, 47), (8, 1)]:
        rng = np.random.default_rng(23 + h)
        src = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)                        # the alpha bits are ignored
        src.reshape(-1)[:min(src.size, 1024)] = (np.arange(1024, dtype=np.uint32) * 0x100401)[:min(src.size, 1024)]      # every code in every channel where the frame has room
        want = pr.from_rgb10(unpack_padded(src), px)
        for layout in ("a64", "exact", "elem", "off1", "one"):
            for force in (0, 1):
                pl = Planes(w, h, px, layout)
                amd.op_resident_to_image(src, pl.desc, force)
                assert same(pl.gather(), want), "%s %dx%d %s form %d: %d bytes differ" % (_id(px), w, h, layout, force, int((pl.gather().view(np.uint8) != want.view(np.uint8)).sum()))
                assert pl.intact(), "%s %dx%d %s form %d: bytes outside the rows were written" % (_id(px), w, h, layout, force)


# ---- 3. image calls ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", FORMATS, ids=_id)
@pytest.mark.parametrize("w,h,layout", [(33, 47, "elem"), (64, 32, "a64"), (64, 32, "off1")])
def test_image_entry_points(g, w, h, layout, px):
    """Host planes and device planes in three allocations with row padding, the output pre-filled with a sentinel.  off1: w % 8 == 0 but every base pointer one
    element past an aligned address - the scalar form, the same bytes."""
    import torch
    a, b = frames(w, h, px)
    want = composed(g, a, b, 0.5, px)
    pa, pb, po = Planes(w, h, px, layout, a), Planes(w, h, px, layout, b), Planes(w, h, px, layout)
    g.process_planes(pa.views(), pb.views(), 0.5, px, out=po.views())
    assert same(po.gather(), want) and po.intact(), "process_planes %s" % layout
    user = torch.cuda.Stream()
    for stream in (None, user.cuda_stream):
        da, db, do = DevicePlanes(pa), DevicePlanes(pb), DevicePlanes(Planes(w, h, px, layout))
        torch.cuda.synchronize()
        g.process_device_image(da.desc, db.desc, 0.5, do.desc, stream)
        torch.cuda.synchronize()
        out = do.fetch()
        assert same(out.gather(), want), "process_device_image %s: %d bytes differ" % (layout, int((out.gather().view(np.uint8) != want.view(np.uint8)).sum()))
        assert out.intact(), "process_device_image %s: bytes outside the rows were written" % layout
        assert same(da.fetch().gather(), a) and pa.intact()


@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_planes_permuted_g_b_r(g, px):
    """ffmpeg's gbrp: the producer's buffers hold G, B, R in that order, and the caller names them R, G, B in plane[0..2] of the descriptor - no format of its
    own.  Inputs and output are permuted alike; the result is the R, G, B result, each plane in the buffer the caller named for it."""
    import torch
    w, h = 64, 32
    a, b = frames(w, h, px)
    want = composed(g, a, b, 0.5, px)
    gbr, rgb_of = [1, 2, 0], (2, 0, 1)                                              # buffer i holds channel gbr[i]; channel c lives in buffer rgb_of[c]
    pa, pb, po = Planes(w, h, px, "a64", a[gbr]), Planes(w, h, px, "a64", b[gbr]), Planes(w, h, px, "a64")
    g.process_planes(tuple(pa.views()[i] for i in rgb_of), tuple(pb.views()[i] for i in rgb_of), 0.5, px, out=tuple(po.views()[i] for i in rgb_of))
    assert same(po.gather(), want[gbr]) and po.intact()
    da, db, do = DevicePlanes(pa, rgb_of), DevicePlanes(pb, rgb_of), DevicePlanes(Planes(w, h, px, "a64"), rgb_of)
    torch.cuda.synchronize()
    g.process_device_image(da.desc, db.desc, 0.5, do.desc, None)
    torch.cuda.synchronize()
    assert same(do.fetch().gather(), want[gbr]) and do.pl.intact()


# ---- 4. timestep 0 / 1 -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_timestep_endpoints_return_the_canonical_samples(g, px):
    import torch
    w, h = 33, 47
    a, b = frames(w, h, px)
    ca, cb = pr.canonical(a, px), pr.canonical(b, px)
    if px == P8:
        assert same(ca, a)
    else:
        assert not same(ca, a)                                                       # clamped / quantised / NaN gone
        assert same(pr.canonical(ca, px), ca)
    if px in (PH, PF):
        assert not np.isnan(ca).any() and ca.min() >= 0 and ca.max() <= 1
    # the tight path: host frames, device frames, the resident batch, resident frames
    rc, got = process_px(g, a, b, 0.0, px); assert rc == 0 and same(got, ca)
    rc, got = process_px(g, a, b, 1.0, px); assert rc == 0 and same(got, cb)
    d0, d1 = _dev(a), _dev(b); out = torch.zeros_like(d0)
    torch.cuda.synchronize()
    g.process_device(d0.data_ptr(), d1.data_ptr(), w, h, 1.0, out.data_ptr(), None, pixfmt=px)
    torch.cuda.synchronize()
    assert same(_host(out, cb), cb)
    g.process_device_batch([d0.data_ptr()], [d1.data_ptr()], w, h, [0.0], [out.data_ptr()], None, pixfmt=px)
    torch.cuda.synchronize()
    assert same(_host(out, ca), ca)
    f0, f1 = g.upload_planes(a, px), g.upload_planes(b, px)
    assert same(g.process_frames(f0, f1, 0.0), ca) and same(g.process_frames(f0, f1, 1.0), cb)
    # images: host planes, resident frames into host planes, pitched device planes
    pa, pb = Planes(w, h, px, "elem", a), Planes(w, h, px, "elem", b)
    po = Planes(w, h, px, "elem")
    g.process_planes(pa.views(), pb.views(), 1.0, px, out=po.views())
    assert same(po.gather(), cb) and po.intact()
    po = Planes(w, h, px, "a64")
    g.process_frames_image(f0, f1, 0.0, po.desc)
    assert same(po.gather(), ca) and po.intact()
    for t, c in ((0.0, ca), (1.0, cb)):
        da, db, do = DevicePlanes(pa), DevicePlanes(pb), DevicePlanes(Planes(w, h, px, "a64"))
        torch.cuda.synchronize()
        g.process_device_image(da.desc, db.desc, t, do.desc, None)
        torch.cuda.synchronize()
        assert same(do.fetch().gather(), c) and do.pl.intact()
    f0.release(); f1.release()


# ---- 5. stream mode, the resident batch, flow scale 2 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_stream_mode_equals_the_single_call(g, px):
    w, h = 33, 47
    a, b = frames(w, h, px)
    pa, pb = Planes(w, h, px, "elem", a), Planes(w, h, px, "elem", b)
    f0, f1 = g.upload_planes(pa.views(), px), g.upload_planes(b, px)                 # pitched planes, and a (3, h, w) array
    got = g.process_frames(f0, f1, 0.5)
    assert got.shape == (3, h, w) and same(got, composed(g, a, b, 0.5, px))
    assert same(g.process_frames(f0, f1, 0.25), composed(g, a, b, 0.25, px))
    assert same(g.process_frames(f1, f0, 0.5), composed(g, b, a, 0.5, px))
    po = Planes(w, h, px, "elem")
    g.process_frames_image(f0, f1, 0.5, po.desc)
    assert same(po.gather(), composed(g, a, b, 0.5, px)) and po.intact()
    f0.release(); f1.release()


def test_frames_of_two_planar_formats_are_refused(g):
    w, h = 32, 32
    fr = {px: g.upload_planes(frames(w, h, px)[0], px) for px in FORMATS}
    out = np.full(pr.frame_bytes(w, h, PF), 0x5a, np.uint8)
    for p, q in ((P10, PH), (PH, P10), (P8, PF), (PF, PH)):                          # RGBP10 and RGBPH have the same frame size
        assert g._L.rife_hip_process_frames(g._h, fr[p]._f, fr[q]._f, ctypes.c_float(0.5), out.ctypes.data) == -1
        assert "differ" in g._L.rife_hip_last_error().decode()
        with pytest.raises(ValueError):
            g.process_frames(fr[p], fr[q], 0.5)
    assert (out == 0x5a).all()
    for f in fr.values():
        f.release()


@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_resident_batch_equals_three_single_calls(g, px):
    import torch
    w, h = 33, 47
    pairs = [frames(w, h, px, seed) for seed in (60, 62, 64)]
    ts = [0.5, 0.25, 0.7]
    want = [composed(g, a, b, t, px) for (a, b), t in zip(pairs, ts)]
    d0 = [_dev(a) for a, _ in pairs]; d1 = [_dev(b) for _, b in pairs]
    single = [torch.zeros_like(x) for x in d0]
    torch.cuda.synchronize()
    for i in range(3):
        g.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], single[i].data_ptr(), None, pixfmt=px)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for stream in (st.cuda_stream, None):
        outs = [torch.zeros_like(x) for x in d0]
        torch.cuda.synchronize()
        g.process_device_batch([x.data_ptr() for x in d0], [x.data_ptr() for x in d1], w, h, ts, [o.data_ptr() for o in outs], stream, pixfmt=px)
        torch.cuda.synchronize()
        for i in range(3):
            assert same(_host(outs[i], want[i]), want[i]), "process_device_batch pair %d" % i
            assert torch.equal(outs[i], single[i]), "the batch and the single call differ in pair %d" % i


def test_flow_scale_2(modeldirs):
    import torch
    g2 = amd.RIFE(0, rife_v4=True); g2.load(modeldirs["rife-v4.6"])
    g2.set_flow_scale(2)
    w, h = 100, 60                                                                   # padded to 128 x 64
    for px in FORMATS:
        a, b = frames(w, h, px)
        want = composed(g2, a, b, 0.5, px)                                           # the A2B10G10R10 call at flow scale 2
        rc, got = process_px(g2, a, b, 0.5, px)
        assert rc == 0 and same(got, want), _id(px)
        pa, pb = Planes(w, h, px, "elem", a), Planes(w, h, px, "elem", b)
        da, db, do = DevicePlanes(pa), DevicePlanes(pb), DevicePlanes(Planes(w, h, px, "a64"))
        torch.cuda.synchronize()
        g2.process_device_image(da.desc, db.desc, 0.5, do.desc, None)
        torch.cuda.synchronize()
        assert same(do.fetch().gather(), want) and do.pl.intact(), _id(px)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal"),
                                         ("rife-v4.6", dict(uhd_mode=True), "UHD")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = amd.RIFE(0, **fl); e.load(modeldirs[fam])
    w, h = 64, 64
    for px in (P8, PF):
        a, b = frames(w, h, px)
        out = np.full_like(a.view(np.uint8), 0x5a).view(a.dtype)
        keep = out.copy()
        for t in (0.5, 0.0):
            rc, _ = process_px(e, a, b, t, px, out=out)
            msg = e._L.rife_hip_last_error().decode()
            assert rc == -amd.ENOSYS and word in msg and "planar RGB" in msg, (rc, msg)
            assert same(out, keep), "the output buffer was written"
        with pytest.raises(amd.RifeError) as ex:
            e.upload_planes(a, px)
        assert "(-6)" in str(ex.value)
        d0, d1, do = _dev(a), _dev(b), _dev(out)
        torch.cuda.synchronize()
        with pytest.raises(amd.RifeError) as ex:
            e.process_device(d0.data_ptr(), d1.data_ptr(), w, h, 0.5, do.data_ptr(), None, pixfmt=px)
        assert "(-6)" in str(ex.value)
        with pytest.raises(amd.RifeError) as ex:
            e.process_device_batch([d0.data_ptr()] * 2, [d1.data_ptr()] * 2, w, h, [0.5, 0.3], [do.data_ptr()] * 2, None, pixfmt=px)
        assert "(-6)" in str(ex.value)
        torch.cuda.synchronize()
        assert same(_host(do, out), keep)
        pa, pb, po = Planes(w, h, px, "a64", a), Planes(w, h, px, "a64", b), Planes(w, h, px, "a64")
        with pytest.raises(amd.RifeError) as ex:
            e.process_planes(pa.views(), pb.views(), 0.5, px, out=po.views())
        assert "(-6)" in str(ex.value) and word in str(ex.value), str(ex.value)
        assert po.intact() and (po.gather().view(np.uint8) == FILL).all()
        da, db, dd = DevicePlanes(pa), DevicePlanes(pb), DevicePlanes(Planes(w, h, px, "a64"))
        torch.cuda.synchronize()
        with pytest.raises(amd.RifeError) as ex:
            e.process_device_image(da.desc, db.desc, 0.5, dd.desc, None)
        assert "(-6)" in str(ex.value)
        torch.cuda.synchronize()
        assert dd.fetch().intact() and (dd.pl.gather().view(np.uint8) == FILL).all()


def test_a_colour_description_and_the_even_slots_are_einval(g):
    import torch
    L = g._L
    w, h = 32, 32
    bad = [(P8 | amd.CSP_BT601, "colour description"), (PF | amd.CSP_FULL, "colour description"), (PH | amd.CSP_BT2020NCL, "colour description"),
           (P10 | (1 << 13), "unknown"), (64, "unknown"), (66, "unknown"), (68, "unknown"), (70, "unknown"), (72, "unknown"), (73, "unknown")]
    for px, word in bad:
        n = 12 * w * h
        a = np.zeros(n, np.uint8); out = np.full(n, 0x5a, np.uint8)
        assert L.rife_hip_process_px(g._h, a.ctypes.data, a.ctypes.data, w, h, ctypes.c_float(0.5), out.ctypes.data, px) == -amd.EINVAL, hex(px)
        assert word in L.rife_hip_last_error().decode(), (hex(px), L.rife_hip_last_error().decode())
        assert (out == 0x5a).all()
        f = ctypes.c_void_p()
        assert L.rife_hip_frame_upload_px(g._h, a.ctypes.data, w, h, px, ctypes.byref(f)) == -amd.EINVAL and not f.value
        d = torch.full((n,), 0x5a, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.rife_hip_process_device_px(g._h, d.data_ptr(), d.data_ptr(), w, h, ctypes.c_float(0.5), d.data_ptr(), px, None) == -amd.EINVAL
        pa = (ctypes.c_void_p * 1)(d.data_ptr())
        assert L.rife_hip_process_device_batch_px(g._h, 1, pa, pa, (ctypes.c_float * 1)(0.5), pa, w, h, px, None) == -amd.EINVAL
        im = amd.device_image(w, h, px, [(d.data_ptr(), 128), (d.data_ptr() + 4096, 128), (d.data_ptr() + 8192, 128)])
        assert L.rife_hip_process_device_image(g._h, ctypes.byref(im), ctypes.byref(im), ctypes.c_float(0.5), ctypes.byref(im), None) == -amd.EINVAL
        torch.cuda.synchronize()
        assert (d == 0x5a).all().item()


# ---- 7. against the reference network -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", FORMATS, ids=_id)
def test_against_the_reference_network_within_one_code(g, modeldirs, px):
    """At most 1 ten-bit code per sample after to10 (RGBP8: at most 1 eight-bit code, since one ten-bit code moves c >> 2 by at most one).  This IS the engine's
    existing depth-10 bound - the conversions are exact - so the case guards the wiring and sets no tolerance of its own."""
    o = _oracle(modeldirs)
    w, h = 96, 64
    a, b = frames(w, h, px)
    rc, got = process_px(g, a, b, 0.5, px)
    assert rc == 0
    want10 = deep_ref.expected_frame(o, pr.to_rgb10(a, px), pr.to_rgb10(b, px), 0.5)      # (h, w, 3) ten-bit codes
    if px == P8:
        d = np.abs(got.astype(np.int32) - pr.from_rgb10(want10, px).astype(np.int32))
    else:
        d = np.abs(pr.to_rgb10(got, px).astype(np.int32) - want10.astype(np.int32))
    print("%s %dx%d: exact %.6f, off by one %.6f, max %d" % (_id(px), w, h, (d == 0).mean(), (d == 1).mean(), d.max()))
    assert d.max() <= 1


_ORACLE = []


def _oracle(modeldirs):
    if not _ORACLE:
        o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(modeldirs["rife-v4.6"])
        _ORACLE.append(o)
    return _ORACLE[0]
