"""4:2:2 / 4:4:4 Y'CbCr (RIFE_HIP_PIX_I422 / I422P10 / I444 / I444P10), the part that needs no device: the format numbers in the header, the Python mirror and
tests/chroma_ref.py; rife_hip_frame_bytes / rife_hip_image_row_bytes / rife_hip_image_check through ctypes on the PRODUCT library; and the specification
itself - the exact round trip YUV -> RGB10 -> YUV on 2x1 blocks that lets 4:2:2 ride the depth-10 path (4:4:4 is the n = 1 round trip of
tests/test_yuv_host.py), whole frames, and agreement with the 4:2:0 specification where the two overlap."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import chroma_ref as cr
import yuv_ref as yr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
N = 2_000_000
NAMES = {cr.PIX_I422: "i422", cr.PIX_I422P10: "i422p10", cr.PIX_I444: "i444", cr.PIX_I444P10: "i444p10"}
SIZES = [(1, 1), (2, 1), (3, 5), (33, 47), (640, 360)]
# every colour description the engine serves: three matrices x {limited, full} at 8 bits, limited at 10
SERVED = [cr.PIX_I422 | m | f for m in cr.MATRICES for f in (0, cr.CSP_FULL)] + [cr.PIX_I422P10 | m for m in cr.MATRICES]


def _id(px):
    return "%s-%s-%s" % (NAMES[px & 0xff], {0: "709", 1: "601", 2: "2020"}[(px >> 8) & 15], "full" if px & cr.CSP_FULL else "limited")


def check(img):
    L = amd.lib()
    rc = L.rife_hip_image_check(ctypes.byref(img))
    return rc, L.rife_hip_last_error().decode()


def refused(img, word):
    rc, msg = check(img)
    assert rc == -1 and word in msg, (rc, msg)      # -RIFE_HIP_EINVAL


def good(px, w=33, h=47, pad=8):
    """A descriptor over three host planes with `pad` bytes of row padding each."""
    es = 2 if cr.depth(px) == 10 else 1
    cw, ch = cr.chroma_dims(w, h, px)
    bufs = [np.zeros((h, w * es + pad), np.uint8), np.zeros((ch, cw * es + pad), np.uint8), np.zeros((ch, cw * es + pad), np.uint8)]
    im = amd.device_image(w, h, px, [(b.ctypes.data, b.strides[0]) for b in bufs])
    im._keep = bufs
    return im


# ---- format numbers -----------------------------------------------------------------------------------------------------------------------------------

def test_format_numbers():
    want = (33, 35, 49, 51)
    assert cr.FORMATS == want == (amd.PIX_I422, amd.PIX_I422P10, amd.PIX_I444, amd.PIX_I444P10)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rife_hip.h")).read()
    for name, v in zip(("I422", "I422P10", "I444", "I444P10"), want):
        assert re.search(r"#define RIFE_HIP_PIX_%s\s+%d\b" % (name, v), hdr), name
    # 16 * class + 2 * (10 bits) + planar
    for px, cls, d in zip(want, (2, 2, 3, 3), (8, 10, 8, 10)):
        assert px >> 4 == cls == cr.chroma_class(px) and bool(px & 2) == (d == 10) and px & 1 == 1
        assert cr.depth(px) == d and np.dtype(amd.yuv_dtype(px)) == np.dtype(cr.dtype(px))
        assert amd.frame_bytes(33, 47, px) == cr.frame_bytes(33, 47, px) > 0
    for px in yr.FORMATS:
        assert px >> 4 == 1


@pytest.mark.parametrize("px", [20, 32, 34, 48, 50, 52])
def test_neighbouring_numbers_stay_unknown(px):
    """20 is the existing tests' example of an unknown format; 32, 34, 48, 50 are the semi-planar slots (NV16 / P210 / NV24 / P410)."""
    assert amd.frame_bytes(33, 47, px) == 0
    for p in range(3):
        assert amd.image_row_bytes(33, px, p) == 0
    im = good(cr.PIX_I444); im.pixfmt = px
    refused(im, "unknown pixel format")
    with pytest.raises(ValueError):
        amd.yuv_frame_bytes(33, 47, px)


# ---- frame bytes and plane offsets, C against numpy ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("px", cr.FORMATS, ids=_id)
def test_frame_bytes_and_plane_offsets(px, size):
    w, h = size
    es = 2 if cr.depth(px) == 10 else 1
    cw = (w + 1) // 2 if px >> 4 == 2 else w
    assert cr.chroma_dims(w, h, px) == (cw, h) == amd.yuv_chroma_dims(w, h, px)
    assert cr.frame_elems(w, h, px) == w * h + 2 * cw * h
    assert amd.frame_bytes(w, h, px) == amd.frame_bytes(w, h, px | cr.CSP_BT601) == cr.frame_bytes(w, h, px) == amd.yuv_frame_bytes(w, h, px) == es * (w * h + 2 * cw * h)
    assert cr.plane_offsets(w, h, px) == (0, w * h, w * h + cw * h)
    # the rows of the planes, glued, are the frame: row bytes per plane from the library, h rows each
    rb = [amd.image_row_bytes(w, px, p) for p in range(4)]
    assert rb == [w * es, cw * es, cw * es, 0]
    assert sum(rb) * h == amd.frame_bytes(w, h, px)
    # a tight image is accepted, and its planes sit at the reference's offsets
    buf = np.zeros(cr.frame_bytes(w, h, px), np.uint8)
    im = amd.device_image(w, h, px, [(buf.ctypes.data + o * es, r) for o, r in zip(cr.plane_offsets(w, h, px), rb)])
    assert check(im)[0] == 0, check(im)


# ---- image rules ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", cr.FORMATS, ids=_id)
def test_image_rules(px):
    w, h = 33, 47
    es = 2 if cr.depth(px) == 10 else 1
    assert check(good(px))[0] == 0 and check(good(px | cr.CSP_BT2020NCL))[0] == 0
    for p in range(3):
        rb = amd.image_row_bytes(w, px, p)
        im = good(px); im.pitch[p] = rb - es
        refused(im, "plane %d: the pitch (%d) is smaller than the row bytes (%d)" % (p, rb - es, rb))
        im = good(px); im.pitch[p] = rb                                # the smallest pitch that passes
        assert check(im)[0] == 0
        im = good(px); im.plane[p] = None
        refused(im, "plane %d is NULL" % p)
        if es == 2:
            im = good(px); im.pitch[p] = rb + 65                       # odd
            refused(im, "not a multiple of the element size (2)")
            im = good(px); im.plane[p] = im.plane[p] + 1
            refused(im, "not aligned to the element size (2)")
        else:
            im = good(px); im.pitch[p] = rb + 65; im.plane[p] = im.plane[p] + 1
            assert check(im)[0] == 0
    im = good(px); im.pixfmt = px | cr.CSP_FULL
    if es == 2:
        refused(im, "full-range")
        assert not cr.served(px | cr.CSP_FULL)
    else:
        assert check(im)[0] == 0 and cr.served(px | cr.CSP_FULL)
    im = good(px); im.pixfmt = px | (3 << 8)
    refused(im, "unknown colour matrix")
    im = good(px); im.pixfmt = px | (1 << 13)
    refused(im, "unknown pixel format")


def test_plane_tuples_of_the_mirror():
    w, h = 33, 47
    y = np.zeros((h, 64), np.uint8)[:, :w]
    im = amd.planes_image((y, np.zeros((h, 32), np.uint8)[:, :17], np.zeros((h, 17), np.uint8)), w, h, amd.PIX_I422 | amd.CSP_BT601)
    assert [im.pitch[i] for i in range(3)] == [64, 32, 17] and check(im)[0] == 0
    y16 = np.zeros((h, w), np.uint16)
    im = amd.planes_image((y16, np.zeros((h, 40), np.uint16)[:, :w], y16.copy()), w, h, amd.PIX_I444P10)
    assert [im.pitch[i] for i in range(3)] == [66, 80, 66] and check(im)[0] == 0
    with pytest.raises(ValueError):
        amd.planes_image((y, np.zeros((24, 17), np.uint8), np.zeros((24, 17), np.uint8)), w, h, amd.PIX_I422)      # 4:2:0 chroma rows
    with pytest.raises(ValueError):
        amd.planes_image((y, np.zeros((h, 17), np.uint8), np.zeros((h, 17), np.uint8)), w, h, amd.PIX_I444)


# ---- the 4:2:2 round trip --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", SERVED, ids=_id)
def test_422_round_trip_is_identity_in_gamut(px):
    """Y0, Y1, Cb, Cr -> two 10-bit RGB pixels -> Y, Y, Cb, Cr with the chroma back through the summed form (+ 0x10000 >> 17): N random 2x1 blocks with
    independent luma, as one 2N x 1 frame; identity on every block neither of whose pixels clamped."""
    rng = np.random.default_rng(2)
    top = 1024 if cr.depth(px) == 10 else 256
    f = rng.integers(0, top, 4 * N).astype(cr.dtype(px))              # Y 2N, Cb N, Cr N
    w, h = 2 * N, 1
    ok = ~cr.clamped(f, w, h, px).reshape(N, 2).any(axis=1)
    assert ok.sum() > N // 20
    back = cr.rgb10_to_yuv(cr.yuv_to_rgb10(f, w, h, px), px)
    y0, cb0, cr0 = cr.split(f, w, h, px)
    y1, cb1, cr1 = cr.split(back, w, h, px)
    dy = np.abs(y1 - y0).reshape(N, 2)[ok].max(); dcb = np.abs(cb1 - cb0).reshape(N)[ok].max(); dcr = np.abs(cr1 - cr0).reshape(N)[ok].max()
    print("4:2:2 round trip %s: %d in-gamut blocks, max difference Y %d Cb %d Cr %d" % (_id(px), ok.sum(), dy, dcb, dcr))
    assert max(dy, dcb, dcr) == 0


# ---- whole frames ------------------------------------------------------------------------------------------------------------------------------------------

def _frame_from_rgb(w, h, px, seed):
    """An in-gamut frame: made from RGB codes 16..1007 that are constant per chroma block (2x1, or the pixel), so that replication gives back what the sum took."""
    rng = np.random.default_rng(seed)
    cw, ch = cr.chroma_dims(w, h, px)
    blocks = rng.integers(16, 1008, (ch, cw, 3), dtype=np.int32)
    return cr.rgb10_to_yuv(np.repeat(blocks, cr.subx(px), axis=1)[:, :w], px)


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (33, 47), (8, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", cr.FORMATS, ids=_id)
def test_whole_frames_round_trip(fmt, size):
    w, h = size
    for csp in [m | f for m in cr.MATRICES for f in ((0, cr.CSP_FULL) if cr.depth(fmt) == 8 else (0,))]:
        px = fmt | csp
        f = _frame_from_rgb(w, h, px, 7 + w)
        assert f.dtype == cr.dtype(px) and f.size == cr.frame_elems(w, h, px)
        assert not cr.clamped(f, w, h, px).any()
        back = cr.rgb10_to_yuv(cr.yuv_to_rgb10(f, w, h, px), px)
        assert np.array_equal(back, f), "round trip of a %dx%d %s frame" % (w, h, _id(px))


@pytest.mark.parametrize("fmt", cr.FORMATS, ids=_id)
def test_pack_and_split_invert_each_other(fmt):
    rng = np.random.default_rng(11)
    for w, h in [(1, 1), (3, 5), (8, 6), (33, 47)]:
        cw, ch = cr.chroma_dims(w, h, fmt)
        top = 1024 if cr.depth(fmt) == 10 else 256
        y = rng.integers(0, top, (h, w), dtype=np.int32); cb = rng.integers(0, top, (ch, cw), dtype=np.int32); cr_ = rng.integers(0, top, (ch, cw), dtype=np.int32)
        f = cr.pack(y, cb, cr_, fmt)
        got = cr.split(f, w, h, fmt)
        assert all(np.array_equal(p, q) for p, q in zip(got, (y, cb, cr_)))
        assert np.array_equal(cr.pack(*got, fmt), f) and np.array_equal(cr.canonical(f, w, h, fmt), f)
        if cr.depth(fmt) == 10:                                        # a larger value is read as 1023
            big = f.copy(); big[::3] |= np.uint16(0xfc00)
            assert np.array_equal(cr.canonical(big, w, h, fmt), np.minimum(big, 1023)) and not np.array_equal(cr.canonical(big, w, h, fmt), big)


# ---- the two specifications agree where they overlap ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d10", [False, True], ids=["d8", "d10"])
def test_444_with_replicated_420_chroma_is_the_420_frame(d10):
    f420, f422, f444 = (yr.PIX_I420P10, cr.PIX_I422P10, cr.PIX_I444P10) if d10 else (yr.PIX_I420, cr.PIX_I422, cr.PIX_I444)
    rng = np.random.default_rng(5)
    for (w, h) in [(1, 1), (3, 5), (33, 47), (8, 2)]:
        for csp in cr.MATRICES + (() if d10 else (cr.CSP_FULL | cr.CSP_BT601,)):
            f = rng.integers(0, 1024 if d10 else 256, yr.frame_elems(w, h)).astype(yr.dtype(f420))
            y, cb, cr_ = yr.split(f, w, h, f420)
            want = yr.yuv_to_rgb10(f, w, h, f420 | csp)
            full = cr.pack(y, np.repeat(np.repeat(cb, 2, axis=0), 2, axis=1)[:h, :w], np.repeat(np.repeat(cr_, 2, axis=0), 2, axis=1)[:h, :w], f444)
            assert np.array_equal(cr.yuv_to_rgb10(full, w, h, f444 | csp), want)
            half = cr.pack(y, np.repeat(cb, 2, axis=0)[:h], np.repeat(cr_, 2, axis=0)[:h], f422)      # chroma rows doubled, columns kept
            assert np.array_equal(cr.yuv_to_rgb10(half, w, h, f422 | csp), want)
