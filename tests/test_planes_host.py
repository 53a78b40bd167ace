"""Strided frames and separate planes (include/rife_hip.h rife_hip_image_t), the part that needs no device: rife_hip_image_check / rife_hip_image_row_bytes
through ctypes on the PRODUCT library, the numpy helper tests/planes_ref.py, and the numpy-view detection of the Python mirror."""
import ctypes
import importlib

import numpy as np
import pytest

import planes_ref as pr
import yuv_ref as yr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
U16_FORMATS = (amd.PIX_RGB10_U16, amd.PIX_P010, amd.PIX_I420P10)


def _id(px):
    return pr.FMT_NAME[px & 0xff]


def check(img):
    """(rc, message) of rife_hip_image_check on the product library."""
    L = amd.lib()
    rc = L.rife_hip_image_check(ctypes.byref(img))
    return rc, L.rife_hip_last_error().decode()


def good(px, w=33, h=47, pitches="a64"):
    tight = np.zeros(pr.frame_bytes(w, h, px), np.uint8)
    return pr.to_image(tight, w, h, px, pitches)


def refused(img, word):
    rc, msg = check(img)
    assert rc == -1 and word in msg, (rc, msg)      # -RIFE_HIP_EINVAL


# ---- rife_hip_image_check -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
@pytest.mark.parametrize("w,h", [(1, 1), (33, 47)])
def test_every_format_is_accepted(px, w, h):
    for pitches in pr.LAYOUTS:
        im = good(px | (amd.CSP_BT601 if pr.is_yuv(px) else 0), w, h, pitches)
        assert check(im.desc)[0] == 0, (pitches, check(im.desc))
    if px == amd.PIX_NV12:
        assert check(good(px | amd.CSP_FULL | amd.CSP_BT2020NCL, w, h).desc)[0] == 0


@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_a_null_plane_is_refused(px):
    for p in range(len(pr.plane_table(33, 47, px))):
        im = good(px)
        im.desc.plane[p] = None
        refused(im.desc, "plane %d is NULL" % p)
    im = good(px)                                     # entries the format does not use are ignored
    for p in range(len(pr.plane_table(33, 47, px)), 3):
        im.desc.plane[p] = None; im.desc.pitch[p] = -7
    assert check(im.desc)[0] == 0


@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_pitch_rules(px):
    for p, (rows, rb, _, _) in enumerate(pr.plane_table(33, 47, px)):
        im = good(px); im.desc.pitch[p] = rb - 1
        refused(im.desc, "smaller than the row bytes")
        im = good(px); im.desc.pitch[p] = -im.desc.pitch[p]
        refused(im.desc, "negative")
        im = good(px); im.desc.pitch[p] = 0
        refused(im.desc, "zero")
        im = good(px); im.desc.pitch[p] = 2 ** 31
        refused(im.desc, "INT32_MAX")
        im = good(px); im.desc.pitch[p] = (2 ** 31 - 1) // pr.elem_size(px) * pr.elem_size(px)      # the largest pitch that passes
        assert check(im.desc)[0] == 0
        im = good(px); im.desc.pitch[p] = rb                                                        # the smallest
        assert check(im.desc)[0] == 0


@pytest.mark.parametrize("px", U16_FORMATS + (amd.PIX_A2B10G10R10,), ids=_id)
def test_element_size_rules(px):
    es = pr.elem_size(px)
    for p, (rows, rb, _, _) in enumerate(pr.plane_table(33, 47, px)):
        im = good(px); im.desc.pitch[p] = rb + 65                      # odd
        refused(im.desc, "not a multiple of the element size (%d)" % es)
        im = good(px); im.desc.plane[p] = im.desc.plane[p] + 1         # odd pointer
        refused(im.desc, "not aligned to the element size (%d)" % es)
    if es == 4:
        im = good(px); im.desc.pitch[0] = 33 * 4 + 2                   # even, but no multiple of 4
        refused(im.desc, "not a multiple of the element size (4)")
        im = good(px); im.desc.plane[0] = im.desc.plane[0] + 2
        refused(im.desc, "not aligned to the element size (4)")


def test_sizes_and_formats():
    for w, h in [(0, 4), (4, 0), (-1, 4)]:
        im = good(amd.PIX_RGB8); im.desc.w = w; im.desc.h = h
        refused(im.desc, "bad frame size")
    for px in (3, 5, 7, 20, -1, amd.PIX_NV12 | (1 << 13)):
        im = good(amd.PIX_RGB8); im.desc.pixfmt = px
        refused(im.desc, "unknown pixel format")
    for px in (amd.PIX_RGB8, amd.PIX_RGB10_U16, amd.PIX_A2B10G10R10, amd.PIX_RGBA8):
        im = good(px); im.desc.pixfmt = px | amd.CSP_BT601
        refused(im.desc, "colour description")
    for px in (amd.PIX_P010, amd.PIX_I420P10):
        im = good(px); im.desc.pixfmt = px | amd.CSP_FULL
        refused(im.desc, "full-range")
    im = good(amd.PIX_NV12); im.desc.pixfmt = amd.PIX_NV12 | (3 << 8)
    refused(im.desc, "unknown colour matrix")
    assert amd.lib().rife_hip_image_check(None) == -1


# ---- rife_hip_image_row_bytes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_row_bytes_equal_the_frame_arithmetic(px):
    for w in (1, 2, 3, 33):
        table = pr.plane_table(w, 5, px)
        for p in range(4):
            want = table[p][1] if p < len(table) else 0
            assert amd.image_row_bytes(w, px, p) == want, (w, p)
            assert amd.image_row_bytes(w, px | (amd.CSP_BT601 if pr.is_yuv(px) else 0), p) == want
        # the planes of the tight frame add up to the frame of the _px calls
        assert sum(rows * rb for (rows, rb, _, _) in table) == amd.frame_bytes(w, 5, px) == (yr.frame_bytes(w, 5, px) if pr.is_yuv(px) else w * 5 * pr.RGB_BPP[px])
    assert amd.image_row_bytes(0, px, 0) == 0 and amd.image_row_bytes(33, px, -1) == 0
    assert amd.image_row_bytes(33, 7, 0) == 0


# ---- tests/planes_ref.py ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.ALL_FORMATS, ids=_id)
def test_to_image_and_from_image_invert_each_other(px):
    rng = np.random.default_rng(7)
    for (w, h) in [(1, 1), (3, 5), (33, 47), (64, 34)]:
        tight = rng.integers(0, 256, pr.frame_bytes(w, h, px), dtype=np.uint8)
        tight[tight == 0xC5] = 0                                                     # so that a window byte is never mistaken for a canary below
        for pitches in pr.LAYOUTS + ([pr.row_bytes(w, px, p) + 8 for p in range(3)],):
            im = pr.to_image(tight, w, h, px, pitches)
            assert np.array_equal(pr.from_image(im), tight), pitches
            assert im.canaries_intact()
            for bi, buf in enumerate(im.bufs):                                       # the windows hold the frame and nothing else does
                assert int(im.window_mask(bi).sum()) <= tight.size and not (buf[im.window_mask(bi)] == 0xC5).any()
            assert sum(int(im.window_mask(bi).sum()) for bi in range(len(im.bufs))) == tight.size
            assert check(im.desc)[0] == 0
            if pitches != "tight" and len(im.bufs) == 1 and im.bufs[0].size > tight.size:
                k = int(np.flatnonzero(~im.window_mask(0))[0])
                im.bufs[0][k] ^= 0xff
                assert not im.canaries_intact()
    t3 = np.arange(pr.frame_bytes(4, 4, amd.PIX_I420), dtype=np.uint8)
    sw = pr.swap_chroma(t3, 4, 4, amd.PIX_I420)
    assert np.array_equal(sw[:16], t3[:16]) and np.array_equal(sw[16:20], t3[20:24]) and np.array_equal(sw[20:24], t3[16:20])
    assert np.array_equal(pr.swap_chroma(t3[:24], 4, 4, amd.PIX_NV12), t3[:24])


def test_layouts_have_the_alignments_they_promise():
    for px in pr.ALL_FORMATS:
        es = pr.elem_size(px)
        tight = np.zeros(pr.frame_bytes(64, 34, px), np.uint8)
        a64 = pr.to_image(tight, 64, 34, px, "a64").desc
        elem = pr.to_image(tight, 64, 34, px, "elem").desc
        for p in range(len(pr.plane_table(64, 34, px))):
            assert a64.plane[p] % 64 == 0 and a64.pitch[p] % 64 == 0
            assert elem.plane[p] % 64 == es and elem.pitch[p] == pr.row_bytes(64, px, p) + es
        win = pr.to_image(tight, 64, 34, px, "window")
        (_, off, pitch, rows, rb, _) = win.planes[0]
        assert pitch >= 2 * rb and win.bufs[0].size >= off + 2 * rows * pitch - 3 * pitch


# ---- the Python mirror: which arrays go to the library without a copy -----------------------------------------------------------------------------------

def test_numpy_view_detection():
    big = np.zeros((100, 120, 3), np.uint8)
    crop = big[3:50, 5:38]
    im = amd.image_of(crop)
    assert (im.w, im.h, im.pixfmt) == (33, 47, amd.PIX_RGB8)
    assert im.plane[0] == big.ctypes.data + 3 * 360 + 5 * 3 and im.pitch[0] == 360
    assert check(im)[0] == 0
    padded = np.zeros((47, 128), np.uint8)[:, :99].reshape(47, 33, 3)                # rows padded to 128 bytes
    assert not padded.flags.c_contiguous
    im = amd.image_of(padded)
    assert im.pitch[0] == 128 and im.plane[0] == padded.ctypes.data and (im.w, im.h) == (33, 47)
    # other formats: dtype and shape select them, as in process()
    d16 = np.zeros((20, 40, 3), np.uint16)[2:12, 4:20]
    im = amd.image_of(d16)
    assert (im.pixfmt, im.w, im.h, im.pitch[0]) == (amd.PIX_RGB10_U16, 16, 10, 240)
    pk = np.zeros((20, 40), np.uint32)[2:12, 4:20]
    im = amd.image_of(pk)
    assert (im.pixfmt, im.w, im.h, im.pitch[0]) == (amd.PIX_A2B10G10R10, 16, 10, 160)
    rgba = np.zeros((20, 40, 4), np.uint8)[2:12, 4:20]
    im = amd.image_of(rgba)
    assert (im.pixfmt, im.pitch[0], im.plane[0] - rgba.base.ctypes.data) == (amd.PIX_RGBA8, 160, 2 * 160 + 16)
    # a contiguous array is its own tight image
    im = amd.image_of(np.zeros((4, 5, 3), np.uint8))
    assert im.pitch[0] == 15
    # anything else falls back to the contiguous copy of today
    assert amd.image_of(big[:, ::2]) is None                                         # column-strided
    assert amd.image_of(big[::-1]) is None                                           # bottom-up rows
    assert amd.image_of(big[:, :, ::-1]) is None                                     # BGR view
    assert amd.image_of(np.zeros((3, 10, 10), np.uint8).transpose(1, 2, 0)) is None  # planar RGB
    assert amd.image_of(np.zeros((10, 10, 3), np.float32)) is None
    assert amd.image_of(np.zeros((10, 10, 3), np.uint8)[::2]) is not None            # every other row IS a row stride (a field of an interlaced frame)
    assert amd.image_of(np.zeros((10, 10, 3), np.uint16)[:, :9]) is not None
    u16_odd_pitch = np.lib.stride_tricks.as_strided(np.zeros(400, np.uint16), shape=(5, 4, 3), strides=(25, 6, 2))
    assert amd.image_of(u16_odd_pitch) is None                                       # a pitch the element size does not divide: the library would refuse it


def test_plane_tuples():
    w, h = 33, 47
    y = np.zeros((h, 64), np.uint8)[:, :w]
    cb = np.zeros((24, 32), np.uint8)[:, :17]
    cr = np.zeros((24, 17), np.uint8)
    im = amd.planes_image((y, cb, cr), w, h, amd.PIX_I420 | amd.CSP_BT601)
    assert [im.pitch[i] for i in range(3)] == [64, 32, 17] and [im.plane[i] for i in range(3)] == [y.ctypes.data, cb.ctypes.data, cr.ctypes.data]
    assert check(im)[0] == 0
    uv = np.zeros((24, 64), np.uint16)[:, :34]
    im = amd.planes_image((np.zeros((h, w), np.uint16), uv), w, h, amd.PIX_P010)
    assert im.pitch[0] == 66 and im.pitch[1] == 128 and check(im)[0] == 0
    with pytest.raises(ValueError):
        amd.planes_image((y, cb), w, h, amd.PIX_I420)                                # a plane missing
    with pytest.raises(ValueError):
        amd.planes_image((y, cb, cr[:, ::-1]), w, h, amd.PIX_I420)                   # not row-strided
    with pytest.raises(ValueError):
        amd.planes_image((y, cb, cr.astype(np.uint16)), w, h, amd.PIX_I420)
    with pytest.raises(ValueError):
        amd.planes_image((y, cb, cr), w, h, amd.PIX_RGB8)
