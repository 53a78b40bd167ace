"""The 4:2:0 Y'CbCr specification itself (tests/yuv_ref.py = include/rife_hip.h "YUV"), on the CPU: accuracy of the integer forward conversion, the exact
round trip YUV -> RGB10 -> YUV that lets 8- and 10-bit YUV ride the depth-10 path, the sensitivity that carries the engine's 1-code contract across, and the
frame geometry.  No GPU, no library."""
import numpy as np
import pytest

import yuv_ref as yr

N = 2_000_000
# every colour description the engine serves: three matrices x {limited, full} at 8 bits, limited at 10
SERVED = [(yr.PIX_NV12, m | f) for m in yr.MATRICES for f in (0, yr.CSP_FULL)] + [(yr.PIX_P010, m) for m in yr.MATRICES]
IDS = ["%s-%s-%s" % ("d8" if yr.depth(p) == 8 else "d10", {0: "709", 256: "601", 512: "2020"}[c & 0xf00], "full" if c & yr.CSP_FULL else "limited") for p, c in SERVED]


def _samples(pixfmt, seed):
    """N random (Y, Cb, Cr) code triples over the whole code range, as a frame of N x 1 blocks... kept as three flat arrays."""
    rng = np.random.default_rng(seed)
    top = 1024 if yr.depth(pixfmt) == 10 else 256
    return rng.integers(0, top, N, dtype=np.int32), rng.integers(0, top, N, dtype=np.int32), rng.integers(0, top, N, dtype=np.int32)


def _fwd(y, cb, cr, pixfmt):
    """The integer forward conversion on flat sample arrays, unclamped (yuv_ref.yuv_to_rgb10 without the frame geometry)."""
    k = yr.coefs(pixfmt)
    yy = k["iy"] * (y - k["yoff"]); u = cb - k["coff"]; v = cr - k["coff"]
    return np.stack([(yy + k["irv"] * v + 0x8000) >> 16, (yy + k["igu"] * u + k["igv"] * v + 0x8000) >> 16, (yy + k["ibu"] * u + 0x8000) >> 16], axis=-1)


def _back(rgb, pixfmt):
    """The integer backward conversion of single pixels (n = 1 blocks)."""
    k = yr.coefs(pixfmt)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = np.clip(((k["oyr"] * r + k["oyg"] * g + k["oyb"] * b + 0x8000) >> 16) + k["yoff"], 0, k["maxv"])
    u = np.clip(((k["our"] * r + k["oug"] * g + k["oub"] * b + 0x8000) >> 16) + k["coff"], 0, k["maxv"])
    v = np.clip(((k["ovr"] * r + k["ovg"] * g + k["ovb"] * b + 0x8000) >> 16) + k["coff"], 0, k["maxv"])
    return y, u, v


@pytest.mark.parametrize("fmt,csp", SERVED, ids=IDS)
def test_forward_against_real_formula(fmt, csp):
    px = fmt | csp
    y, cb, cr = _samples(px, 1)
    got = _fwd(y, cb, cr, px)
    want = yr.yuv_to_rgb10_real(y, cb, cr, px)
    err = np.abs(got - want).max()
    print("forward %s: max |integer - real| = %.4f codes" % (hex(px), err))
    assert err <= 0.52


@pytest.mark.parametrize("fmt,csp", SERVED, ids=IDS)
def test_round_trip_is_identity_in_gamut(fmt, csp):
    px = fmt | csp
    y, cb, cr = _samples(px, 2)
    rgb = _fwd(y, cb, cr, px)
    ok = ((rgb >= 0) & (rgb <= 1023)).all(axis=-1)
    assert ok.sum() > N // 20
    y2, u2, v2 = _back(rgb[ok], px)
    d = max(np.abs(y2 - y[ok]).max(), np.abs(u2 - cb[ok]).max(), np.abs(v2 - cr[ok]).max())
    print("round trip %s: %d in-gamut samples, max difference %d" % (hex(px), ok.sum(), d))
    assert d == 0


@pytest.mark.parametrize("fmt,csp", SERVED, ids=IDS)
def test_sensitivity_one_code(fmt, csp):
    """RGB codes perturbed by +-1 per channel move no Y, Cb, Cr by more than 1: the engine's 1-code bound on RGB10 is a 1-code bound on YUV."""
    px = fmt | csp
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 1024, (N, 3), dtype=np.int32)
    pert = np.clip(rgb + rng.integers(-1, 2, (N, 3), dtype=np.int32), 0, 1023)
    a = _back(rgb, px); b = _back(pert, px)
    d = max(np.abs(p - q).max() for p, q in zip(a, b))
    assert d <= 1


def test_ten_bit_full_range_is_not_served():
    """... because its round trip is not exact (1 code off on a few samples per million): the engine refuses it (tests/test_gpu_yuv.py checks the value)."""
    for f in (yr.PIX_P010, yr.PIX_I420P10):
        assert not yr.served(f | yr.CSP_FULL)
        assert yr.served(f) and yr.served(f | yr.CSP_BT2020NCL)
    assert yr.served(yr.PIX_NV12 | yr.CSP_FULL | yr.CSP_BT601)
    assert not yr.served(yr.PIX_NV12 | (3 << 8))


def _frame_from_rgb(w, h, px, seed):
    """An in-gamut YUV frame: made from RGB (codes 16..1007: quantising to YUV moves a colour by a few codes, and one at the very edge of the cube may land
    outside it), with whole 2x2 blocks of one colour so that replication gives back what the box average took."""
    rng = np.random.default_rng(seed)
    cw, ch = yr.chroma_dims(w, h)
    blocks = rng.integers(16, 1008, (ch, cw, 3), dtype=np.int32)
    rgb = np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)[:h, :w]
    return yr.rgb10_to_yuv(rgb, px)


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (33, 47), (8, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", yr.FORMATS, ids=["nv12", "i420", "p010", "i420p10"])
def test_whole_frames_round_trip(fmt, size):
    w, h = size
    for csp in [m | f for m in yr.MATRICES for f in ((0, yr.CSP_FULL) if yr.depth(fmt) == 8 else (0,))]:
        px = fmt | csp
        f = _frame_from_rgb(w, h, px, 7 + w)
        assert f.dtype == yr.dtype(px) and f.size == yr.frame_elems(w, h)
        assert not yr.clamped(f, w, h, px).any()
        back = yr.rgb10_to_yuv(yr.yuv_to_rgb10(f, w, h, px), px)
        assert np.array_equal(back, f), "round trip of a %dx%d %s frame" % (w, h, hex(px))


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (33, 47), (640, 360)], ids=lambda s: "%dx%d" % s)
def test_frame_bytes_and_plane_offsets(size):
    w, h = size
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert yr.frame_bytes(w, h, yr.PIX_NV12) == w * h + 2 * cw * ch == yr.frame_bytes(w, h, yr.PIX_I420)
    assert yr.frame_bytes(w, h, yr.PIX_P010) == 2 * (w * h + 2 * cw * ch) == yr.frame_bytes(w, h, yr.PIX_I420P10 | yr.CSP_BT601)
    assert yr.plane_offsets(w, h, yr.PIX_NV12) == (0, w * h) == yr.plane_offsets(w, h, yr.PIX_P010)
    assert yr.plane_offsets(w, h, yr.PIX_I420) == (0, w * h, w * h + cw * ch) == yr.plane_offsets(w, h, yr.PIX_I420P10)


@pytest.mark.parametrize("fmt", yr.FORMATS, ids=["nv12", "i420", "p010", "i420p10"])
def test_pack_and_split_invert_each_other(fmt):
    rng = np.random.default_rng(11)
    for w, h in [(1, 1), (3, 5), (8, 6), (33, 47)]:
        cw, ch = yr.chroma_dims(w, h)
        top = 1024 if yr.depth(fmt) == 10 else 256
        y = rng.integers(0, top, (h, w), dtype=np.int32); cb = rng.integers(0, top, (ch, cw), dtype=np.int32); cr = rng.integers(0, top, (ch, cw), dtype=np.int32)
        f = yr.pack(y, cb, cr, fmt)
        y2, cb2, cr2 = yr.split(f, w, h, fmt)
        assert np.array_equal(y, y2) and np.array_equal(cb, cb2) and np.array_equal(cr, cr2)
        assert np.array_equal(yr.pack(y2, cb2, cr2, fmt), f)
        if fmt == yr.PIX_P010:
            assert not (f & 63).any()
            assert np.array_equal(yr.canonical(f | 63, w, h, fmt), f)        # input low bits are ignored, output low bits are zero
        # the two layouts of one depth hold the same samples
        other = {yr.PIX_NV12: yr.PIX_I420, yr.PIX_I420: yr.PIX_NV12, yr.PIX_P010: yr.PIX_I420P10, yr.PIX_I420P10: yr.PIX_P010}[fmt]
        g = yr.pack(y, cb, cr, other)
        assert all(np.array_equal(p, q) for p, q in zip(yr.split(g, w, h, other), (y, cb, cr)))


def test_format_numbers_leave_5_to_15_reserved():
    """The 4:2:0 formats are 16 + 2 * (10 bits) + (planar); 3 and 5 .. 15 stay unknown formats (tests/test_alpha_host.py and tests/test_deep_host.py use 5 and 7 as
    their examples of one), and the header, the Python mirror and this file agree."""
    import importlib
    import os
    import re
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    assert (yr.PIX_NV12, yr.PIX_I420, yr.PIX_P010, yr.PIX_I420P10) == (16, 17, 18, 19) == (amd.PIX_NV12, amd.PIX_I420, amd.PIX_P010, amd.PIX_I420P10)
    assert (yr.CSP_BT709, yr.CSP_BT601, yr.CSP_BT2020NCL, yr.CSP_FULL) == (amd.CSP_BT709, amd.CSP_BT601, amd.CSP_BT2020NCL, amd.CSP_FULL) == (0, 256, 512, 4096)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rife_hip.h")).read()
    for name, v in (("NV12", 16), ("I420", 17), ("P010", 18), ("I420P10", 19)):
        assert re.search(r"#define RIFE_HIP_PIX_%s\s+%d\b" % (name, v), hdr), name
    for px in yr.FORMATS:
        assert yr.depth(px) == (10 if px & 2 else 8) and yr.planar(px) == bool(px & 1)
        assert amd.yuv_frame_bytes(33, 47, px | yr.CSP_BT601) == yr.frame_bytes(33, 47, px)
