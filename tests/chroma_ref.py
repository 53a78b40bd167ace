"""The specification of the 4:2:2 / 4:4:4 Y'CbCr boundary (include/rife_hip.h RIFE_HIP_PIX_I422 .. I444P10), once in numpy: what csrc/yuv.h k_preproc_yuvc /
k_postproc_yuvc restate in HIP.

Coefficients, offsets, clamps and colour bits are those of tests/yuv_ref.py (imported, not restated); ONLY THE BLOCK changes: 4:2:2 chroma belongs to a 2x1
block (cw = (w + 1) // 2, ch = h), 4:4:4 chroma to the pixel (cw = w, ch = h).  A call in one of these formats is, byte for byte,
    rgb10_to_yuv(process_px(yuv_to_rgb10(in0), yuv_to_rgb10(in1), t, A2B10G10R10)).
Frames are FLAT arrays (uint8 for I422 / I444, uint16 with the code in the low ten bits for I422P10 / I444P10): Y, then Cb, then Cr."""
import numpy as np

import yuv_ref as yr

PIX_I422, PIX_I422P10, PIX_I444, PIX_I444P10 = 33, 35, 49, 51
FORMATS = (PIX_I422, PIX_I422P10, PIX_I444, PIX_I444P10)
CSP_BT709, CSP_BT601, CSP_BT2020NCL, CSP_FULL = yr.CSP_BT709, yr.CSP_BT601, yr.CSP_BT2020NCL, yr.CSP_FULL
MATRICES = yr.MATRICES


def base(pixfmt):
    return pixfmt & 0xff


def chroma_class(pixfmt):
    """2 = 4:2:2, 3 = 4:4:4 (format = 16 * class + 2 * (10 bits) + planar)."""
    return base(pixfmt) >> 4


def depth(pixfmt):
    return 10 if base(pixfmt) & 2 else 8


def dtype(pixfmt):
    return np.uint16 if depth(pixfmt) == 10 else np.uint8


def served(pixfmt):
    return base(pixfmt) in FORMATS and (pixfmt & 0xf00) in MATRICES and not (pixfmt & ~0x1fff) and not (depth(pixfmt) == 10 and pixfmt & CSP_FULL)


def subx(pixfmt):
    """Pixels per chroma sample along a row: 2 (4:2:2) or 1 (4:4:4)."""
    return 2 if chroma_class(pixfmt) == 2 else 1


def chroma_dims(w, h, pixfmt):
    return (w + subx(pixfmt) - 1) // subx(pixfmt), h


def frame_elems(w, h, pixfmt):
    cw, ch = chroma_dims(w, h, pixfmt)
    return w * h + 2 * cw * ch


def frame_bytes(w, h, pixfmt):
    return frame_elems(w, h, pixfmt) * (2 if depth(pixfmt) == 10 else 1)


def plane_offsets(w, h, pixfmt):
    """Element offsets of Y, Cb, Cr in the flat frame."""
    cw, ch = chroma_dims(w, h, pixfmt)
    return 0, w * h, w * h + cw * ch


def coefs(pixfmt):
    """yuv_ref's Q16 coefficients for this depth and colour description (they do not depend on the chroma layout)."""
    return yr.coefs((pixfmt & ~0xff) | (yr.PIX_I420P10 if depth(pixfmt) == 10 else yr.PIX_I420))


def split(buf, w, h, pixfmt):
    """Flat frame -> (Y (h, w), Cb (h, cw), Cr (h, cw)) int32 CODES; a 10-bit sample above 1023 is read as 1023."""
    cw, ch = chroma_dims(w, h, pixfmt)
    a = np.asarray(buf).reshape(-1)
    assert a.dtype == dtype(pixfmt) and a.size == frame_elems(w, h, pixfmt), "a %dx%d frame of this format has %d %s elements" % (w, h, frame_elems(w, h, pixfmt), dtype(pixfmt).__name__)
    a = a.astype(np.int32)
    if depth(pixfmt) == 10:
        a = np.minimum(a, 1023)
    o = plane_offsets(w, h, pixfmt)
    return a[:o[1]].reshape(h, w).copy(), a[o[1]:o[2]].reshape(ch, cw).copy(), a[o[2]:].reshape(ch, cw).copy()


def pack(y, cb, cr, pixfmt):
    """Codes -> the flat frame."""
    return np.concatenate([np.asarray(p, np.int32).reshape(-1) for p in (y, cb, cr)]).astype(dtype(pixfmt))


def canonical(buf, w, h, pixfmt):
    """What timestep 0 / 1 return: bytes unchanged at 8 bits, u16 clamped to 1023 at 10 bits."""
    return pack(*split(buf, w, h, pixfmt), pixfmt)


def _unclamped(buf, w, h, pixfmt):
    k = coefs(pixfmt)
    y, cb, cr = split(buf, w, h, pixfmt)
    cb = np.repeat(cb, subx(pixfmt), axis=1)[:, :w] - k["coff"]      # the chroma of a pixel = the sample of its 2x1 block (4:4:4: its own)
    cr = np.repeat(cr, subx(pixfmt), axis=1)[:, :w] - k["coff"]
    yy = k["iy"] * (y - k["yoff"])
    return np.stack([(yy + k["irv"] * cr + 0x8000) >> 16, (yy + k["igu"] * cb + k["igv"] * cr + 0x8000) >> 16, (yy + k["ibu"] * cb + 0x8000) >> 16], axis=-1)


def yuv_to_rgb10(buf, w, h, pixfmt):
    """Flat YUV frame -> (h, w, 3) uint16 RGB codes 0..1023."""
    return np.clip(_unclamped(buf, w, h, pixfmt), 0, 1023).astype(np.uint16)


def clamped(buf, w, h, pixfmt):
    """(h, w) bool: pixels whose RGB left 0..1023 before the clamp (out of gamut: the round trip need not be the identity there)."""
    v = _unclamped(buf, w, h, pixfmt)
    return ((v < 0) | (v > 1023)).any(axis=-1)


def rgb10_to_yuv_planes(rgb10, pixfmt):
    """(h, w, 3) RGB codes -> (Y, Cb, Cr) int32 codes: Y per pixel; chroma from the SUM of the RGB codes of the block's pixels inside the frame - n = 2, or 1 in
    the last column of an odd width (4:2:2); n = 1 everywhere (4:4:4) - shifted by 16 + log2 n with the rounding constant scaled alike."""
    k = coefs(pixfmt)
    c = np.asarray(rgb10).astype(np.int32)
    h, w = c.shape[:2]
    sx = subx(pixfmt)
    cw, ch = chroma_dims(w, h, pixfmt)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = np.clip(((k["oyr"] * r + k["oyg"] * g + k["oyb"] * b + 0x8000) >> 16) + k["yoff"], 0, k["maxv"])
    s = np.zeros((h, sx * cw, 3), np.int32)
    s[:, :w] = c
    s = s.reshape(h, cw, sx, 3).sum(axis=2)
    n = np.zeros((h, sx * cw), np.int32)
    n[:, :w] = 1
    lg = np.log2(n.reshape(h, cw, sx).sum(axis=2)).astype(np.int32)      # 1 or 0
    rnd = np.int32(0x8000) << lg
    cb = np.clip(((k["our"] * s[..., 0] + k["oug"] * s[..., 1] + k["oub"] * s[..., 2] + rnd) >> (16 + lg)) + k["coff"], 0, k["maxv"])
    cr = np.clip(((k["ovr"] * s[..., 0] + k["ovg"] * s[..., 1] + k["ovb"] * s[..., 2] + rnd) >> (16 + lg)) + k["coff"], 0, k["maxv"])
    return y, cb, cr


def rgb10_to_yuv(rgb10, pixfmt):
    """(h, w, 3) RGB codes 0..1023 -> the flat YUV frame."""
    return pack(*rgb10_to_yuv_planes(rgb10, pixfmt), pixfmt)
