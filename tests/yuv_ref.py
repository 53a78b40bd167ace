"""The specification of the 4:2:0 Y'CbCr boundary (include/rife_hip.h RIFE_HIP_PIX_NV12 .. I420P10), once in numpy: what csrc/yuv.h restates in HIP.

A YUV call of the engine is, byte for byte,
    rgb10_to_yuv(process_px(yuv_to_rgb10(in0), yuv_to_rgb10(in1), t, A2B10G10R10))
with the integer conversions below (Q16 coefficients, + 0x8000, arithmetic shift), so kernel, this mirror and the tests agree bit for bit.
Frames are FLAT arrays (uint8 for NV12 / I420, uint16 for P010 / I420P10) of frame_elems(w, h) elements; cw = (w + 1) // 2, ch = (h + 1) // 2."""
import numpy as np

PIX_NV12, PIX_I420, PIX_P010, PIX_I420P10 = 16, 17, 18, 19
CSP_BT709, CSP_BT601, CSP_BT2020NCL = 0 << 8, 1 << 8, 2 << 8
CSP_FULL = 1 << 12
FORMATS = (PIX_NV12, PIX_I420, PIX_P010, PIX_I420P10)
MATRICES = (CSP_BT709, CSP_BT601, CSP_BT2020NCL)
KR_KB = {CSP_BT709: (0.2126, 0.0722), CSP_BT601: (0.299, 0.114), CSP_BT2020NCL: (0.2627, 0.0593)}


def base(pixfmt):
    return pixfmt & 0xff


def depth(pixfmt):
    return 10 if base(pixfmt) in (PIX_P010, PIX_I420P10) else 8


def planar(pixfmt):
    return base(pixfmt) in (PIX_I420, PIX_I420P10)


def dtype(pixfmt):
    return np.uint16 if depth(pixfmt) == 10 else np.uint8


def served(pixfmt):
    """The colour descriptions the engine serves: a known matrix, and full range at 8 bits only."""
    return base(pixfmt) in FORMATS and (pixfmt & 0xf00) in MATRICES and not (pixfmt & ~0x1fff) and not (depth(pixfmt) == 10 and pixfmt & CSP_FULL)


def chroma_dims(w, h):
    return (w + 1) // 2, (h + 1) // 2


def frame_elems(w, h):
    cw, ch = chroma_dims(w, h)
    return w * h + 2 * cw * ch


def frame_bytes(w, h, pixfmt):
    return frame_elems(w, h) * (2 if depth(pixfmt) == 10 else 1)


def plane_offsets(w, h, pixfmt):
    """Element offsets of the planes: (Y, CbCr) for the NV12 layout, (Y, Cb, Cr) for the I420 layout."""
    cw, ch = chroma_dims(w, h)
    return (0, w * h, w * h + cw * ch) if planar(pixfmt) else (0, w * h)


def real_ranges(pixfmt):
    """(luma offset, luma range, chroma offset, chroma range, largest code) in codes of the format's depth."""
    s = 4 if depth(pixfmt) == 10 else 1
    if pixfmt & CSP_FULL:
        return 0, 255 * s + (s - 1), 128 * s, 255 * s + (s - 1), 256 * s - 1      # 255 at depth 8 (1023 at depth 10: not served)
    return 16 * s, 219 * s, 128 * s, 224 * s, 256 * s - 1


def _q16(x):
    return int(np.floor(x * 65536.0 + 0.5))


def coefs(pixfmt):
    """The Q16 integer coefficients of both directions: the matrix's real coefficients times 1023 / range (in) and range / 1023 (out)."""
    kr, kb = KR_KB[pixfmt & 0xf00]
    kg = 1.0 - kr - kb
    yoff, yr, coff, cr, maxv = real_ranges(pixfmt)
    gi, gc = 1023.0 / yr, 1023.0 / cr
    go, gco = yr / 1023.0, cr / 1023.0
    return dict(
        yoff=yoff, coff=coff, maxv=maxv,
        iy=_q16(gi), irv=_q16(2 * (1 - kr) * gc), igu=_q16(-2 * kb * (1 - kb) / kg * gc), igv=_q16(-2 * kr * (1 - kr) / kg * gc), ibu=_q16(2 * (1 - kb) * gc),
        oyr=_q16(kr * go), oyg=_q16(kg * go), oyb=_q16(kb * go),
        our=_q16(-kr / (2 * (1 - kb)) * gco), oug=_q16(-kg / (2 * (1 - kb)) * gco), oub=_q16(0.5 * gco),
        ovr=_q16(0.5 * gco), ovg=_q16(-kg / (2 * (1 - kr)) * gco), ovb=_q16(-kb / (2 * (1 - kr)) * gco))


def split(buf, w, h, pixfmt):
    """Flat frame -> (Y (h, w), Cb (ch, cw), Cr (ch, cw)) int32 CODES: P010's high ten bits, an I420P10 sample above 1023 read as 1023."""
    cw, ch = chroma_dims(w, h)
    a = np.asarray(buf).reshape(-1)
    assert a.dtype == dtype(pixfmt) and a.size == frame_elems(w, h), "a %dx%d frame of this format has %d %s elements" % (w, h, frame_elems(w, h), dtype(pixfmt).__name__)
    a = a.astype(np.int32)
    y = a[:w * h].reshape(h, w)
    if planar(pixfmt):
        cb = a[w * h:w * h + cw * ch].reshape(ch, cw)
        cr = a[w * h + cw * ch:].reshape(ch, cw)
    else:
        uv = a[w * h:].reshape(ch, cw, 2)
        cb, cr = uv[..., 0], uv[..., 1]
    if base(pixfmt) == PIX_P010:
        y, cb, cr = y >> 6, cb >> 6, cr >> 6
    elif base(pixfmt) == PIX_I420P10:
        y, cb, cr = np.minimum(y, 1023), np.minimum(cb, 1023), np.minimum(cr, 1023)
    return y.copy(), cb.copy(), cr.copy()


def pack(y, cb, cr, pixfmt):
    """Codes -> the flat frame (P010: code << 6, zero low bits)."""
    y, cb, cr = (np.asarray(p, np.int32) for p in (y, cb, cr))
    if base(pixfmt) == PIX_P010:
        y, cb, cr = y << 6, cb << 6, cr << 6
    c = np.concatenate([cb.reshape(-1), cr.reshape(-1)]) if planar(pixfmt) else np.stack([cb, cr], axis=-1).reshape(-1)
    return np.concatenate([y.reshape(-1), c]).astype(dtype(pixfmt))


def canonical(buf, w, h, pixfmt):
    """What timestep 0 / 1 return: the frame's codes (P010 low bits cleared, I420P10 samples clamped to 1023)."""
    return pack(*split(buf, w, h, pixfmt), pixfmt)


def yuv_to_rgb10(buf, w, h, pixfmt):
    """Flat YUV frame -> (h, w, 3) uint16 RGB codes 0..1023; chroma of a pixel = the sample of its 2x2 block."""
    k = coefs(pixfmt)
    y, cb, cr = split(buf, w, h, pixfmt)
    cb = np.repeat(np.repeat(cb, 2, axis=0), 2, axis=1)[:h, :w] - k["coff"]
    cr = np.repeat(np.repeat(cr, 2, axis=0), 2, axis=1)[:h, :w] - k["coff"]
    yy = k["iy"] * (y - k["yoff"])
    r = (yy + k["irv"] * cr + 0x8000) >> 16
    g = (yy + k["igu"] * cb + k["igv"] * cr + 0x8000) >> 16
    b = (yy + k["ibu"] * cb + 0x8000) >> 16
    return np.clip(np.stack([r, g, b], axis=-1), 0, 1023).astype(np.uint16)


def clamped(buf, w, h, pixfmt):
    """(h, w) bool: pixels whose RGB left 0..1023 before the clamp (out of gamut: the round trip need not be the identity there)."""
    k = coefs(pixfmt)
    y, cb, cr = split(buf, w, h, pixfmt)
    cb = np.repeat(np.repeat(cb, 2, axis=0), 2, axis=1)[:h, :w] - k["coff"]
    cr = np.repeat(np.repeat(cr, 2, axis=0), 2, axis=1)[:h, :w] - k["coff"]
    yy = k["iy"] * (y - k["yoff"])
    v = np.stack([(yy + k["irv"] * cr + 0x8000) >> 16, (yy + k["igu"] * cb + k["igv"] * cr + 0x8000) >> 16, (yy + k["ibu"] * cb + 0x8000) >> 16], axis=-1)
    return ((v < 0) | (v > 1023)).any(axis=-1)


def rgb10_to_yuv_planes(rgb10, pixfmt):
    """(h, w, 3) RGB codes -> (Y, Cb, Cr) int32 codes: Y per pixel, chroma from the SUM of the RGB codes of the block's pixels inside the frame (n = 4, 2, 1)."""
    k = coefs(pixfmt)
    c = np.asarray(rgb10).astype(np.int32)
    h, w = c.shape[:2]
    cw, ch = chroma_dims(w, h)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = np.clip(((k["oyr"] * r + k["oyg"] * g + k["oyb"] * b + 0x8000) >> 16) + k["yoff"], 0, k["maxv"])
    s = np.zeros((2 * ch, 2 * cw, 3), np.int32)
    s[:h, :w] = c
    s = s.reshape(ch, 2, cw, 2, 3).sum(axis=(1, 3))
    n = np.zeros((2 * ch, 2 * cw), np.int32)
    n[:h, :w] = 1
    lg = np.log2(n.reshape(ch, 2, cw, 2).sum(axis=(1, 3))).astype(np.int32)      # 2, 1 or 0
    rnd = np.int32(0x8000) << lg
    cb = np.clip(((k["our"] * s[..., 0] + k["oug"] * s[..., 1] + k["oub"] * s[..., 2] + rnd) >> (16 + lg)) + k["coff"], 0, k["maxv"])
    cr = np.clip(((k["ovr"] * s[..., 0] + k["ovg"] * s[..., 1] + k["ovb"] * s[..., 2] + rnd) >> (16 + lg)) + k["coff"], 0, k["maxv"])
    return y, cb, cr


def rgb10_to_yuv(rgb10, pixfmt):
    """(h, w, 3) RGB codes 0..1023 -> the flat YUV frame."""
    return pack(*rgb10_to_yuv_planes(rgb10, pixfmt), pixfmt)


# ---- the exact real-valued formulas (float64), for the accuracy test of the integer forward conversion ----
def yuv_to_rgb10_real(y, cb, cr, pixfmt):
    """Codes (any broadcastable arrays) -> unclamped real RGB in 10-bit code units."""
    kr, kb = KR_KB[pixfmt & 0xf00]
    kg = 1.0 - kr - kb
    yoff, yr, coff, crng, _ = real_ranges(pixfmt)
    yn = (np.asarray(y, np.float64) - yoff) / yr
    u = (np.asarray(cb, np.float64) - coff) / crng
    v = (np.asarray(cr, np.float64) - coff) / crng
    r = yn + 2 * (1 - kr) * v
    b = yn + 2 * (1 - kb) * u
    g = (yn - kr * r - kb * b) / kg
    return np.stack([r, g, b], axis=-1) * 1023.0
