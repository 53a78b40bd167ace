"""Planar RGB (RIFE_HIP_PIX_RGBP8 / RGBP10 / RGBPH / RGBPF, include/rife_hip.h "planar RGB") in numpy: the conversions to and from 10-bit codes that the header
fixes to the bit, and the frame layout.  Every float step is one float32 operation on float32 arrays, so nothing is fused and nothing runs in double.

A frame is a (3, h, w) array R, G, B of the format's dtype; a tight frame is that array C-contiguous."""
import numpy as np

PIX_RGBP8, PIX_RGBP10, PIX_RGBPH, PIX_RGBPF = 65, 67, 69, 71
FORMATS = (PIX_RGBP8, PIX_RGBP10, PIX_RGBPH, PIX_RGBPF)
NAMES = {PIX_RGBP8: "rgbp8", PIX_RGBP10: "rgbp10", PIX_RGBPH: "rgbph", PIX_RGBPF: "rgbpf"}
_DTYPE = {PIX_RGBP8: np.uint8, PIX_RGBP10: np.uint16, PIX_RGBPH: np.float16, PIX_RGBPF: np.float32}
F32 = np.float32


def dtype(px):
    return _DTYPE[px]


def elem(px):
    return np.dtype(_DTYPE[px]).itemsize


def frame_bytes(w, h, px):
    return 3 * w * h * elem(px)


def float_code(x):
    """float32 samples -> codes: c = (int)(fminf(fmaxf(x, 0.f), 1.f) * 1023.f + 0.5f), the product and the sum each rounded to float32.  NaN reads as 0."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        x = np.where(x > F32(0), x, F32(0)).astype(F32)      # NaN and negatives (and -0): 0
        x = np.where(x < F32(1), x, F32(1)).astype(F32)      # +inf and everything above 1: 1
    p = (x * F32(1023)).astype(F32)
    s = (p + F32(0.5)).astype(F32)
    return s.astype(np.int32)                                 # truncation; s is in [0.5, 1023.5]


def to10(v, px):
    """Samples of format px (any shape) -> int32 codes 0..1023."""
    v = np.asarray(v)
    assert v.dtype == _DTYPE[px], (v.dtype, px)
    if px == PIX_RGBP8:
        v = v.astype(np.int32)
        return (v << 2) | (v >> 6)
    if px == PIX_RGBP10:
        return np.minimum(v.astype(np.int32), 1023)
    return float_code(v.astype(F32))                           # half widens exactly


def code_float(c):
    """codes -> float32 samples: (float)c / 1023.f, one correctly rounded float32 division."""
    return (np.asarray(c).astype(F32) / F32(1023)).astype(F32)


def from10(c, px):
    """int codes 0..1023 -> samples of format px."""
    c = np.asarray(c).astype(np.int32)
    if px == PIX_RGBP8:
        return (c >> 2).astype(np.uint8)
    if px == PIX_RGBP10:
        return c.astype(np.uint16)
    f = code_float(c)
    return f.astype(np.float16) if px == PIX_RGBPH else f      # float32 -> float16 rounds to nearest even


def canonical(v, px):
    """What timestep 0 / 1 return for a frame: from10(to10(v))."""
    return from10(to10(v, px), px)


def to_rgb10(frame, px):
    """(3, h, w) frame -> (h, w, 3) uint16 codes, the layout of the engine's RGB10 frames (pack with pack_a2b10g10r10)."""
    frame = np.asarray(frame)
    assert frame.ndim == 3 and frame.shape[0] == 3
    return to10(frame, px).transpose(1, 2, 0).astype(np.uint16)


def from_rgb10(codes, px):
    """(h, w, 3) codes -> (3, h, w) frame of format px, C-contiguous (= the tight frame)."""
    return np.ascontiguousarray(from10(np.asarray(codes).transpose(2, 0, 1), px))


def pack(r, g, b, px):
    """Three (h, w) planes -> the tight frame, (3, h, w)."""
    return np.ascontiguousarray(np.stack([np.asarray(p, _DTYPE[px]) for p in (r, g, b)]))


def split(frame):
    return frame[0], frame[1], frame[2]


def boundary_floats():
    """For every k in 0..1022 the three float32 values nearest (k + 0.5) / 1023: where x * 1023 + 0.5 is nearest an integer, so where a fused multiply-add
    (one rounding) and the two-step form (two roundings) give different codes.  Shape (1023, 3)."""
    k = np.arange(1023, dtype=np.float64)
    mid = ((k + 0.5) / 1023.0).astype(F32)
    return np.stack([np.nextafter(mid, F32(0)), mid, np.nextafter(mid, F32(2))], axis=1)
