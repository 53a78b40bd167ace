"""Semi-planar high bit depth (include/rife_hip.h "semi-planar high bit depth") in numpy: the definition of a semi-planar call, stated with nothing of the code under test.
A surface is a pair (y, cbcr) of uint16 arrays: (h, w) luma and (ch, 2 * cw) interleaved Cb, Cr pairs, cw = (w + 1) // 2, ch = (h + 1) // 2 (chroma 1) or h (chroma 2),
codes of `depth` bits in the HIGH bits; s = 16 - depth.
  split / join                a surface -> the three planes Y >> s, Cb >> s, Cr >> s of the planar hbd layout; three planes of codes -> the tight surface, codes << s;
  pixfmt                      the planar layout of the definition: PIX_I420P10 | csp (chroma 1) or PIX_I422P10 | csp (chroma 2);
  chroma_shape                (ch, 2 * cw);
  surface / blank_like        pitched and misaligned surfaces inside sentinel-filled parents (hbd_ref._view); untouched / big speak about the parents;
  surfaces                    two seeded test surfaces: the planes of hbd_ref.planes as codes in the high bits, random garbage in the low bits;
  random_surfaces             two surfaces of full-range random samples;
  expected                    the composition itself: the EXISTING process_hbd on split(in0), split(in1), joined back."""
import importlib

import numpy as np

import hbd_ref as hr

amd = importlib.import_module("rife-ncnn-vulkan_amd")

SENTINEL = hr.SENTINEL


def pixfmt(chroma, csp=0):
    return {1: amd.PIX_I420P10, 2: amd.PIX_I422P10}[chroma] | csp


def chroma_shape(w, h, chroma):
    return ((h + 1) // 2 if chroma == 1 else h, 2 * ((w + 1) // 2))


def split(surface, depth):
    """the planes Y >> s, Cb >> s, Cr >> s, each a new contiguous array"""
    y, c = surface
    s = 16 - depth
    return [np.ascontiguousarray(y >> s), np.ascontiguousarray(c[:, 0::2] >> s), np.ascontiguousarray(c[:, 1::2] >> s)]


def join(planes, depth):
    """a new tight surface from three planes of codes: Y << s, and Cb << s, Cr << s interleaved"""
    s = 16 - depth
    yy, cb, cr = (np.asarray(p).astype(np.uint16) for p in planes)
    c = np.empty((cb.shape[0], 2 * cb.shape[1]), np.uint16)
    c[:, 0::2] = cb << s
    c[:, 1::2] = cr << s
    return np.ascontiguousarray(yy << s), c


def surface(w, h, chroma, pad=0, offset=0, multiple=1, odd=False):
    """a sentinel-filled surface: each plane `offset` samples into a 64-byte-aligned array whose rows are `pad` samples longer than the plane and the offset, the pitch
    rounded up to `multiple` samples (odd: made odd)"""
    out = []
    for rows, cols in ((h, w), chroma_shape(w, h, chroma)):
        pitch = (cols + pad + offset + multiple - 1) // multiple * multiple
        out.append(hr._view(rows, cols, pitch | 1 if odd else pitch, offset))
    return tuple(out)


def big(a):
    """the whole (rows, pitch) array behind a plane of surface() / blank_like()"""
    return hr._GEOM[a.ctypes.data][0]


def blank_like(sf):
    """an output surface with the geometry (pitch, offset) of the surface `sf` of surface(): the sentinel everywhere"""
    return tuple(hr.blank_like(list(sf)))


def untouched(sf):
    return all(hr.untouched(p) for p in sf)


def fill(sf, planes, depth, rng=None):
    """write join(planes) into the surface; rng: random garbage in the low 16 - depth bits of every sample"""
    s = 16 - depth
    for dst, src in zip(sf, join(planes, depth)):
        dst[...] = src | (rng.integers(0, 1 << s, src.shape, dtype=np.uint32).astype(np.uint16) if rng is not None and s else np.uint16(0))
    return sf


def surfaces(w, h, chroma, depth, seed, pad=0, offset=0, multiple=1, odd=False, low_bits=True):
    """Two surfaces: the smooth moving pattern of hbd_ref.planes (codes up to maxval) in the high bits, random low bits under the code"""
    rng = np.random.default_rng(seed + 77)
    return [fill(surface(w, h, chroma, pad, offset, multiple, odd), ps, depth, rng if low_bits else None)
            for ps in hr.planes(w, h, pixfmt(chroma), depth, seed, over=False)]


def random_surfaces(w, h, chroma, rng, pad=0, offset=0, multiple=1, odd=False):
    """two surfaces of random u16 over the whole range: every code, every low-bit pattern"""
    out = []
    for _ in range(2):
        sf = surface(w, h, chroma, pad, offset, multiple, odd)
        for p in sf:
            p[...] = rng.integers(0, 65536, p.shape, dtype=np.uint32).astype(np.uint16)
        out.append(sf)
    return out


def expected(engine, in0, in1, timestep, depth, chroma, csp=0):
    """join(planes << s) of what the existing process_hbd writes for split(in0), split(in1): the surface a semi-planar call must write, as new tight arrays"""
    planes = engine.process_hbd(tuple(split(in0, depth)), tuple(split(in1, depth)), timestep, depth, pixfmt(chroma, csp))
    return join(planes, depth)
