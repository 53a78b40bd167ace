"""16-bit packed RGB and RGBA (include/rife_hip.h "16-bit packed RGB and RGBA") in numpy: the definition of a packed call, stated with nothing of the code under test.
  deinterleave / interleave   a packed (h, w, ch) frame <-> its ch contiguous (h, w) planes;
  view / blank_like           pitched and misaligned packed arrays inside sentinel-filled parents; untouched / big speak about the parent;
  frames                      two seeded packed test frames: smooth motion between them, full use of the depth, a sprinkle of samples above maxval;
  random_frames               two frames of full-range random samples;
  expected                    the composition itself: reduce10 (hbd_ref) of the colour planes as a tight RGBP10 proxy, then the EXISTING rife_hip_process_apply_sets with
                              ONE set of ch planes at shift (0, 0), maxval (1 << depth) - 1, extent 0, 0; re-interleaved."""
import ctypes
import importlib

import numpy as np

import hbd_ref as hr
from hbd_ref import reduce10  # noqa: F401   (the proxy sample: one statement for both sections)

amd = importlib.import_module("rife-ncnn-vulkan_amd")

SENTINEL = hr.SENTINEL


def deinterleave(a):
    """the ch planes of a packed (h, w, ch) frame, each a new contiguous (h, w) array"""
    return [np.ascontiguousarray(a[:, :, k]) for k in range(a.shape[2])]


def interleave(planes):
    """a new tight (h, w, ch) frame from ch (h, w) planes"""
    return np.ascontiguousarray(np.stack(planes, axis=2))


def view(w, h, ch, pitch, offset=0):
    """an (h, w, ch) uint16 window `offset` samples into a 64-byte-aligned sentinel-filled array of h rows of `pitch` samples"""
    assert pitch >= w * ch + offset
    return hr._view(h, w * ch, pitch, offset).reshape(h, w, ch)


def tight_pitch(w, ch, multiple=1, pad=0, offset=0):
    """the smallest pitch in samples that holds a row, `pad` samples and the offset, rounded up to `multiple` samples"""
    return (w * ch + pad + offset + multiple - 1) // multiple * multiple


def big(a):
    """the whole (rows, pitch) array behind a frame of view() / blank_like()"""
    return hr._GEOM[a.ctypes.data][0]


def blank_like(a):
    """an output frame with the geometry (pitch, offset) of the frame `a` of view(): the sentinel everywhere"""
    parent, off = hr._GEOM[a.ctypes.data]
    return view(a.shape[1], a.shape[0], a.shape[2], parent.shape[1], off)


def untouched(a):
    """every sample of the array behind an output frame, outside the frame, still holds the sentinel"""
    parent, off = hr._GEOM[a.ctypes.data]
    rest = parent.copy()
    rest[:, off:off + a.shape[1] * a.shape[2]] = SENTINEL
    return bool((rest == SENTINEL).all())


def frames(w, h, ch, depth, seed, pitch=None, offset=0, over=True, opaque=False):
    """Two packed frames: the colour planes of hbd_ref.planes (RGBP10 layout) plus, for ch = 4, a moving soft-edged matte (opaque: maxval everywhere)."""
    p0, p1 = hr.planes(w, h, amd.PIX_RGBP10, depth, seed, over=over)
    maxval = (1 << depth) - 1
    out = []
    for f, ps in enumerate((p0, p1)):
        ps = [np.ascontiguousarray(p) for p in ps]
        if ch == 4:
            y, x = np.mgrid[0:h, 0:w].astype(np.float64)
            al = np.clip(0.5 + 0.6 * np.sin((x + 2.0 * f) / 5.0) * np.cos((y - 1.0 * f) / 6.0), 0.0, 1.0)
            ps.append(np.full((h, w), maxval, np.uint16) if opaque else (al * maxval + 0.5).astype(np.uint16))
        v = view(w, h, ch, pitch if pitch is not None else w * ch + offset, offset)
        v[...] = interleave(ps)
        out.append(v)
    return out


def random_frames(w, h, ch, rng, pitch, offset=0):
    """two frames of random u16 over the whole range (samples above maxval are read as stored)"""
    out = []
    for _ in range(2):
        v = view(w, h, ch, pitch, offset)
        v[...] = rng.integers(0, 65536, (h, w, ch), dtype=np.uint32).astype(np.uint16)
        out.append(v)
    return out


def proxy_frame(a, depth):
    """the tight RGBP10 frame: the reduced colour planes glued one after the other"""
    return np.concatenate([reduce10(a[:, :, k], depth).ravel() for k in range(3)])


def expected(engine, in0, in1, timestep, depth):
    """rife_hip_process_apply_sets(r, proxy0, proxy1, w, h, timestep, NULL, RIFE_HIP_PIX_RGBP10, 1, set) on the host with the set of ch planes: the frame a packed
    call must write, as a new tight array"""
    h, w, ch = in0.shape
    f0, f1 = proxy_frame(in0, depth), proxy_frame(in1, depth)
    out = tuple(np.zeros((h, w), np.uint16) for _ in range(ch))
    n, arr = amd._set_array([amd.apply_set(tuple(deinterleave(in0)), tuple(deinterleave(in1)), (0, 0), (1 << depth) - 1, None, out)])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = engine._L.rife_hip_process_apply_sets(engine._h, p(f0), p(f1), w, h, float(timestep), None, int(amd.PIX_RGBP10), n, arr)
    if rc:
        raise amd.RifeError("reference process_apply_sets failed (%d): %s" % (rc, engine._L.rife_hip_last_error().decode()))
    return interleave(out)
