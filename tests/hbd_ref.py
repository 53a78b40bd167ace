"""High bit depth (include/rife_hip.h "high bit depth") in numpy: the definition of an hbd call, stated with nothing of the code under test.
  reduce10        the proxy sample of a stored sample;
  plane_shapes    the three planes of a layout;
  proxy_frame     the tight ten-bit frame of the image's pixfmt that holds the reduced planes (what the _px calls and the sets calls take);
  make_sets       the sets of the definition over host planes (amd.apply_set: u16, maxval (1 << depth) - 1, extent 0, 0);
  expected        the composition itself through the EXISTING rife_hip_process_apply_sets;
  planes          seeded test planes of a layout: smooth motion between the two frames, full use of the depth, a sprinkle of samples above maxval."""
import ctypes
import importlib

import numpy as np

amd = importlib.import_module("rife-ncnn-vulkan_amd")

BASES = (amd.PIX_I420P10, amd.PIX_I422P10, amd.PIX_I444P10, amd.PIX_RGBP10)
NAME = {amd.PIX_I420P10: "i420", amd.PIX_I422P10: "i422", amd.PIX_I444P10: "i444", amd.PIX_RGBP10: "rgbp"}
SHIFT = {amd.PIX_I420P10: (-1, -1), amd.PIX_I422P10: (-1, 0)}      # the chroma set of a subsampled layout
SENTINEL = 0xabcd                                                  # what planes() puts around a plane


_GEOM = {}                                                         # address of a plane of planes() / blank_like() -> (the (rows, pitch) array behind it, its offset)


def _view(rows, cols, pitch, offset):
    raw = np.full(rows * pitch + 32, SENTINEL, np.uint16)
    lead = (-raw.ctypes.data % 64) // 2                               # the array behind the view starts on 64 bytes, whatever the allocator gave
    big = raw[lead:lead + rows * pitch].reshape(rows, pitch)
    v = big[:, offset:offset + cols]
    _GEOM[v.ctypes.data] = (big, offset)                              # keeps `big` alive: no address comes back
    return v


def blank_like(ps):
    """output planes with the geometry (pitch, offset) of the planes `ps` of planes(): the sentinel everywhere"""
    return [_view(p.shape[0], p.shape[1], _GEOM[p.ctypes.data][0].shape[1], _GEOM[p.ctypes.data][1]) for p in ps]


def untouched(view):
    """every sample of the array behind an output plane, outside the plane, still holds the sentinel"""
    big, off = _GEOM[view.ctypes.data]
    rest = big.copy()
    rest[:, off:off + view.shape[1]] = SENTINEL
    return bool((rest == SENTINEL).all())


def reduce10(v, depth):
    """c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023); depth 10: min(v, 1023).  v: any unsigned integer array (or scalar) of stored samples."""
    v = np.asarray(v).astype(np.uint32)
    if not 10 <= depth <= 16:
        raise ValueError("depth is 10..16")
    c = (v + np.uint32(1 << (depth - 11))) >> np.uint32(depth - 10) if depth > 10 else v
    return np.minimum(c, 1023).astype(np.uint16)


def plane_shapes(w, h, pixfmt):
    b = pixfmt & 0xff
    if b not in BASES:
        raise ValueError("not a high-bit-depth layout")
    cw = w if b in (amd.PIX_I444P10, amd.PIX_RGBP10) else (w + 1) // 2
    ch = (h + 1) // 2 if b == amd.PIX_I420P10 else h
    return [(h, w), (ch, cw), (ch, cw)]


def proxy_frame(planes, depth):
    """the tight frame: the reduced planes glued one after the other"""
    return np.concatenate([reduce10(p, depth).ravel() for p in planes])


def make_sets(planes0, planes1, depth, pixfmt, out):
    """the sets of the definition; `out`: three writable plane arrays, filled in place"""
    maxval = (1 << depth) - 1
    if (pixfmt & 0xff) in SHIFT:
        return [amd.apply_set(planes0[:1], planes1[:1], (0, 0), maxval, None, out[:1]), amd.apply_set(planes0[1:], planes1[1:], SHIFT[pixfmt & 0xff], maxval, None, out[1:])]
    return [amd.apply_set(tuple(planes0), tuple(planes1), (0, 0), maxval, None, tuple(out))]


def expected(engine, planes0, planes1, timestep, depth, pixfmt):
    """rife_hip_process_apply_sets(r, proxy0, proxy1, w, h, timestep, NULL, pixfmt, nsets, sets) on the host: the planes an hbd call must write, as new tight arrays"""
    h, w = planes0[0].shape
    f0, f1 = proxy_frame(planes0, depth), proxy_frame(planes1, depth)
    out = tuple(np.zeros(p.shape, np.uint16) for p in planes0)
    n, arr = amd._set_array(make_sets(planes0, planes1, depth, pixfmt, out))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = engine._L.rife_hip_process_apply_sets(engine._h, p(f0), p(f1), w, h, float(timestep), None, int(pixfmt), n, arr)
    if rc:
        raise amd.RifeError("reference process_apply_sets failed (%d): %s" % (rc, engine._L.rife_hip_last_error().decode()))
    return out


def planes(w, h, pixfmt, depth, seed, pitch_pad=0, offset=0, over=True):
    """Two frames of a layout as lists of three uint16 planes: a smooth pattern that moves by a few pixels between the frames plus noise in the low bits, scaled to the
    depth; over: about 1 sample in 64 lies above maxval (the blend reads it as stored, the proxy clamps it).  pitch_pad, offset: each plane is a view into a larger
    array, rows pitch_pad samples longer than the plane and the first sample `offset` samples in (alignment cases)."""
    rng = np.random.default_rng(seed)
    maxval = (1 << depth) - 1
    frames = []
    for f in range(2):
        ps = []
        for k, (ph, pw) in enumerate(plane_shapes(w, h, pixfmt)):
            y, x = np.mgrid[0:ph, 0:pw].astype(np.float64)
            sx, sy = w / pw, h / ph
            v = 0.5 + 0.25 * np.sin((x * sx + 3.0 * f + 5 * k) / 9.0) + 0.2 * np.cos((y * sy - 2.0 * f + 3 * k) / 7.0)
            a = np.clip(v * maxval + rng.integers(-(1 << (depth - 8)), 1 << (depth - 8), (ph, pw)), 0, maxval).astype(np.uint16)
            if over and depth < 16:
                hit = rng.random((ph, pw)) < 1.0 / 64
                a[hit] = rng.integers(maxval + 1, 65536, int(hit.sum()), dtype=np.uint32).astype(np.uint16)
            v = _view(ph, pw, pw + pitch_pad + offset, offset)
            v[...] = a
            ps.append(v)
        frames.append(ps)
    return frames
