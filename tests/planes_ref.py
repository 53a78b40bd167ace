"""Strided frames and separate planes (include/rife_hip.h rife_hip_image_t) in numpy: a tight frame of the _px calls scattered into strided planes whose every
byte outside the windows holds a canary, and gathered back.  Built on tests/yuv_ref.py's plane arithmetic; no library call, no GPU.

    im = to_image(tight, w, h, pixfmt, pitches)      # pitches: one of LAYOUTS, or a list of pitches in bytes (one buffer per plane, no misalignment)
    im.desc                                          # the ctypes descriptor (amd.rife_hip_image) over im.bufs
    from_image(im)                                   # the tight frame again (bytes)
    im.canaries_intact()                             # every byte outside the windows still holds the canary

LAYOUTS (the pitch cases of the tests):
    tight     planes glued one after the other, pitch = row bytes: the frame of the _px calls
    elem      pitch = row bytes + one element, plane bases one element past a 64-byte boundary: breaks every alignment of the wide kernels
    a64       rows and plane bases aligned to 64 bytes (VapourSynth / AviSynth)
    window    a window at offset (5, 3) inside a plane at least twice as large (a crop or a tile with its parent's pitch)
    separate  every plane in an allocation of its own, and for the three-plane formats in the order Y, Cr, Cb (YV12): the descriptor's plane[1] / plane[2]
              are swapped by the caller, so the frame the call sees is the tight frame with its chroma planes exchanged (swap_chroma)
"""
import ctypes
import importlib

import numpy as np

import yuv_ref as yr

amd = importlib.import_module("rife-ncnn-vulkan_amd")

RGB_BPP = {amd.PIX_RGB8: 3, amd.PIX_RGB10_U16: 6, amd.PIX_A2B10G10R10: 4, amd.PIX_RGBA8: 4}
ELEM = {amd.PIX_RGB8: 1, amd.PIX_RGB10_U16: 2, amd.PIX_A2B10G10R10: 4, amd.PIX_RGBA8: 1, amd.PIX_NV12: 1, amd.PIX_I420: 1, amd.PIX_P010: 2, amd.PIX_I420P10: 2}
ALL_FORMATS = (amd.PIX_RGB8, amd.PIX_RGB10_U16, amd.PIX_A2B10G10R10, amd.PIX_RGBA8, amd.PIX_NV12, amd.PIX_I420, amd.PIX_P010, amd.PIX_I420P10)
FMT_NAME = {amd.PIX_RGB8: "rgb8", amd.PIX_RGB10_U16: "rgb10u16", amd.PIX_A2B10G10R10: "a2b10g10r10", amd.PIX_RGBA8: "rgba8", amd.PIX_NV12: "nv12", amd.PIX_I420: "i420",
            amd.PIX_P010: "p010", amd.PIX_I420P10: "i420p10"}
LAYOUTS = ("tight", "elem", "a64", "window", "separate")
MARGIN = 64      # canary bytes before and after every plane


def is_yuv(pixfmt):
    return (pixfmt & 0xff) >= amd.PIX_NV12


def elem_size(pixfmt):
    return ELEM[pixfmt & 0xff]


def plane_table(w, h, pixfmt):
    """[(rows, row_bytes, byte offset in the tight frame, bytes per x step of the plane)] per plane: pix_bpp for the RGB formats, tests/yuv_ref.py for 4:2:0."""
    b = pixfmt & 0xff
    if not is_yuv(pixfmt):
        return [(h, w * RGB_BPP[b], 0, RGB_BPP[b])]
    es = elem_size(pixfmt)
    cw, ch = yr.chroma_dims(w, h)
    offs = [o * es for o in yr.plane_offsets(w, h, pixfmt)]
    if yr.planar(pixfmt):
        return [(h, w * es, offs[0], es), (ch, cw * es, offs[1], es), (ch, cw * es, offs[2], es)]
    return [(h, w * es, offs[0], es), (ch, 2 * cw * es, offs[1], 2 * es)]


def row_bytes(w, pixfmt, plane):
    t = plane_table(w, 2, pixfmt)
    return t[plane][1] if 0 <= plane < len(t) else 0


def frame_bytes(w, h, pixfmt):
    t = plane_table(w, h, pixfmt)
    return t[-1][2] + t[-1][0] * t[-1][1]


def swap_chroma(tight, w, h, pixfmt):
    """The tight frame with its Cb and Cr planes exchanged (three-plane formats; any other format: unchanged)."""
    b = np.frombuffer(np.ascontiguousarray(tight).tobytes(), np.uint8).copy()
    t = plane_table(w, h, pixfmt)
    if len(t) == 3:
        n = t[1][0] * t[1][1]
        b[t[1][2]:t[1][2] + n], b[t[2][2]:t[2][2] + n] = b[t[2][2]:t[2][2] + n].copy(), b[t[1][2]:t[1][2] + n].copy()
    return b


def _aligned(nbytes, misalign, canary):
    """A uint8 array of nbytes whose address is `misalign` past a 64-byte boundary, filled with the canary."""
    raw = np.full(nbytes + 128, canary, np.uint8)
    start = (-raw.ctypes.data) % 64 + misalign
    return raw[start:start + nbytes]


class StridedImage:
    def __init__(self, w, h, pixfmt, canary):
        self.w, self.h, self.pixfmt, self.canary = w, h, pixfmt, canary
        self.bufs = []        # uint8 arrays (canaries + windows)
        self.planes = []      # per plane of the DESCRIPTOR: (buffer index, byte offset of the window's first byte, pitch, rows, row_bytes, tight offset)
        self.desc = None

    def _finish(self):
        self.desc = amd.device_image(self.w, self.h, self.pixfmt, [(self.bufs[bi].ctypes.data + off, pitch) for (bi, off, pitch, _, _, _) in self.planes])
        self.desc._keep = self      # to_image(...).desc alone keeps the buffers alive
        return self

    def window_mask(self, bi):
        m = np.zeros(self.bufs[bi].size, bool)
        for (b, off, pitch, rows, rb, _) in self.planes:
            if b == bi:
                for y in range(rows):
                    m[off + y * pitch: off + y * pitch + rb] = True
        return m

    def canaries_intact(self):
        return all(bool((self.bufs[bi][~self.window_mask(bi)] == self.canary).all()) for bi in range(len(self.bufs)))

    def rebased(self, addresses):
        """The descriptor over copies of the buffers at other base addresses (device memory): one address per buffer."""
        return amd.device_image(self.w, self.h, self.pixfmt, [(addresses[bi] + off, pitch) for (bi, off, pitch, _, _, _) in self.planes])


def to_image(tight, w, h, pixfmt, pitches="tight", canary=0xC5):
    """Scatter the tight frame (any array of frame_bytes(w, h, pixfmt) bytes) into strided planes; every byte outside the windows = canary."""
    src = np.frombuffer(np.ascontiguousarray(tight).tobytes(), np.uint8)
    table = plane_table(w, h, pixfmt)
    assert src.size == frame_bytes(w, h, pixfmt), (src.size, frame_bytes(w, h, pixfmt))
    es = elem_size(pixfmt)
    im = StridedImage(w, h, pixfmt, canary)
    order = list(range(len(table)))
    if pitches == "tight":
        im.bufs.append(_aligned(src.size, 0, canary))
        im.planes = [(0, toff, rb, rows, rb, toff) for (rows, rb, toff, _) in table]
    elif pitches == "separate":
        if len(table) == 3:
            order = [0, 2, 1]                                   # Y, Cr, Cb: what the caller of a YV12 producer passes as plane[1], plane[2]
        for k, p in enumerate(order):
            rows, rb, toff, _ = table[p]
            pitch = (rb + 63) // 64 * 64 if k == 0 else rb + es
            im.bufs.append(_aligned(2 * MARGIN + rows * pitch, 0, canary))
            im.planes.append((k, MARGIN, pitch, rows, rb, toff))
    else:
        at = 0
        spans = []
        for (rows, rb, toff, step) in table:
            if isinstance(pitches, (list, tuple)):
                pitch, lead = int(pitches[len(spans)]), 0
            elif pitches == "elem":
                pitch, lead = rb + es, es                         # one element past a 64-byte boundary
            elif pitches == "a64":
                pitch, lead = (rb + 63) // 64 * 64, 0
            elif pitches == "window":                           # parent plane: (2 * units + 6) x steps wide, 2 * rows + 4 high; the window starts at (5, 3)
                pitch = (2 * (rb // step) + 6) * step
                lead = 3 * pitch + 5 * step
            else:
                raise ValueError(pitches)
            total = (2 * rows + 4) * pitch if pitches == "window" else rows * pitch
            at = (at + 63) // 64 * 64 + MARGIN
            spans.append((at + lead, pitch, rows, rb, toff))
            at += total + MARGIN
        im.bufs.append(_aligned(at, 0, canary))
        im.planes = [(0, off, pitch, rows, rb, toff) for (off, pitch, rows, rb, toff) in spans]
    for (bi, off, pitch, rows, rb, toff) in im.planes:
        for y in range(rows):
            im.bufs[bi][off + y * pitch: off + y * pitch + rb] = src[toff + y * rb: toff + (y + 1) * rb]
    return im._finish()


def from_image(im):
    """Gather the windows of a StridedImage back into the tight frame (uint8 bytes), by the tight offsets its planes were scattered from."""
    out = np.zeros(frame_bytes(im.w, im.h, im.pixfmt), np.uint8)
    for (bi, off, pitch, rows, rb, toff) in im.planes:
        for y in range(rows):
            out[toff + y * rb: toff + (y + 1) * rb] = im.bufs[bi][off + y * pitch: off + y * pitch + rb]
    return out


def seen_by_call(tight, w, h, pixfmt, pitches):
    """The tight frame the CALL sees for an image made by to_image: the frame itself, except for `separate` on a three-plane format, whose descriptor lists
    Cr before Cb - the call reads (and writes) plane[1] as Cb, so it is the frame with the chroma planes exchanged."""
    return swap_chroma(tight, w, h, pixfmt) if pitches == "separate" else np.frombuffer(np.ascontiguousarray(tight).tobytes(), np.uint8)
