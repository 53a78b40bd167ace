"""Every entry point, one after the other, on ONE workspace: the device calls find their stream's workspace through one shared lookup, the host calls lease theirs from one
pool, and a workspace that has served one frame layout must serve the next as a new one would.

  A  device calls on one engine, first on the NULL stream (the engine's own stream and its workspace), then on one caller-created stream (a second workspace):
     process_device_px (RGB8), process_device_image (8-bit I420, padded rows), process_device_apply_sets (one u16 set), process_device_hbd (I420P10 layout, depth 12),
     process_device_hbd_packed (3 channels, depth 16), process_device_hbd_semiplanar (4:2:0, depth 10), process_device_px (RGB8) again.  Every output, row padding and all,
     is byte for byte what the same call writes as the first call of a freshly created engine.
  B  the host twins of the six calls on one engine of the test build, against the same kind of reference; afterwards the pool holds no lease.

100 x 60 pads to 128 x 64: the smallest frame with edge tiles in both axes.  Byte equality: the kernels are deterministic by the build's flags."""
import importlib

import numpy as np
import pytest

from tools import gen_frames

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")

W, H, T = 100, 60, 0.5
CW, CH = W // 2, H // 2
FILL = 0x5a
_IN = {}


def _blank(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def _padded(a, cols):
    """`a` in the first columns of a contiguous array of `cols` elements per row, FILL bytes after them"""
    full = _blank((a.shape[0], cols), a.dtype)
    full[:, :a.shape[1]] = a
    return full


def _inputs():
    """per frame of a moving pair: the RGB8 frame, I420 planes in padded rows, two 12-bit planes, I420 planes of 12-bit codes, a 16-bit packed frame, a 10-bit 4:2:0 surface"""
    if not _IN:
        for i, f in enumerate(gen_frames.smooth_pair(W, H, 5)):
            y, u, v = f[..., 1], f[::2, ::2, 0], f[::2, ::2, 2]
            cbcr = np.empty((CH, 2 * CW), np.uint16)
            cbcr[:, 0::2] = u.astype(np.uint16) << 8; cbcr[:, 1::2] = v.astype(np.uint16) << 8
            _IN[i] = dict(rgb=np.ascontiguousarray(f),
                          i420=(_padded(y, 128), _padded(u, 64), _padded(v, 64)),
                          set=np.ascontiguousarray(np.stack([f[..., 0], f[..., 2]]).astype(np.uint16) * 16),
                          hbd=tuple(np.ascontiguousarray(p.astype(np.uint16) * 16) for p in (y, u, v)),
                          packed=np.ascontiguousarray(f.astype(np.uint16) * 257),
                          sp=(np.ascontiguousarray(y.astype(np.uint16) << 8), cbcr))
    return _IN[0], _IN[1]


def _fresh(modeldirs, test_build=False):
    g = (pkg.test_build() if test_build else pkg).RIFE(0, rife_v4=True)
    g.load(modeldirs["rife-v4.6"])
    return g


# ---- the device calls: arrays go up whole (padding included), descriptors name them by address and pitch, everything comes back ----
class _Dev:
    def __init__(self, a):
        import torch
        self.like = a
        self.t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        self.ptr = self.t.data_ptr()

    def back(self):
        return self.t.cpu().numpy().view(self.like.dtype).reshape(self.like.shape)


def _blank_like(x):
    return tuple(_blank(a.shape, a.dtype) for a in x) if isinstance(x, tuple) else _blank(x.shape, x.dtype)


def _dev_px(g, st):
    i0, i1 = _inputs()
    a, b, o = _Dev(i0["rgb"]), _Dev(i1["rgb"]), _Dev(_blank_like(i0["rgb"]))
    _sync()
    pkg._check(g._L.rife_hip_process_device_px(g._h, a.ptr, b.ptr, W, H, T, o.ptr, pkg.PIX_RGB8, st), "process_device_px", g._L)
    _sync()
    return (o.back(),)


def _dev_image(g, st):
    i0, i1 = _inputs()
    d = [[_Dev(p) for p in planes] for planes in (i0["i420"], i1["i420"], _blank_like(i0["i420"]))]
    img = [pkg.device_image(W, H, pkg.PIX_I420, [(p.ptr, p.like.strides[0]) for p in planes]) for planes in d]
    _sync()
    g.process_device_image(img[0], img[1], T, img[2], st)
    _sync()
    return tuple(p.back() for p in d[2])


def _dev_sets(g, st):
    i0, i1 = _inputs()
    a, b, o = _Dev(i0["rgb"]), _Dev(i1["rgb"]), _Dev(_blank_like(i0["rgb"]))
    p = [_Dev(x) for x in (i0["set"], i1["set"], _blank_like(i0["set"]))]
    desc = [pkg.planes_desc(W, H, pkg.SAMPLE_U16, [(x.ptr + k * H * W * 2, W * 2) for k in range(2)], 4095) for x in p]
    _sync()
    g.process_device_apply_sets(a.ptr, b.ptr, W, H, T, o.ptr, [pkg.apply_set_desc(desc[0], desc[1], desc[2])], stream=st)
    _sync()
    return o.back(), p[2].back()


def _dev_hbd(g, st):
    i0, i1 = _inputs()
    d = [[_Dev(p) for p in planes] for planes in (i0["hbd"], i1["hbd"], _blank_like(i0["hbd"]))]
    img = [pkg.device_image(W, H, pkg.PIX_I420P10, [(p.ptr, p.like.strides[0]) for p in planes]) for planes in d]
    _sync()
    g.process_device_hbd(img[0], img[1], T, img[2], 12, stream=st)
    _sync()
    return tuple(p.back() for p in d[2])


def _dev_packed(g, st):
    i0, i1 = _inputs()
    d = [_Dev(x) for x in (i0["packed"], i1["packed"], _blank_like(i0["packed"]))]
    img = [pkg.packed_desc(W, H, 3, 16, x.ptr, W * 6) for x in d]
    _sync()
    g.process_device_hbd_packed(img[0], img[1], T, img[2], stream=st)
    _sync()
    return (d[2].back(),)


def _dev_sp(g, st):
    i0, i1 = _inputs()
    d = [[_Dev(p) for p in planes] for planes in (i0["sp"], i1["sp"], _blank_like(i0["sp"]))]
    img = [pkg.semiplanar_desc(W, H, 1, 10, s[0].ptr, W * 2, s[1].ptr, CW * 4) for s in d]
    _sync()
    g.process_device_hbd_semiplanar(img[0], img[1], T, img[2], stream=st)
    _sync()
    return tuple(p.back() for p in d[2])


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- the host twins ----
def _host_px(g):
    i0, i1 = _inputs()
    out = _blank_like(i0["rgb"])
    pkg._check(g._L.rife_hip_process_px(g._h, pkg._p(i0["rgb"]), pkg._p(i1["rgb"]), W, H, T, pkg._p(out), pkg.PIX_RGB8), "process_px", g._L)
    return (out,)


def _host_image(g):
    i0, i1 = _inputs()
    out = _blank_like(i0["i420"])
    views = lambda planes: tuple(p[:, :n] for p, n in zip(planes, (W, CW, CW)))
    g.process_planes(views(i0["i420"]), views(i1["i420"]), T, pkg.PIX_I420, out=views(out))
    return out


def _host_sets(g):
    i0, i1 = _inputs()
    frame, planes = _blank_like(i0["rgb"]), _blank_like(i0["set"])
    g.process_apply_sets(i0["rgb"], i1["rgb"], T, [pkg.apply_set(i0["set"], i1["set"], maxval=4095, out=planes)], outimage=frame)
    return frame, planes


def _host_hbd(g):
    i0, i1 = _inputs()
    return g.process_hbd(i0["hbd"], i1["hbd"], T, 12, pkg.PIX_I420P10, out=_blank_like(i0["hbd"]))


def _host_packed(g):
    i0, i1 = _inputs()
    return (g.process_hbd_packed(i0["packed"], i1["packed"], T, 16, out=_blank_like(i0["packed"])),)


def _host_sp(g):
    i0, i1 = _inputs()
    return g.process_hbd_semiplanar(i0["sp"], i1["sp"], T, 10, 1, out=_blank_like(i0["sp"]))


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), "%s, array %d: %d elements differ from a fresh engine's" % (what, k, int((a != b).sum()))


def _assert_written(out, what):
    for k, a in enumerate(out):
        assert len(np.unique(a.view(np.uint8))) > 8, "%s, array %d: a flat output checks nothing" % (what, k)


def test_device_entry_points_share_a_stream_workspace(modeldirs):
    import torch
    calls = [("px", _dev_px), ("image", _dev_image), ("apply_sets", _dev_sets), ("hbd", _dev_hbd), ("hbd_packed", _dev_packed), ("hbd_semiplanar", _dev_sp), ("px", _dev_px)]
    want = {}
    for name, call in calls[:-1]:
        want[name] = call(_fresh(modeldirs), None)
        _assert_written(want[name], "process_device_" + name)
    assert not np.array_equal(want["px"][0], _inputs()[0]["rgb"]), "a pair without motion checks nothing"
    g = _fresh(modeldirs)
    user = torch.cuda.Stream()
    for st in (None, user.cuda_stream):
        for k, (name, call) in enumerate(calls):
            _assert_same(call(g, st), want[name], "call %d, process_device_%s on %s" % (k, name, "the NULL stream" if st is None else "a caller's stream"))


def test_host_entry_points_share_the_pool(modeldirs):
    calls = [("px", _host_px), ("image", _host_image), ("apply_sets", _host_sets), ("hbd", _host_hbd), ("hbd_packed", _host_packed), ("hbd_semiplanar", _host_sp)]
    want = {}
    for name, call in calls:
        want[name] = call(_fresh(modeldirs, test_build=True))
        _assert_written(want[name], "process_" + name)
    g = _fresh(modeldirs, test_build=True)
    for rnd in range(2):
        for k, (name, call) in enumerate(calls):
            _assert_same(call(g), want[name], "round %d, call %d, process_%s" % (rnd, k, name))
    assert g.pool_state()[1] == 0, "a host call kept its lease"
