"""Apply motion (include/rife_hip.h rife_hip_planes_t) on the GPU: the exported motion applied to the caller's own planes.

  1  single launches of k_apply_motion through rife_hip_op_apply (test build), the vector form and the forced one-pixel-per-lane form on the same input: apply_ref's
     planted and far cases byte for byte, its dense cases within the bars derived in tests/apply_ref.py; row padding of the output keeps its bytes.
  2  pitched planes in device memory: row padding, pointers off by one element (the scalar form for real), a window inside a larger allocation filled with a sentinel.
  3  the engine against itself: process_motion, then apply_motion on the split u8 planes with padded_size, equals the call's own frame outside the boundary set;
     the alpha byte of an RGBA8 call against apply_motion on the alpha planes with extent w, h; flow scale 1 and 2.
  4  the contract: process_apply / process_device_apply are byte for byte process_*_motion (F32) then apply_*; frame not wanted; u16 / 65535 and float planes;
     timestep 0 / 1; fast precision.
  5  apply_motion on an engine that has loaded no model, and on a rife-v2.3 engine.
  6  refusals of process_apply on other families and -x / -z: -ENOSYS, the words "apply motion", outputs untouched."""
import ctypes
import importlib

import numpy as np
import pytest

import apply_ref as ar
import motion_ref as mr
import tail_ref as tr

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")
amd = pkg.test_build()

_S = {ar.SAMPLE_U8: "u8", ar.SAMPLE_U16: "u16", ar.SAMPLE_F16: "f16", ar.SAMPLE_F32: "f32"}
FILL = 0x5a
KINDS = [(ar.SAMPLE_U8, 255), (ar.SAMPLE_U16, 1023), (ar.SAMPLE_U16, 65535), (ar.SAMPLE_F16, 0), (ar.SAMPLE_F32, 0)]
_kid = lambda k: "%s-%d" % (_S[k[0]], k[1])
_sid = lambda s: "%dx%d" % s


def _extents(w, h):
    return [(w, h), ar.padded(w, h, 32), ar.padded(w, h, 64)]


def _out(c, pad):
    """n output planes inside one sentinel-filled array with `pad` samples of row padding: (planes, the array).  (w + pad) % 8 == 0 and numpy's 16-byte base keep every
    plane store-aligned, so force_scalar = 0 is the vector form."""
    n, h, w = c["p0"].shape
    big = np.frombuffer(np.full(n * h * (w + pad) * c["p0"].itemsize, FILL, np.uint8), c["p0"].dtype).reshape(n, h, w + pad).copy()
    assert big.ctypes.data % 16 == 0
    return tuple(big[k, :, :w] for k in range(n)), big


def _launch(c, force_scalar):
    n, h, w = c["p0"].shape
    pad = (-w) % 8 + 8
    planes, big = _out(c, pad)
    amd.op_apply(c["p0"], c["p1"], c["flow"], c["mask"], planes, maxval=c["maxval"] or None, extent=c["extent"], force_scalar=force_scalar)
    assert (big[:, :, w:].view(np.uint8) == FILL).all(), "row padding of the output planes was written"
    return np.ascontiguousarray(big[:, :, :w])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _exact(kind, w, h, n, sample, maxval, ext, half):
    c = ar.cached(kind, w, h, n, sample, maxval, ext, half)
    want = ar.expected_exact(c["ref"], sample, maxval)
    for fs in (0, 1):
        got = _launch(c, fs)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), "%s %s/%d %dx%d n %d extent %s %s motion, %s form: %d of %d bytes differ; first sample %s: got %r, want %r" % (
            kind, _S[sample], maxval, w, h, n, ext, "f16" if half else "f32", "scalar" if fs else "vector", int(bad.sum()), bad.size,
            tuple(np.argwhere(got != want)[0]), got[tuple(np.argwhere(got != want)[0])], want[tuple(np.argwhere(got != want)[0])])


@pytest.mark.parametrize("kind", KINDS, ids=_kid)
@pytest.mark.parametrize("size", ar.SIZES, ids=_sid)
def test_planted_single_launch(size, kind):
    w, h = size
    sample, maxval = kind
    for n in (1, 3, 4):
        for ext in _extents(w, h):
            for half in (False, True):
                if n != 3 and (half or ext != (w, h)):
                    continue      # the plane count is a loop bound: every extent and motion format at n = 3, the other counts once
                _exact("planted", w, h, n, sample, maxval, ext, half)


@pytest.mark.parametrize("kind", [k for k in KINDS if k[1] <= 1023], ids=_kid)
@pytest.mark.parametrize("size", ar.SIZES[1:], ids=_sid)
def test_far_single_launch(size, kind):
    w, h = size
    sample, maxval = kind
    for ext in _extents(w, h):
        for half in (False, True):
            _exact("far", w, h, 3, sample, maxval, ext, half)


@pytest.mark.parametrize("kind", ar.DENSE_KINDS + [ar.DENSE_WIDE], ids=_kid)
@pytest.mark.parametrize("size", ar.SIZES[1:], ids=_sid)
def test_dense_single_launch(size, kind):
    w, h = size
    sample, maxval = kind
    for ext in _extents(w, h)[:2]:
        for half in (False, True):
            c = ar.cached("dense", w, h, 3, sample, maxval, ext, half)
            got = [_launch(c, fs) for fs in (0, 1)]
            assert np.array_equal(_bits(got[0]), _bits(got[1])), "the vector and the scalar form differ"
            ok, fig = ar.holds(got[0], c["ref"], sample, maxval, equality=kind != ar.DENSE_WIDE)
            print("apply dense %s/%d %dx%d extent %s %s motion: %s" % (_S[sample], maxval, w, h, ext, "f16" if half else "f32", fig))
            assert ok, fig


def test_single_launch_refusals():
    c = ar.cached("planted", 33, 47, 3, ar.SAMPLE_U16, 1023)
    planes, _ = _out(c, 7)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*the extent"):
        amd.op_apply(c["p0"], c["p1"], c["flow"], c["mask"], planes, maxval=1023, extent=(32, 47))
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*differ"):
        amd.op_apply(c["p0"], c["p1"][:2], c["flow"], c["mask"], planes, maxval=1023)
    with pytest.raises(pkg.RifeError, match=r"\(-1\).*force_scalar"):
        amd.op_apply(c["p0"], c["p1"], c["flow"], c["mask"], planes, maxval=1023, force_scalar=2)


# ---- 2: pitched planes in device memory ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare():
    """an engine that has loaded no model: the apply calls need only its device"""
    return pkg.RIFE(0, rife_v4=True)


def _dev_window(torch, arrs, es, off, pad):
    """n planes (h, w) -> one sentinel-filled uint8 device buffer with every plane in a window: `off` bytes into its slot, rows padded by `pad` bytes, 64 bytes of
    sentinel around each slot.  Returns (buffer, [(byte offset, pitch)], the host image of the buffer before the planes went in)."""
    n = len(arrs); h, w = arrs[0].shape
    pitch = w * es + pad
    slot = 64 + off + h * pitch + 64
    slot = (slot + 15) // 16 * 16
    host = np.full(n * slot, FILL, np.uint8)
    where = []
    for k, a in enumerate(arrs):
        o = k * slot + 64 + off
        rows = host[o:o + h * pitch].reshape(h, pitch)
        rows[:, :w * es] = np.ascontiguousarray(a).view(np.uint8).reshape(h, w * es)
        where.append((o, pitch))
    return torch.from_numpy(host).cuda(), where, host


@pytest.mark.parametrize("kind", KINDS, ids=_kid)
@pytest.mark.parametrize("off_elems,pad_elems", [(0, 8), (1, 3)], ids=["aligned", "off-by-one-element"])
def test_pitched_device_planes(bare, kind, off_elems, pad_elems):
    import torch
    sample, maxval = kind
    w, h, n = 100, 60, 3
    c = ar.cached("planted", w, h, n, sample, maxval, ar.padded(w, h))
    es = c["p0"].itemsize
    d0, w0, _ = _dev_window(torch, list(c["p0"]), es, off_elems * es, pad_elems * es)
    d1, w1, _ = _dev_window(torch, list(c["p1"]), es, off_elems * es, pad_elems * es)
    blank = np.frombuffer(np.full(h * w * es, FILL, np.uint8), c["p0"].dtype).reshape(h, w)
    do, wo, before = _dev_window(torch, [blank] * n, es, off_elems * es, pad_elems * es)
    assert (before == FILL).all()
    fpad, mpad = 32, 8
    df = torch.full((h, w * 16 + fpad), FILL, dtype=torch.uint8, device="cuda"); dm = torch.full((h, w * 4 + mpad), FILL, dtype=torch.uint8, device="cuda")
    df[:, :w * 16] = torch.from_numpy(_bits(c["flow"]).reshape(h, w * 16)).cuda(); dm[:, :w * 4] = torch.from_numpy(_bits(c["mask"]).reshape(h, w * 4)).cuda()
    torch.cuda.synchronize()
    desc = lambda t, wh: pkg.planes_desc(w, h, sample, [(t.data_ptr() + o, p) for o, p in wh], maxval or None)
    mo = pkg.motion_desc(df.data_ptr(), dm.data_ptr(), 0, df.stride(0), dm.stride(0))
    for stream in (None, torch.cuda.Stream()):
        bare.apply_device_motion(desc(d0, w0), desc(d1, w1), mo, desc(do, wo), extent=c["extent"], stream=stream.cuda_stream if stream else None)
        torch.cuda.synchronize()
        got = do.cpu().numpy()
        want = before.copy()
        exp = ar.expected_exact(c["ref"], sample, maxval)
        for k, (o, p) in enumerate(wo):
            want[o:o + h * p].reshape(h, p)[:, :w * es] = _bits(exp[k]).reshape(h, w * es)
        assert np.array_equal(got, want), "%d bytes differ (%d of them outside the windows' rows)" % (int((got != want).sum()), int(((got != want) & (want == FILL)).sum()))
        do.copy_(torch.from_numpy(before).cuda()); torch.cuda.synchronize()


# ---- 3: the engine against itself ------------------------------------------------------------------------------------------------------------------------------
_ENG = {}


def _engine(modeldirs, scale=1, precision="full"):
    key = (scale, precision)
    if key not in _ENG:
        g = pkg.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
        if scale == 2:
            g.set_flow_scale(2)
        g.set_precision(precision)
        _ENG[key] = g
    return _ENG[key]


@pytest.mark.parametrize("name", ["ragged", "scale2"])
def test_apply_reproduces_the_engines_own_frame_and_alpha(name, modeldirs):
    _, w, h, scale, _ = mr.E2E[name]
    g = _engine(modeldirs, scale)
    assert g.padded_size(w, h) == ar.padded(w, h, 32 * scale)
    a, b = mr.e2e_pair(name)
    frame, flow, mask = g.process_motion(a, b, 0.5)
    split = lambda x: np.ascontiguousarray(np.moveaxis(x, -1, 0))
    got = np.moveaxis(np.stack(g.apply_motion(split(a), split(b), flow, mask, extent=g.padded_size(w, h))), 0, -1)
    val, amax = mr.rebuilt((a, b), flow, mask, 32 * scale)
    ok, frac = mr.frame_matches(got, val, amax, 8)
    assert ok and frac < tr.CAP, "apply_motion is not the reference's frame"
    bnd = tr.boundary(dict(val=val), 2.0 ** -6 * amax)
    d = got.astype(np.int64) - frame.astype(np.int64)
    print("apply_vs_frame %s: boundary set %.4f, %d codes differ (all inside it)" % (name, frac, int((d != 0).sum())))
    assert not d[~bnd].any() and np.abs(d).max() <= 1, "apply_motion with the padded extent differs from the call's own frame outside the boundary set"
    # alpha: the fourth byte of an RGBA8 call is apply_motion on the alpha planes with edge semantics
    ys, xs = np.mgrid[0:h, 0:w]
    al0 = ((xs * 5 + ys * 3) % 256).astype(np.uint8); al1 = ((xs * 2 + ys * 7 + 40) % 256).astype(np.uint8)
    fr4, fl4, mk4 = g.process_motion(np.dstack([a, al0]), np.dstack([b, al1]), 0.5, pixfmt=pkg.PIX_RGBA8)
    assert np.array_equal(fl4, flow) and np.array_equal(mk4, mask) and np.array_equal(fr4[..., :3], frame)
    (ga,) = g.apply_motion(al0, al1, flow, mask)
    r = ar.apply64(al0[None], al1[None], flow, mask)
    ok, frac = mr.frame_matches(ga[..., None], np.moveaxis(r["v"], 0, -1) + 0.5, r["amax"], 8)
    assert ok and frac < tr.CAP
    bnd = tr.boundary(dict(val=np.moveaxis(r["v"], 0, -1) + 0.5), 2.0 ** -6 * r["amax"])[..., 0]
    d = ga.astype(np.int64) - fr4[..., 3].astype(np.int64)
    print("apply_vs_alpha %s: boundary set %.4f, %d codes differ" % (name, frac, int((d != 0).sum())))
    assert not d[~bnd].any() and np.abs(d).max() <= 1, "apply_motion with extent w, h differs from the call's alpha outside the boundary set"


# ---- 4: the contract ----------------------------------------------------------------------------------------------------------------------------------------------
def _aux(rng, w, h, sample, maxval, n=3):
    if ar.is_int(sample):
        return rng.integers(0, 65536 if sample == ar.SAMPLE_U16 else 256, (2, n, h, w)).astype(ar.DTYPE[sample])
    return (rng.random((2, n, h, w)) * 4 - 1).astype(ar.DTYPE[sample])


@pytest.mark.parametrize("precision", ["full", "fast"])
@pytest.mark.parametrize("kind", [(ar.SAMPLE_U8, 255), (ar.SAMPLE_U16, 65535), (ar.SAMPLE_U16, 1023), (ar.SAMPLE_F32, 0)], ids=_kid)
def test_process_apply_is_process_motion_then_apply_motion(kind, precision, modeldirs):
    sample, maxval = kind
    g = _engine(modeldirs, 1, precision)
    a, b = mr.e2e_pair("ragged")
    h, w = a.shape[:2]
    q = _aux(np.random.default_rng([4, sample, maxval]), w, h, sample, maxval)      # u16 / 1023: samples above maxval go in as stored, only the output is clamped
    ext = g.padded_size(w, h)
    frame, flow, mask = g.process_motion(a, b, 0.5)
    want = g.apply_motion(q[0], q[1], flow, mask, maxval=maxval or None, extent=ext)
    fr, got = g.process_apply(a, b, 0.5, q[0], q[1], maxval=maxval or None, extent=ext)
    assert np.array_equal(fr, frame), "the frame of process_apply is not process_motion's"
    for k in range(3):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), "plane %d: %d bytes differ" % (k, int((_bits(got[k]) != _bits(want[k])).sum()))
    if ar.is_int(sample):
        assert max(int(p.max()) for p in got) <= maxval
    # the frame not wanted; output planes with padded rows, written in place
    big = np.frombuffer(np.full(3 * h * (w + 5) * q.itemsize, FILL, np.uint8), q.dtype).reshape(3, h, w + 5).copy()
    none, got2 = g.process_apply(a, b, 0.5, q[0], q[1], maxval=maxval or None, extent=ext, out=big[:, :, :w], want_frame=False)
    assert none is None and np.array_equal(_bits(big[:, :, :w]), _bits(np.stack(want))) and (_bits(big[:, :, w:]) == FILL).all()
    # timestep 0 / 1: copies, integer samples clamped to maxval
    for t, src, fsrc in ((0.0, q[0], a), (1.0, q[1], b)):
        fr, got = g.process_apply(a, b, t, q[0], q[1], maxval=maxval or None, extent=ext)
        wantc = np.minimum(src, maxval).astype(src.dtype) if ar.is_int(sample) else src
        assert np.array_equal(fr, fsrc) and np.array_equal(_bits(np.stack(got)), _bits(wantc))
    assert np.array_equal(g.process(a, b, 0.5), frame)      # a plain call afterwards returns its usual bytes


@pytest.mark.parametrize("kind", [(ar.SAMPLE_U16, 65535), (ar.SAMPLE_F16, 0)], ids=_kid)
def test_process_device_apply_is_the_two_device_calls(kind, modeldirs):
    import torch
    sample, maxval = kind
    g = _engine(modeldirs)
    a, b = mr.e2e_pair("ragged")
    h, w = a.shape[:2]
    q = _aux(np.random.default_rng([5, sample]), w, h, sample, maxval)
    es = q.itemsize
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dq = torch.from_numpy(_bits(q).reshape(2, 3, h, w * es)).cuda()
    planes = lambda t: pkg.planes_desc(w, h, sample, [(t[k].data_ptr(), w * es) for k in range(3)], maxval or None)
    ext = g.padded_size(w, h)
    for t in (0.5, 0.0, 1.0):
        for stream in (None, torch.cuda.Stream()):
            st = stream.cuda_stream if stream else None
            do1 = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda"); do2 = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda")
            df = torch.zeros((h, w * 16), dtype=torch.uint8, device="cuda"); dm = torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda")
            o1 = torch.full((3, h, w * es), FILL, dtype=torch.uint8, device="cuda"); o2 = torch.full((3, h, w * es), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            mo = pkg.motion_desc(df.data_ptr(), dm.data_ptr(), 0, w * 16, w * 4)
            g.process_device_motion(da.data_ptr(), db.data_ptr(), w, h, t, do1.data_ptr(), mo, stream=st)
            g.apply_device_motion(planes(dq[0]), planes(dq[1]), mo, planes(o1), extent=ext, stream=st)
            g.process_device_apply(da.data_ptr(), db.data_ptr(), w, h, t, do2.data_ptr(), planes(dq[0]), planes(dq[1]), planes(o2), extent=ext, stream=st)
            torch.cuda.synchronize()
            assert torch.equal(do1, do2), "timestep %s: the frames differ" % t
            if t == 0.5:
                assert torch.equal(o1, o2), "the planes differ in %d bytes" % int((o1 != o2).sum().item())
            else:      # a copy of the frame's planes (flow 0 and mask 1 - t give the same samples wherever they are finite and within maxval)
                src = q[0] if t == 0.0 else q[1]
                assert np.array_equal(o2.cpu().numpy(), _bits(src).reshape(3, h, w * es))


# ---- 5: no model, another family ----------------------------------------------------------------------------------------------------------------------------------
def test_apply_motion_needs_no_model_and_serves_every_family(bare, modeldirs):
    v23 = pkg.RIFE(0, rife_v2=True); v23.load(modeldirs["rife-v2.3"])
    for e in (bare, v23):
        for sample, maxval in ((ar.SAMPLE_U16, 65535), (ar.SAMPLE_F16, 0)):
            c = ar.cached("planted", 100, 60, 3, sample, maxval, (128, 64))
            got = e.apply_motion(c["p0"], c["p1"], c["flow"], c["mask"], maxval=maxval or None, extent=(128, 64))
            assert np.array_equal(_bits(np.stack(got)), _bits(ar.expected_exact(c["ref"], sample, maxval)))
    with pytest.raises(pkg.RifeError, match="before load"):
        bare.process_apply(np.zeros((60, 100, 3), np.uint8), np.zeros((60, 100, 3), np.uint8), 0.5, c["p0"], c["p1"])
    assert bare.padded_size(100, 60) == (128, 64)


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife-v3.1", {}, "rife-v3"), ("rife", {}, "rife (v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = pkg.RIFE(0, **fl); e.load(modeldirs[fam])
    w, h = 64, 64
    a = np.zeros((h, w, 3), np.uint8)
    q = np.zeros((3, h, w), np.uint16)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for t in (0.5, 0.0):
        out = np.full((h, w, 3), FILL, np.uint8); po = np.full((3, h, w), FILL * 257, np.uint16)
        d0, do = pkg.planes_of(q), pkg.planes_of(po)
        rc = e._L.rife_hip_process_apply(e._h, p(a), p(a), w, h, t, p(out), 0, ctypes.byref(d0), ctypes.byref(d0), 0, 0, ctypes.byref(do))
        msg = e._L.rife_hip_last_error().decode()
        assert rc == -pkg.ENOSYS and word in msg and "apply motion" in msg, (rc, msg)
        assert (out == FILL).all() and (po == FILL * 257).all(), "a refused call wrote into an output buffer"
        da = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"); dq = torch.zeros((3, h, w * 2), dtype=torch.uint8, device="cuda")
        dout = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda"); dpo = torch.full((3, h, w * 2), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        planes = lambda tt: pkg.planes_desc(w, h, ar.SAMPLE_U16, [(tt[k].data_ptr(), w * 2) for k in range(3)])
        with pytest.raises(pkg.RifeError) as ex:
            e.process_device_apply(da.data_ptr(), da.data_ptr(), w, h, t, dout.data_ptr(), planes(dq), planes(dq), planes(dpo))
        assert "(-6)" in str(ex.value) and word in str(ex.value) and "apply motion" in str(ex.value), str(ex.value)
        torch.cuda.synchronize()
        assert (dout == FILL).all().item() and (dpo == FILL).all().item()
