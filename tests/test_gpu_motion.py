"""Motion export (include/rife_hip.h rife_hip_motion_t) on the GPU: the final flows and the blend mask, stored by the kernel that finishes the frame.

  1  single launches of the four motion kernels through rife_hip_op_tail_motion (test build), tail_ref's planted, far and dense cases: flow byte for byte
     (dense: tail_ref's bar for inexact deltas), mask within 2^-20 (F16: an admissible half), the frame byte-identical to rife_hip_op_tail's, guard bytes and pitch
     gaps untouched, null flow / null mask leave the other buffer's bytes alone.  The bars are derived in tests/motion_ref.py.
  2  end to end against the oracle's blobs (tests/motion_ref.py E2E; tests/test_motion_host.py holds the oracle to the same conditions without a GPU).
  3  the motion is the frame's: the returned frame is rebuilt from the returned motion and the input codes, at precision full and fast.
  4  the product library: same frame bytes as process_px in five formats; host, device and stream-mode calls agree; F16 is the RNE half of F32; timestep 0 / 1;
     a plain call after a motion call; two caller threads.
  5  refusals: every other family and -x / -z, -ENOSYS with the family or mode and "motion export" in the message, outputs untouched."""
import ctypes
import importlib
import os
import threading

import numpy as np
import pytest

import motion_ref as mr
import s16_ref
import tail_ref as tr

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("rife-ncnn-vulkan_amd")
amd = pkg.test_build()      # librife_hip_test.so: single-kernel entry points (include/rife_hip_test.h) and the kernel-selection switches

_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None
_FMT = {tr.PIX_RGB8: "rgb8", tr.PIX_A2B10G10R10: "a2b10g10r10"}
_MO = {mr.MOTION_F32: "f32", mr.MOTION_F16: "f16"}
_KERNEL = {tr.TAIL_RS: "tail_rs", tr.TAIL_HEAD_S16: "head_final_s16", tr.TAIL_HEAD_F32: "head_final_f32", tr.TAIL_UNFUSED: "head_ps+k_final"}
_S16 = {}
FILL = 0x5a


def _trunk(kind, w, h, depth, kernel, c):
    if kernel == tr.TAIL_HEAD_F32:
        return c["x"]
    key = (kind, w, h, depth)
    if key not in _S16:
        wp, hp = tr.padded(w, h)
        _S16[key] = s16_ref.pack(c["x"], hp // 4, wp // 4)
    return _S16[key]


def _pattern(n, k):
    return ((np.arange(n, dtype=np.int64) * k + 11) & 0xff).astype(np.uint8)


def _rows(buf, h, pitch, row):
    """(the h rows' payload (h, row) uint8, everything else of the guarded buffer as one flat array)"""
    body = buf[tr.GUARD:tr.GUARD + h * pitch].reshape(h, pitch)
    return body[:, :row], np.concatenate([buf[:tr.GUARD], body[:, row:].reshape(-1), buf[tr.GUARD + h * pitch:]])


def _single(kind, kernel, w, h, cus, pixfmt, fmt, pad):
    depth = tr.depth_of(pixfmt)
    c = tr.cached(kind, w, h, depth)
    es = 2 if fmt == mr.MOTION_F16 else 4
    frow, mrow = w * 4 * es, w * es
    fp, mp = frow + pad, mrow + pad
    nframe = w * h * (3 if pixfmt == tr.PIX_RGB8 else 4)
    out0 = _pattern(nframe + 2 * tr.GUARD, 37); f0 = _pattern(h * fp + 2 * tr.GUARD, 29); m0 = _pattern(h * mp + 2 * tr.GUARD, 53)
    args = (kernel, pixfmt, w, h, _trunk(kind, w, h, depth, kernel, c), c["wgt"], c["b"], c["F"], c["M"], c["img0"], c["img1"], out0)
    frame, fb, mb = amd.op_tail_motion(*args, fmt=fmt, flow=f0, flow_pitch=fp, mask=m0, mask_pitch=mp, cus=cus)
    # the frame of the same launch is rife_hip_op_tail's, guards included
    plain = amd.op_tail(*args, cus=cus)
    assert np.array_equal(frame, plain), "the motion kernel's frame differs from the plain kernel's in %d bytes" % int((frame != plain).sum())
    # guards and pitch gaps
    fpay, frest = _rows(fb, h, fp, frow); mpay, mrest = _rows(mb, h, mp, mrow)
    assert np.array_equal(frest, _rows(f0, h, fp, frow)[1]), "bytes around the flow rows were written"
    assert np.array_equal(mrest, _rows(m0, h, mp, mrow)[1]), "bytes around the mask rows were written"
    dt = mr.DTYPE[fmt]
    flow = np.ascontiguousarray(fpay).view(dt).reshape(h, w, 4); mask = np.ascontiguousarray(mpay).view(dt).reshape(h, w)
    # null flow, then null mask: the other buffer has the same bytes
    _, none, mb2 = amd.op_tail_motion(*args, fmt=fmt, flow=None, mask=m0, mask_pitch=mp, cus=cus)
    assert none is None and np.array_equal(mb2, mb), "the mask differs when the flow is not wanted"
    _, fb2, none = amd.op_tail_motion(*args, fmt=fmt, flow=f0, flow_pitch=fp, mask=None, cus=cus)
    assert none is None and np.array_equal(fb2, fb), "the flow differs when the mask is not wanted"
    return c, flow, mask


def _hold_mask(mask, want, fmt, what):
    if fmt == mr.MOTION_F32:
        err = np.abs(mask.astype(np.float64) - want)
        print("motion %s: mask max |err| %.3g (bar 2^-20 = %.3g)" % (what, err.max(), mr.MASK_TOL))
        assert err.max() <= mr.MASK_TOL, (what, float(err.max()))
    else:
        ok = mr.mask_half_ok(mask, want)
        print("motion %s: %d of %d half masks are not the half of the reference itself" % (what, int((mask != want.astype(np.float16)).sum()), mask.size))
        assert ok.all(), (what, int((~ok).sum()))


def _exact_case(kind, case, pixfmt, fmt):
    kernel, w, h, cus = case
    c, flow, mask = _single(kind, kernel, w, h, cus, pixfmt, fmt, 0 if pixfmt == tr.PIX_RGB8 else 48)
    wf, wm = mr.expected(c, w, h)
    want = wf.astype(np.float32) if fmt == mr.MOTION_F32 else mr.half(wf.astype(np.float32))
    assert np.array_equal(wf.astype(np.float32).astype(np.float64), wf)
    bits = np.uint32 if fmt == mr.MOTION_F32 else np.uint16
    bad = flow.view(bits) != want.view(bits)
    assert not bad.any(), "%d of %d flow samples are not the reference's bits; first at %s: got %r, want %r" % (
        int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), flow[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
    _hold_mask(mask, wm, fmt, "%s %s %s %s %dx%d cus %d" % (kind, _KERNEL[kernel], _FMT[pixfmt], _MO[fmt], w, h, cus))


@pytest.mark.parametrize("fmt", [mr.MOTION_F32, mr.MOTION_F16], ids=lambda f: _MO[f])
@pytest.mark.parametrize("pixfmt", [tr.PIX_RGB8, tr.PIX_A2B10G10R10], ids=lambda p: _FMT[p])
@pytest.mark.parametrize("case", tr.CASES, ids=_ids)
def test_planted_single_launch(case, pixfmt, fmt):
    _exact_case("planted", case, pixfmt, fmt)


FAR = [(k, w, h, cus) for k in (tr.TAIL_RS, tr.TAIL_HEAD_S16, tr.TAIL_HEAD_F32, tr.TAIL_UNFUSED) for (w, h, cus) in ((100, 60, 3 if k == tr.TAIL_RS else 0), (257, 130, 7 if k == tr.TAIL_RS else 0))]


@pytest.mark.parametrize("fmt", [mr.MOTION_F32, mr.MOTION_F16], ids=lambda f: _MO[f])
@pytest.mark.parametrize("pixfmt", [tr.PIX_RGB8, tr.PIX_A2B10G10R10], ids=lambda p: _FMT[p])
@pytest.mark.parametrize("case", FAR, ids=_ids)
def test_far_single_launch(case, pixfmt, fmt):
    _exact_case("far", case, pixfmt, fmt)


@pytest.mark.parametrize("fmt", [mr.MOTION_F32, mr.MOTION_F16], ids=lambda f: _MO[f])
@pytest.mark.parametrize("case", tr.DENSE_CASES, ids=_ids)
def test_dense_single_launch(case, fmt):
    kernel, w, h, cus = case
    c, flow, mask = _single("dense", kernel, w, h, cus, tr.PIX_RGB8, fmt, 48)
    wf, wm = mr.expected(c, w, h)
    tol = mr.DENSE_FLOW_TOL(c["dmax"])
    if fmt == mr.MOTION_F32:
        err = np.abs(flow.astype(np.float64) - wf).max()
        print("motion dense %s %dx%d cus %d: flow max |err| %.3g px (bar %.3g)" % (_KERNEL[kernel], w, h, cus, err, tol))
        assert err <= tol
    else:      # the RNE half of some value within the bar: rounding is monotone
        g = flow.astype(np.float64)
        assert ((g >= (wf - tol).astype(np.float16).astype(np.float64)) & (g <= (wf + tol).astype(np.float16).astype(np.float64))).all()
    _hold_mask(mask, wm, fmt, "dense %s %s %dx%d cus %d" % (_KERNEL[kernel], _MO[fmt], w, h, cus))


def test_single_launch_refusals():
    c = tr.cached("planted", 100, 60, 8)
    w, h = 100, 60
    args = (tr.TAIL_HEAD_S16, tr.PIX_RGB8, w, h, _trunk("planted", w, h, 8, tr.TAIL_HEAD_S16, c), c["wgt"], c["b"], c["F"], c["M"], c["img0"], c["img1"], _pattern(w * h * 3 + 2 * tr.GUARD, 37))
    f0 = _pattern(h * w * 16 + 2 * tr.GUARD, 29)
    for kw, word in ((dict(fmt=2, flow=f0, flow_pitch=w * 16), "unknown motion format"), (dict(fmt=0), "both NULL"),
                     (dict(fmt=0, flow=_pattern(h * (w * 16 - 16) + 2 * tr.GUARD, 29), flow_pitch=w * 16 - 16), "smaller than the row bytes"),
                     (dict(fmt=0, flow=_pattern(h * (w * 16 + 4) + 2 * tr.GUARD, 29), flow_pitch=w * 16 + 4), "not a multiple of 16")):
        with pytest.raises(pkg.RifeError) as ex:
            amd.op_tail_motion(*args, **kw)
        assert "(-1)" in str(ex.value) and word in str(ex.value), str(ex.value)


# ---- 2, 3: end to end -------------------------------------------------------------------------------------------------------------------------------------------
_ENG = {}


def _engine(modeldirs, name, precision="full"):
    """the engine an end-to-end case runs on: the product, except "rs" - the test build with the row-streaming tail at every frame size"""
    key = (name == "rs", mr.E2E[name][3], precision)
    if key not in _ENG:
        if name == "rs":
            old = os.environ.get("RIFE_HIP_TAIL_RS")
            os.environ["RIFE_HIP_TAIL_RS"] = "2"                          # read at create time (tests/test_gpu_tail_rs.py)
            try:
                g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
            finally:
                if old is None: del os.environ["RIFE_HIP_TAIL_RS"]
                else: os.environ["RIFE_HIP_TAIL_RS"] = old
        else:
            g = pkg.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
        if mr.E2E[name][3] == 2:
            g.set_flow_scale(2)
        g.set_precision(precision)
        _ENG[key] = g
    return _ENG[key]


@pytest.mark.parametrize("name", sorted(mr.E2E))
def test_motion_against_the_oracle_blobs(name, modeldirs, tmp_path_factory):
    o = mr.oracle_motion(name, modeldirs["rife-v4.6"], tmp_path_factory.getbasetemp())
    g = _engine(modeldirs, name)
    frame, flow, mask = g.process_motion(o["a"], o["b"], 0.5)
    assert np.array_equal(frame, g.process(o["a"], o["b"], 0.5)), "the frame of a motion call is not the plain call's"
    fe, me = np.abs(flow.astype(np.float64) - o["flow"]).max(), np.abs(mask.astype(np.float64) - o["mask"]).max()
    print("motion_parity %s %dx%d scale %d: flow max |err| %.3g px (bar %.0e), mask max |err| %.3g (bar %.0e)" % (name, mr.E2E[name][1], mr.E2E[name][2], mr.E2E[name][3], fe, mr.E2E_FLOW_TOL, me, mr.E2E_MASK_TOL))
    assert fe <= mr.E2E_FLOW_TOL and me <= mr.E2E_MASK_TOL


@pytest.mark.parametrize("precision", ["full", "fast"])
@pytest.mark.parametrize("name", sorted(mr.E2E))
def test_the_motion_is_the_frames(name, precision, modeldirs):
    """The returned frame, rebuilt from the RETURNED motion and the input codes: a stale flow, another lane's mask or a value from before block 3's update fails."""
    a, b = mr.e2e_pair(name)
    g = _engine(modeldirs, name, precision)
    frame, flow, mask = g.process_motion(a, b, 0.5)
    val, amax = mr.rebuilt((a, b), flow, mask, 32 * mr.E2E[name][3])
    ok, frac = mr.frame_matches(frame, val, amax, 8)
    print("motion_rebuild %s %s: boundary set %.4f of the codes" % (name, precision, frac))
    assert frac < tr.CAP and ok


# ---- 4: the product library ------------------------------------------------------------------------------------------------------------------------------------
W4, H4 = 100, 60


@pytest.fixture(scope="module")
def g(modeldirs):
    e = pkg.RIFE(0, rife_v4=True); e.load(modeldirs["rife-v4.6"])
    return e


def _formats(a):
    """the frame `a` (h, w, 3) uint8 in five _px formats, as flat uint8 buffers"""
    h, w, _ = a.shape
    c10 = (a.astype(np.uint16) << 2) | (a >> 6)
    nv12 = np.concatenate([a[..., 1].reshape(-1), np.ascontiguousarray(a[::2, ::2, ::2][..., :2]).reshape(-1)])
    assert nv12.size == pkg.frame_bytes(w, h, pkg.PIX_NV12)
    return {pkg.PIX_RGB8: a.reshape(-1), pkg.PIX_A2B10G10R10: pkg.pack_a2b10g10r10(c10).view(np.uint8).reshape(-1),
            pkg.PIX_RGBA8: np.ascontiguousarray(np.dstack([a, a[..., :1] ^ 0xff])).reshape(-1), pkg.PIX_NV12: np.ascontiguousarray(nv12),
            pkg.PIX_RGBPF: np.ascontiguousarray((a.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).view(np.uint8).reshape(-1)}


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _host_call(e, fa, fb, t, px, w, h, fmt=mr.MOTION_F32, pad=0, want_flow=True, want_mask=True):
    es = 2 if fmt == mr.MOTION_F16 else 4
    out = np.full(fa.size, FILL, np.uint8)
    fbuf = np.full((h, w * 4 * es + pad), FILL, np.uint8); mbuf = np.full((h, w * es + pad), FILL, np.uint8)
    d = pkg.motion_desc(fbuf.ctypes.data if want_flow else None, mbuf.ctypes.data if want_mask else None, fmt, fbuf.strides[0], mbuf.strides[0])
    rc = e._L.rife_hip_process_motion(e._h, _p(fa), _p(fb), w, h, float(t), _p(out), px, ctypes.byref(d))
    return rc, out, fbuf, mbuf


def test_the_frame_is_process_px_in_every_format(g):
    a, b = mr.e2e_pair("ragged")
    fa, fb = _formats(a), _formats(b)
    for px in fa:
        want = np.full(fa[px].size, FILL, np.uint8)
        assert g._L.rife_hip_process_px(g._h, _p(fa[px]), _p(fb[px]), W4, H4, 0.5, _p(want), px) == 0
        rc, out, fbuf, mbuf = _host_call(g, fa[px], fb[px], 0.5, px, W4, H4, pad=32)
        assert rc == 0, g._L.rife_hip_last_error()
        assert np.array_equal(out, want), "pixfmt %d: the frame of the motion call differs from process_px in %d bytes" % (px, int((out != want).sum()))
        assert (fbuf[:, W4 * 16:] == FILL).all() and (mbuf[:, W4 * 4:] == FILL).all(), "pitch gaps were written"
        m = np.ascontiguousarray(mbuf[:, :W4 * 4]).view(np.float32)
        assert np.isfinite(m).all() and 0.0 < m.min() and m.max() < 1.0
        after = np.full(fa[px].size, FILL, np.uint8)      # a plain call after a motion call returns its usual bytes
        assert g._L.rife_hip_process_px(g._h, _p(fa[px]), _p(fb[px]), W4, H4, 0.5, _p(after), px) == 0 and np.array_equal(after, want)


def test_host_device_and_stream_mode_agree_and_f16_is_the_half_of_f32(g):
    import torch
    a, b = mr.e2e_pair("ragged")
    frame, flow, mask = g.process_motion(a, b, 0.5)
    again = g.process_motion(a, b, 0.5)
    assert np.array_equal(again[1].view(np.uint32), flow.view(np.uint32)) and np.array_equal(again[2].view(np.uint32), mask.view(np.uint32)), "two calls differ"
    # row-padded arrays and views are filled in place
    big = np.full((H4, W4 + 3, 4), 7.0, np.float32); mk = np.full((H4 + 2, W4 + 5), 7.0, np.float32)
    _, f2, m2 = g.process_motion(a, b, 0.5, flow=big[:, :W4], mask=mk[1:H4 + 1, 2:W4 + 2])
    assert np.array_equal(f2, flow) and np.array_equal(m2, mask) and (big[:, W4:] == 7.0).all() and (mk[0] == 7.0).all() and (mk[:, :2] == 7.0).all() and (mk[:, W4 + 2:] == 7.0).all()
    # F16: the RNE half of the F32 result of the same call, exactly; and one buffer alone
    _, fh, mh = g.process_motion(a, b, 0.5, dtype=np.float16)
    assert np.array_equal(fh.view(np.uint16), mr.half(flow).view(np.uint16)) and np.array_equal(mh.view(np.uint16), mr.half(mask).view(np.uint16))
    _, f3, none = g.process_motion(a, b, 0.5, mask=False)
    assert none is None and np.array_equal(f3, flow)
    # stream mode
    u0, u1 = g.upload(a), g.upload(b)
    fr, ff, fm = g.process_frames_motion(u0, u1, 0.5)
    assert np.array_equal(fr, frame) and np.array_equal(ff, flow) and np.array_equal(fm, mask)
    # device buffers with padded rows, on the engine's stream and on a caller's
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for fmt, es, wf, wm in ((mr.MOTION_F32, 4, flow, mask), (mr.MOTION_F16, 2, fh, mh)):
        for stream in (None, torch.cuda.Stream()):
            do = torch.full((H4, W4, 3), FILL, dtype=torch.uint8, device="cuda")
            df = torch.full((H4, W4 * 4 * es + 32), FILL, dtype=torch.uint8, device="cuda"); dm = torch.full((H4, W4 * es + 32), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            d = pkg.motion_desc(df.data_ptr(), dm.data_ptr(), fmt, df.stride(0), dm.stride(0))
            g.process_device_motion(da.data_ptr(), db.data_ptr(), W4, H4, 0.5, do.data_ptr(), d, stream=stream.cuda_stream if stream else None)
            torch.cuda.synchronize()
            hf, hm = df.cpu().numpy(), dm.cpu().numpy()
            assert np.array_equal(do.cpu().numpy(), frame)
            assert np.array_equal(np.ascontiguousarray(hf[:, :W4 * 4 * es]).view(mr.DTYPE[fmt]).reshape(H4, W4, 4).view(np.uint16), wf.view(np.uint16))
            assert np.array_equal(np.ascontiguousarray(hm[:, :W4 * es]).view(mr.DTYPE[fmt]).view(np.uint16), wm.view(np.uint16))
            assert (hf[:, W4 * 4 * es:] == FILL).all() and (hm[:, W4 * es:] == FILL).all(), "pitch gaps of the device buffers were written"
    assert np.array_equal(g.process(a, b, 0.5), frame)      # a plain call after motion calls returns its usual bytes


def test_timestep_0_and_1_give_zero_flow_and_a_constant_mask(g):
    import torch
    a, b = mr.e2e_pair("ragged")
    for t, src in ((0.0, a), (1.0, b)):
        for dt in (np.float32, np.float16):
            frame, flow, mask = g.process_motion(a, b, t, dtype=dt)
            assert np.array_equal(frame, src) and not flow.view(np.uint16).any() and (mask == dt(1.0 - t)).all()
            u0, u1 = g.upload(a), g.upload(b)
            fr, ff, fm = g.process_frames_motion(u0, u1, t, dtype=dt)
            assert np.array_equal(fr, src) and not ff.view(np.uint16).any() and (fm == dt(1.0 - t)).all()
            es = np.dtype(dt).itemsize
            da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            do = torch.zeros((H4, W4, 3), dtype=torch.uint8, device="cuda")
            df = torch.full((H4, W4 * 4 * es + 16), FILL, dtype=torch.uint8, device="cuda"); dm = torch.full((H4, W4 * es + 16), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            g.process_device_motion(da.data_ptr(), db.data_ptr(), W4, H4, t, do.data_ptr(), pkg.motion_desc(df.data_ptr(), dm.data_ptr(), 0 if dt == np.float32 else 1, df.stride(0), dm.stride(0)))
            torch.cuda.synchronize()
            hf, hm = df.cpu().numpy(), dm.cpu().numpy()
            assert np.array_equal(do.cpu().numpy(), src) and not hf[:, :W4 * 4 * es].any() and (hf[:, W4 * 4 * es:] == FILL).all() and (hm[:, W4 * es:] == FILL).all()
            assert (np.ascontiguousarray(hm[:, :W4 * es]).view(dt) == dt(1.0 - t)).all()


def test_two_caller_threads(g):
    a, b = mr.e2e_pair("ragged")
    want = g.process_motion(a, b, 0.5)
    got = [None, None]

    def work(i):
        got[i] = [g.process_motion(a, b, 0.5) for _ in range(3)]
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    for runs in got:
        assert runs is not None
        for fr, fl, mk in runs:
            assert np.array_equal(fr, want[0]) and np.array_equal(fl.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(mk.view(np.uint32), want[2].view(np.uint32))


# ---- 5: refusals --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife-v3.1", {}, "rife-v3"), ("rife", {}, "rife (v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    e = pkg.RIFE(0, **fl); e.load(modeldirs[fam])
    w, h = 64, 64
    a = np.zeros((h, w, 3), np.uint8)
    for t in (0.5, 0.0):
        rc, out, fbuf, mbuf = _host_call(e, a.reshape(-1), a.reshape(-1), t, pkg.PIX_RGB8, w, h)
        msg = e._L.rife_hip_last_error().decode()
        assert rc == -pkg.ENOSYS and word in msg and "motion export" in msg, (rc, msg)
        assert (out == FILL).all() and (fbuf == FILL).all() and (mbuf == FILL).all(), "a refused call wrote into an output buffer"
        da = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        do = torch.full((h, w, 3), FILL, dtype=torch.uint8, device="cuda"); df = torch.full((h, w * 16), FILL, dtype=torch.uint8, device="cuda"); dm = torch.full((h, w * 4), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pkg.RifeError) as ex:
            e.process_device_motion(da.data_ptr(), da.data_ptr(), w, h, t, do.data_ptr(), pkg.motion_desc(df.data_ptr(), dm.data_ptr(), 0, w * 16, w * 4))
        assert "(-6)" in str(ex.value) and word in str(ex.value) and "motion export" in str(ex.value), str(ex.value)
        torch.cuda.synchronize()
        assert (do == FILL).all().item() and (df == FILL).all().item() and (dm == FILL).all().item()
    if fam.startswith("rife-v4"):      # resident frames exist for these engines: the stream-mode call refuses alike
        u = e.upload(a)
        with pytest.raises(pkg.RifeError) as ex:
            e.process_frames_motion(u, u, 0.5)
        assert "(-6)" in str(ex.value) and "motion export" in str(ex.value)
