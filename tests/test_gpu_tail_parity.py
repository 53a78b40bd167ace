"""The kernels that read the LAST S16 trunk tensor of block 3 and write the quantised frame, ONE launch at a time against a float64 reference (GPU box only).

  tail_rs_kernel<0, PX>                          launch_tail_rs                                        rife_hip_op_tail kernel 0
  head_h2_kernel<EPI_FINAL, true, PX>            launch_conv with the fused tail, S16 geometry         kernel 1
  head_h2_kernel<EPI_FINAL, false, PX>           the same on an fp32 NHWC tensor (fed hi + lo)         kernel 2
  head_h2_kernel<EPI_DECONV_PS> + k_final / k_final_px<PX>, as a pass launches them unfused            kernel 3

PX ranges over RGB8, RGB10_U16, A2B10G10R10 and RGBA8.  The entry point uses the product's layer upload and the product's launchers; `cus` sizes the persistent
grid of tail_rs_kernel, so that a small frame gives its workgroups the long ranges of the product's regime (16 steps and more, strip changes, mid-strip starts:
tests/tail_ref.py restates the ranges, tests/test_tail_ref.py asserts them).  tests/tail_ref.py holds the reference, tau and the cases; tests/test_tail_ref.py
checks every case's precondition, power and cap on the CPU.

The rule, for every case: a code may differ from the reference's by ONE only where the float64 value lies within tau of a rounding boundary (and then only to
the other side of that boundary); everywhere else the frame is held code for code.  The 256 guard bytes on either side of the frame still hold their pattern, and
a second call on the same inputs returns the same bytes.
  planted  the lo planes alone carry the flow deltas (a lost lo plane, lo product or K partial sum moves most of the frame by many codes): every row of the table x
           the four formats.
  dense    Gaussian activations and weights, max|d| < 4 px, tau with the head's dense bar on top: the hi path.
  far      flows that leave the padded frame, a few by hundreds of pixels: the clamps.
  refusals weights that are not fp16, an unknown pixfmt, kernel = 4: -RIFE_HIP_EINVAL."""
import ctypes
import importlib

import numpy as np
import pytest

import s16_ref
import tail_ref as tr

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()      # librife_hip_test.so: single-kernel entry points (include/rife_hip_test.h)

_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None
_FMT = {tr.PIX_RGB8: "rgb8", tr.PIX_RGB10_U16: "rgb10_u16", tr.PIX_A2B10G10R10: "a2b10g10r10", tr.PIX_RGBA8: "rgba8"}
_KERNEL = {tr.TAIL_RS: "tail_rs", tr.TAIL_HEAD_S16: "head_final_s16", tr.TAIL_HEAD_F32: "head_final_f32", tr.TAIL_UNFUSED: "head_ps+k_final"}
_S16 = {}
_FRAMES = {}      # (w, h, pixfmt) -> {kernel: frame bytes} of the planted cases at cus = 0: do the four kernels return the same bytes?


def _trunk(kind, w, h, depth, kernel, c):
    if kernel == tr.TAIL_HEAD_F32:
        return c["x"]                                                    # the fp32 value hi + lo
    key = (kind, w, h, depth)
    if key not in _S16:
        wp, hp = tr.padded(w, h)
        _S16[key] = s16_ref.pack(c["x"], hp // 4, wp // 4)
    return _S16[key]


def _frame_bytes(w, h, pixfmt):
    return w * h * {tr.PIX_RGB8: 3, tr.PIX_RGB10_U16: 6, tr.PIX_A2B10G10R10: 4, tr.PIX_RGBA8: 4}[pixfmt]


def _launch(kind, kernel, w, h, cus, pixfmt):
    """two calls on the same inputs -> the frame's bytes; asserts the guards and the repeat"""
    depth = tr.depth_of(pixfmt)
    c = tr.cached(kind, w, h, depth)
    n = _frame_bytes(w, h, pixfmt)
    before = ((np.arange(n + 2 * tr.GUARD, dtype=np.int64) * 37 + 11) & 0xff).astype(np.uint8)
    args = (kernel, pixfmt, w, h, _trunk(kind, w, h, depth, kernel, c), c["wgt"], c["b"], c["F"], c["M"], c["img0"], c["img1"], before)
    got = amd.op_tail(*args, cus=cus)
    assert got.size == before.size
    assert np.array_equal(got[:tr.GUARD], before[:tr.GUARD]), "the launch wrote in front of the frame"
    assert np.array_equal(got[-tr.GUARD:], before[-tr.GUARD:]), "the launch wrote behind the frame"
    again = amd.op_tail(*args, cus=cus)
    assert np.array_equal(again, got), "two calls on the same inputs differ in %d bytes" % int((again != got).sum())
    return c, got[tr.GUARD:-tr.GUARD]


def _hold(kind, kernel, w, h, cus, pixfmt):
    c, frame = _launch(kind, kernel, w, h, cus, pixfmt)
    depth, n = tr.depth_of(pixfmt), tr.channels_of(pixfmt)
    got, well_formed = tr.unpack_frame(frame, w, h, pixfmt)
    assert well_formed, "alpha bits of an A2B10G10R10 pixel are not 3"
    ref = c["ref"]
    want, val = ref["code"][..., :n], ref["val"][..., :n]
    lo, hi = tr.allowed_range(ref, c["tau"], depth)
    lo, hi = lo[..., :n], hi[..., :n]
    differ = got != want
    # how much of tau the kernel uses: the distance of the reference value from the boundary it crossed, over tau
    use = float((np.abs(val - np.rint(val)) / c["tau"][..., None])[differ].max()) if differ.any() else 0.0
    print("tail_parity %s %s %s %dx%d cus %d: %d of %d codes differ from the reference, %d outside the boundary set (%d codes in it), largest |v - boundary| / tau = %.4f" % (
        kind, _KERNEL[kernel], _FMT[pixfmt], w, h, cus, int(differ.sum()), differ.size, int((differ & ~c["boundary"][..., :n]).sum()), int(c["boundary"][..., :n].sum()), use))
    bad = (got < lo) | (got > hi) | (np.abs(got - want) > 1)
    if bad.any():
        y, x, ch = np.argwhere(bad)[0]
        raise AssertionError("%d of %d codes are not the reference's where they must be (%d of them differ by more than one); first (y, x, channel) = (%d, %d, %d): got %d, "
                             "reference %d from %.6f, tau %.4f" % (int(bad.sum()), bad.size, int((np.abs(got - want) > 1).sum()), y, x, ch, got[y, x, ch], want[y, x, ch],
                                                                  val[y, x, ch], c["tau"][y, x]))
    return frame


# ---- planted: the lo planes decide the frame ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixfmt", tr.FORMATS, ids=lambda p: _FMT[p])
@pytest.mark.parametrize("case", tr.CASES, ids=_ids)
def test_planted_lo_planes_decide_the_frame(case, pixfmt):
    kernel, w, h, cus = case
    frame = _hold("planted", kernel, w, h, cus, pixfmt)
    if cus == 0:
        _FRAMES.setdefault((w, h, pixfmt), {})[kernel] = frame


def test_planted_frames_of_the_four_kernels():
    """The deltas are exact, so the four kernels differ in nothing but the order of the fp32 tail: whether they return the same bytes is printed for the record
    (profiles/tail_parity/README.md); what is asserted is the rule above, per kernel."""
    for w, h in tr.TILE_SHAPES:
        for pixfmt in tr.FORMATS:
            frames = _FRAMES.get((w, h, pixfmt), {})
            for kernel in (tr.TAIL_RS, tr.TAIL_HEAD_S16, tr.TAIL_HEAD_F32, tr.TAIL_UNFUSED):
                if kernel not in frames:
                    frames[kernel] = _launch("planted", kernel, w, h, 0, pixfmt)[1]
            base = frames[tr.TAIL_UNFUSED]
            print("tail_parity same bytes %dx%d %s: %s" % (w, h, _FMT[pixfmt], ", ".join(
                "%s %s" % (_KERNEL[k], "same" if np.array_equal(frames[k], base) else "%d bytes differ" % int((frames[k] != base).sum())) for k in sorted(frames))))
            assert all(f.size == base.size for f in frames.values())


# ---- dense: the hi path -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixfmt", [tr.PIX_RGB8, tr.PIX_A2B10G10R10], ids=lambda p: _FMT[p])
@pytest.mark.parametrize("case", tr.DENSE_CASES, ids=_ids)
def test_dense_gaussian_trunk(case, pixfmt):
    kernel, w, h, cus = case
    _hold("dense", kernel, w, h, cus, pixfmt)


# ---- far: the clamps ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixfmt", tr.FORMATS, ids=lambda p: _FMT[p])
@pytest.mark.parametrize("case", tr.FAR_CASES, ids=_ids)
def test_far_flows_leave_the_frame(case, pixfmt):
    kernel, w, h, cus = case
    _hold("far", kernel, w, h, cus, pixfmt)


# ---- refusals, by return code -----------------------------------------------------------------------------------------------------------------------------------
def _raw_call(kernel, pixfmt, weight=None, w=32, h=32):
    c = tr.cached("planted", 32, 32, 8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    trunk = s16_ref.pack(c["x"], 8, 8)
    wgt = np.ascontiguousarray(c["wgt"] if weight is None else weight, np.float32)
    out = np.full(2 * tr.GUARD + 32 * 32 * 6, 0x5a, np.uint8)
    keep = (trunk, wgt, out)
    rc = amd.testlib().rife_hip_op_tail(0, kernel, pixfmt, w, h, p(trunk), p(wgt), p(c["b"]), p(c["F"]), p(c["M"]), p(c["img0"]), p(c["img1"]), 0, p(out))
    assert np.all(keep[2] == 0x5a) or rc == 0, "a refused call wrote into the output buffer"
    return rc


def test_refusals():
    assert _raw_call(tr.TAIL_RS, tr.PIX_RGB8) == 0                      # the same call goes through when nothing is wrong with it
    w = tr.cached("planted", 32, 32, 8)["wgt"].copy()
    w[3, 5, 1, 2] = np.float32(1.0 + 2.0 ** -12)                         # not an fp16 value
    for kernel in (tr.TAIL_RS, tr.TAIL_HEAD_S16, tr.TAIL_HEAD_F32, tr.TAIL_UNFUSED):
        assert _raw_call(kernel, tr.PIX_RGB8, weight=w) == -amd.EINVAL
        for pixfmt in (3, 5, amd.PIX_NV12, amd.PIX_RGBP8, -1):
            assert _raw_call(kernel, pixfmt) == -amd.EINVAL
    for kernel in (4, -1):
        assert _raw_call(kernel, tr.PIX_RGB8) == -amd.EINVAL
    assert _raw_call(tr.TAIL_RS, tr.PIX_RGB8, w=0) == -amd.EINVAL
    assert _raw_call(tr.TAIL_RS, tr.PIX_RGB8, w=1 << 14, h=1 << 13) == -amd.EINVAL      # 2^27 pixels: refused before anything is read or uploaded
    L = amd.testlib()
    assert L.rife_hip_op_tail(0, 0, 0, 32, 32, None, None, None, None, None, None, None, 0, None) == -amd.EINVAL
    assert b"op_tail" in L.rife_hip_last_error()
