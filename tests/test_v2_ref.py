"""tests/v2_ref.py pinned to the CPU oracle, without a GPU.

tests/test_gpu_v2_ops.py holds the rife-v2.x / v3.x schedule's kernels to the numpy restatements of v2_ref BIT FOR BIT.  Here every restatement is held bit for bit to
the oracle's graph: OracleRIFE.net_extract with blobs injected - the upsampled head outputs of flownet.param bound to a chosen field and zeros, the Deconvolution tops
bound to chosen head outputs, ContextNet features and FusionNet's sigmoid head bound to noise - so that the graph's own Interp / BinaryOp / rife.Warp / Concat / Crop
layers compute what the restatement computes, in milliseconds.  Blob names come from the STRUCTURE of the .param files (v2_ref.Param), as in tests/test_gpu_gather.py.
The float frames stand for both image forms: the oracle in UHD mode feeds the same graphs Interp(0.5) of the padded frame.

The last test is the condition on the injected fields: the smooth field keeps between a quarter and nine tenths of the sampling positions inside the frame at every
size and scale the GPU tests use, so none of them can pass by sampling only in-frame or only clamped pixels."""
import os

import numpy as np
import pytest

import v2_ref as R
from oracle import pyoracle

SIZES = [(32, 32), (96, 64)]                          # padded frames: one flow cell row at the coarsest scale, and a rectangle
GPU_SIZES = [(32, 32), (96, 64), (160, 96), (288, 32)]


def chw(x):
    return np.ascontiguousarray(np.moveaxis(np.asarray(x, np.float32), -1, 0))


def hwc(x):
    return np.ascontiguousarray(np.moveaxis(x, 0, -1))


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d of %d floats differ, max %g" % (what, int((got != want).sum()), want.size, float(np.abs(got - want).max()))


@pytest.fixture(scope="module")
def nets(modeldirs):
    out = {}
    for fam in ("rife-v2.3", "rife-v3.1"):
        d = modeldirs[fam]
        o = pyoracle.OracleRIFE(rife_v2=True, num_threads=2); o.set_gpu_crop(1); o.load(d)
        out[fam] = (o, {n: R.Param(os.path.join(d, n + ".param")) for n in ("flownet", "contextnet", "fusionnet")})
    return out


def float_frames(wp, hp, seed, f4):
    """(img0, img1) for v2_ref and the same as 3 x hp x wp oracle inputs.  f4: float frames that are no multiples of 1 / 255 (the ImgF4 form)."""
    a, b = R.padded_frames(wp - 3, hp - 5, seed)
    if f4:
        rng = np.random.default_rng(seed)
        a, b = [np.concatenate([rng.random((hp, wp, 3), dtype=np.float32), np.zeros((hp, wp, 1), np.float32)], axis=-1) for _ in range(2)]
    return a, b, chw(R.unpack_rgb(a)), chw(R.unpack_rgb(b))


@pytest.mark.parametrize("f4", [False, True])
@pytest.mark.parametrize("kind", R.FIELDS)
@pytest.mark.parametrize("wp,hp", SIZES)
def test_block_inputs_v23(nets, wp, hp, kind, f4):
    """Interp x2, x 2, two rife.Warp, Concat, Interp 1/S of flownet.param (blocks 1 - 3) and the Interp 1/8 of block 0 against assemble10 / assemble0."""
    o, P = nets["rife-v2.3"]
    fl = P["flownet"]
    heads = fl.head_tops()
    assert len(heads) == 4 and len(fl.conv_inputs(10)) == 3 and len(fl.conv_inputs(6)) == 1
    a, b, x0, x1 = float_frames(wp, hp, 3, f4)
    acc = R.injected_acc(wp, hp, kind, 1)
    z = np.zeros_like(chw(acc))
    bind = {"input0": x0, "input1": x1, heads[0]: chw(acc), heads[1]: z, heads[2]: z}
    for blob, S in zip(fl.conv_inputs(10), (4, 2, 1)):
        same(hwc(o.net_extract(0, bind, blob, 16 * wp * hp)), R.assemble10(a, b, acc, S), "block input at 1/%d" % S)
        pre = fl.producer(blob)
        if pre[0] == "Interp":                            # the 10 channels before Interp 1/S: the full-resolution block input
            same(hwc(o.net_extract(0, bind, pre[2][0], 16 * wp * hp)), R.block_input_full(a, b, acc), "block input before Interp 1/%d" % S)
    same(hwc(o.net_extract(0, bind, fl.conv_inputs(6)[0], 16 * wp * hp)), R.assemble0(a, b, 8)[..., :6], "block 0 input")
    assert not R.assemble(a, b, acc, 2)[..., 10:].any() and not R.assemble0(a, b, 8)[..., 6:].any()


@pytest.mark.parametrize("f4", [False, True])
@pytest.mark.parametrize("kind", R.FIELDS)
@pytest.mark.parametrize("wp,hp", SIZES)
def test_block_inputs_v31(nets, wp, hp, kind, f4):
    """rife-v3.1: block 0 at 1/4, block 1 at 1/2 with the flow channels x 1/2 (FSCALE), block 2 at full resolution (x 1.0)."""
    o, P = nets["rife-v3.1"]
    fl = P["flownet"]
    heads = fl.head_tops()
    assert len(heads) == 3 and len(fl.conv_inputs(10)) == 2 and len(fl.conv_inputs(6)) == 1
    a, b, x0, x1 = float_frames(wp, hp, 4, f4)
    acc = R.injected_acc(wp, hp, kind, 2)
    bind = {"input0": x0, "input1": x1, heads[0]: chw(acc), heads[1]: np.zeros_like(chw(acc))}
    same(hwc(o.net_extract(0, bind, fl.conv_inputs(10)[0], 16 * wp * hp)), R.assemble10(a, b, acc, 2, fscale=True), "block 1 input")
    same(hwc(o.net_extract(0, bind, fl.conv_inputs(10)[1], 16 * wp * hp)), R.assemble10(a, b, acc, 1), "block 2 input")
    same(hwc(o.net_extract(0, bind, fl.conv_inputs(6)[0], 16 * wp * hp)), R.assemble0(a, b, 4)[..., :6], "block 0 input")


@pytest.mark.parametrize("wp,hp", SIZES)
def test_flow_accum_chain(nets, wp, hp):
    """The Deconvolution tops bound to noise: blob `flow` is the chain of k2_flow_accum launches of run_v2_ifnet, for both families."""
    rng = np.random.default_rng(wp)
    hh, wh = hp // 2, wp // 2
    for fam, scales, mul in (("rife-v2.3", (8, 4, 2, 1), False), ("rife-v3.1", (4, 2, 1), True)):
        o, P = nets[fam]
        tops = [l[3][0] for l in P["flownet"].of_type("Deconvolution")]
        assert len(tops) == len(scales)
        D = [rng.normal(0, 3, (hh // s, wh // s, 4)).astype(np.float32) for s in scales]
        bind = {t: chw(d) for t, d in zip(tops, D)}
        acc = None
        for k, s in enumerate(scales):
            acc = R.flow_accum(D[k], acc, s, first=k == 0, mul=mul)
        same(hwc(o.net_extract(0, bind, "flow", 4 * wp * hp)), acc, fam + " flow")


@pytest.mark.parametrize("kind", R.FIELDS)
@pytest.mark.parametrize("wp,hp", SIZES)
def test_context_pyramid_and_warps(nets, wp, hp, kind):
    """contextnet.param with the four feature blobs bound to noise and flow.0 to two channels of acc: f1..f4 are the warps of the pyramid's levels."""
    o, P = nets["rife-v2.3"]
    cx = P["contextnet"]
    warps = cx.of_type("rife.Warp")
    assert [l[3][0] for l in warps] == ["f1", "f2", "f3", "f4"]
    rng = np.random.default_rng(hp)
    acc = R.injected_acc(wp, hp, kind, 3)
    for c0 in (0, 2):
        pyr = R.flow_pyramid(acc, c0)
        feats = [rng.normal(0, 1, (hp >> (l + 2), wp >> (l + 2), 32 << l)).astype(np.float32) for l in range(4)]
        bind = {"flow.0": chw(acc[..., c0:c0 + 2])}
        for l, wl in enumerate(warps):
            src = cx.producer(wl[2][0])
            bind[src[2][0] if src[0] == "Split" else wl[2][0]] = chw(feats[l])
        for l, wl in enumerate(warps):
            same(hwc(o.net_extract(1, bind, wl[2][1], wp * hp)), pyr[l], "flow level %d" % l)
            same(hwc(o.net_extract(1, bind, wl[3][0], 64 * wp * hp)), R.warp_nhwc(feats[l], pyr[l]), "f%d" % (l + 1))


@pytest.mark.parametrize("kind", R.FIELDS)
@pytest.mark.parametrize("wp,hp", SIZES)
def test_fusion_tail(nets, wp, hp, kind):
    """fusionnet.param with the sigmoid head bound to noise: `output` is k2_final_float, its first convolution's input is the block input at scale 1, and the
    quantised frame is the reference's postproc of it."""
    o, P = nets["rife-v2.3"]
    fu = P["fusionnet"]
    sig = [l for l in fu.of_type("Deconvolution") if l[4].get("9") == "4"]
    assert len(sig) == 1 and len(fu.conv_inputs(10)) == 1
    a, b, x0, x1 = float_frames(wp, hp, 5, False)
    acc = R.injected_acc(wp, hp, kind, 4)
    head = np.random.default_rng(wp + hp).random((hp, wp, 4), dtype=np.float32)
    bind = {"img0": x0, "img1": x1, "flow": chw(acc), sig[0][3][0]: chw(head)}
    want = R.final_float(a, b, acc, head)
    same(hwc(o.net_extract(2, bind, "output", 4 * wp * hp)), want[..., :3], "output")
    assert not want[..., 3].any()
    same(hwc(o.net_extract(2, bind, fu.conv_inputs(10)[0], 16 * wp * hp)), R.assemble10(a, b, acc, 1), "FusionNet input")
    w, h = wp - 3, hp - 5
    q = R.final_u8(a, b, acc, head, w, h)
    assert q.shape == (h, w, 3) and np.array_equal(q, np.clip((want[:h, :w, :3] * 255.0 + 0.5).astype(np.int32), 0, 255))      # rife.cpp:1167-1182


@pytest.mark.parametrize("wp,hp", SIZES)
def test_uhd_resamplers(wp, hp):
    a, _ = R.padded_frames(wp - 1, hp - 2, 6)
    same(R.image_half(a)[..., :3], hwc(pyoracle.interp(chw(R.unpack_rgb(a)), 0.5, 0.5)), "image_half")
    assert not R.image_half(a)[..., 3].any()
    acc = R.injected_acc(wp, hp, "smooth", 5)
    same(R.flow_up2_double(acc), hwc(pyoracle.interp(chw(acc), 2.0, 2.0)) * np.float32(2), "flow_up2_double")


def test_conv3x3_s2_f64_is_the_oracles_convolution():
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1, (13, 18, 10)).astype(np.float32)
    wt = rng.normal(0, 0.2, (12, 10, 3, 3)).astype(np.float32); bias = rng.normal(0, 0.1, 12).astype(np.float32)
    want = hwc(pyoracle.conv2d(chw(x), wt, bias, stride=2))
    got = R.conv3x3_s2_f64(x, wt, bias, np.ones(12))
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-5
    slope = rng.uniform(-0.5, 0.5, 12)
    assert np.allclose(R.conv3x3_s2_f64(x, wt, bias, slope), np.where(got < 0, got * slope, got))


@pytest.mark.parametrize("wp,hp", GPU_SIZES)
def test_injected_fields_sample_inside_and_outside(wp, hp):
    """The condition tests/test_gpu_v2_ops.py rests on, on the reference alone: at every size and scale the smooth field keeps between a quarter and nine tenths of
    the sampling positions inside the frame; the zero field keeps all but the last row and column; the clamping field keeps none; the shift lands on pixels."""
    for seed in range(8):
        for kind in R.SMOOTH:
            sh = R.inside_shares(R.injected_acc(wp, hp, kind, seed))
            assert "ctx0_l0" in sh and all(0.25 <= v <= 0.9 for v in sh.values()), (kind, seed, sh)
    z = R.inside_shares(R.injected_acc(wp, hp, "zero"))
    assert all(v > 0.75 for v in z.values())              # (7 / 8)^2 on the 8 x 8 level of a 32 x 32 frame
    assert all(v == 0.0 for v in R.inside_shares(R.injected_acc(wp, hp, "clamp")).values())
    F = R.flow_up2x2(R.injected_acc(wp, hp, "shift"))
    assert np.array_equal(F, np.round(F)) and np.abs(F).min() >= 2
