"""The rife-v2.x / v3.x schedule's own kernels, ONE LAUNCH each, on inputs built to hurt (include/rife_hip_test.h "rife-v2 / v3 kernels alone").

tests/test_gpu_v2.py and test_gpu_v3.py compare the final u8 frame with the oracle on smooth frames and the synthetic weights, whose flow stays under one pixel:
warp_taps never clamps there, the edge coefficients of flow_up2x2 hardly matter, the halo of stem2_fused_kernel is filled from the pixel under it and k2_final blends
two nearly unwarped frames - a wrong tap index, clamp bound, record swizzle or blockIdx.z table entry costs a fraction of a code.  Here every kernel runs alone on
INJECTED running flows (tests/v2_ref.py: zero, an integer shift, a smooth field that takes a quarter to nine tenths of the samples out of the frame, a field that
clamps everywhere; tests/test_v2_ref.py asserts those shares on the reference alone) and on noise frames:
  * elementwise_v2.h (k2_assemble0, k2_assemble, k2_flow_accum, k2_flow_half, k2_warp_nhwc, k2_warp_nhwc_batch, k2_final, k2_final_float, k2_image_half,
    k2_flow_up2_double) BIT FOR BIT against the float32 restatements of v2_ref, which test_v2_ref.py pins bit for bit to the oracle's graph; every output buffer goes in
    full of sentinels and comes back whole;
  * the seven instantiations of stem2_fused_kernel: (a) with one-hot weights the kernel returns hi + lo of every block-input channel at every tap - 2^-22 relative,
    the bar of tests/test_gpu_gather.py; (b) on random fp16 weights, bias and PReLU slopes the fused launch is the unfused pair (k2_assemble + conv_h2s2_kernel) byte
    for byte, and the R64 form is the plain form byte for byte; (c) for 32, 48, 80 and 96 output channels;
  * conv_img_s2_kernel: two tensors per launch = two launches, a grid under a CU budget = the full grid, values against the float64 convolution;
  * launch_conv with a second tensor pair and with a second destination view: byte for byte the one-tensor launch, foreign channel slices untouched.
Sizes: 32 x 32 (one partial tile, under 8 workgroups for the XCD remap), 96 x 64 (a second, partial tile across), 160 x 96 (three tiles across, 36 workgroups,
n & 7 != 0), 288 x 32 (wide and flat); k2_final on unpadded 1 x 1, 33 x 31, 100 x 60."""
import functools
import importlib

import numpy as np
import pytest

import v2_ref as R

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()      # librife_hip_test.so (include/rife_hip_test.h)

SIZES = [(32, 32), (96, 64), (160, 96), (288, 32)]
SENT = np.float32(-12345.5)


def sent(*shape):
    return np.full(shape, SENT, np.float32)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d of %d floats differ, max %g, first at %s" % (
        what, int((got != want).sum()), want.size, float(np.abs(got - want).max()), np.argwhere(got != want)[0])


@functools.lru_cache(maxsize=None)
def frames(wp, hp, f4):
    """Noise frames of (wp - 3) x (hp - 5) padded to wp x hp - resident dwords, or (f4) float4 frames that are no multiples of 1 / 255."""
    if not f4:
        return R.padded_frames(wp - 3, hp - 5, wp + hp)
    rng = np.random.default_rng(wp * hp)
    return tuple(np.concatenate([rng.random((hp, wp, 3), dtype=np.float32), np.zeros((hp, wp, 1), np.float32)], axis=-1) for _ in range(2))


@functools.lru_cache(maxsize=None)
def acc_of(wp, hp, kind):
    return R.injected_acc(wp, hp, kind, wp)


@functools.lru_cache(maxsize=None)
def block_input(wp, hp, kind, f4, S, fscale):
    a, b = frames(wp, hp, f4)
    return R.assemble10(a, b, acc_of(wp, hp, kind), S, fscale)


def fp16_layer(cout, cin, k, seed, scale=0.25):
    rng = np.random.default_rng(seed)
    wt = rng.normal(0, scale, (cout, cin, k, k)).astype(np.float16).astype(np.float32)
    bias = rng.normal(0, 0.3, cout).astype(np.float32)
    slope = rng.uniform(-0.5, 1.2, cout).astype(np.float32)      # PReLU slopes, about a third of them negative
    return wt, bias, slope


# ---- elementwise_v2.h, bit for bit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f4", [False, True], ids=["u8", "f4"])
@pytest.mark.parametrize("wp,hp", SIZES)
def test_assemble_bit_exact(wp, hp, f4):
    """k2_assemble0<8 | 4, IMG> and k2_assemble<4 | 2 | 1, IMG, FSCALE>: every launch of run_v2_ifnet / run_v2_synth, pad channels zero, for both image forms."""
    a, b = frames(wp, hp, f4)
    for S in (8, 4):
        same(amd.op_v2_assemble(S, a, b, None, sent(hp // S, wp // S, 8), first=True), R.assemble0(a, b, S), "k2_assemble0<%d>" % S)
    for kind in R.FIELDS:
        acc = acc_of(wp, hp, kind)
        for S, fs in ((4, False), (2, False), (2, True), (1, False)):
            want = np.concatenate([block_input(wp, hp, kind, f4, S, fs), np.zeros((hp // S, wp // S, 6), np.float32)], axis=-1)
            same(amd.op_v2_assemble(S, a, b, acc, sent(hp // S, wp // S, 16), fscale=fs), want, "k2_assemble<%d, %s> on the %s field" % (S, fs, kind))


@pytest.mark.parametrize("wp,hp", SIZES)
def test_flow_accum_bit_exact(wp, hp):
    """k2_flow_accum<S, FIRST, MUL>: the seven launches of run_v2_ifnet (six instantiations); acc goes in and comes out."""
    rng = np.random.default_rng(hp)
    hh, wh = hp // 2, wp // 2
    acc = rng.normal(0, 20, (hh, wh, 4)).astype(np.float32)
    for S, first, mul in ((8, True, False), (4, False, False), (2, False, False), (1, False, False), (4, True, True), (2, False, True)):
        D = rng.normal(0, 5, (hh // S, wh // S, 4)).astype(np.float32)
        same(amd.op_v2_flow_accum(S, D, sent(hh, wh, 4) if first else acc, first=first, mul=mul), R.flow_accum(D, acc, S, first, mul), "k2_flow_accum<%d, %s, %s>" % (S, first, mul))


@pytest.mark.parametrize("batch", [False, True], ids=["launches", "batch"])
@pytest.mark.parametrize("wp,hp", SIZES)
def test_ctx_warps_bit_exact(wp, hp, batch):
    """Both flow pyramids and the four concat buffers, in both forms: the warped levels in their slices, every other channel still the sentinel."""
    rng = np.random.default_rng(wp)
    feats = [rng.normal(0, 1, (hp >> (l + 2), wp >> (l + 2), 32 << l)).astype(np.float32) for l in (0, 1, 2, 3, 0, 1, 2, 3)]
    fl = [sent(hp >> (l + 2), wp >> (l + 2), 2) for l in (0, 1, 2, 3, 0, 1, 2, 3)]
    cat = [sent(hp >> (l + 2), wp >> (l + 2), 128 << l) for l in range(4)]
    for kind in R.FIELDS:
        acc = acc_of(wp, hp, kind)
        want_fl, want_cat = R.ctx_concat(acc, feats, cat)
        got_fl, got_cat = amd.op_v2_ctx_warps(acc, feats, fl, cat, batch=batch)
        for z in range(8):
            same(got_fl[z], want_fl[z], "flow level %d of frame %d (%s)" % (z & 3, z >> 2, kind))
        for l in range(4):
            same(got_cat[l], want_cat[l], "B%d (%s)" % (l + 1, kind))
            assert (got_cat[l][..., :64 << l] == SENT).all()


@pytest.mark.parametrize("w,h", [(1, 1), (33, 31), (100, 60)] + SIZES)
def test_final_bit_exact(w, h):
    """k2_final (u8 frame of w x h) and k2_final_float (float4 frame of wp x hp) with guards around the frame; no rounding-boundary exclusion."""
    wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32
    a, b = R.padded_frames(w, h, w * h)
    head = np.random.default_rng(w).random((hp, wp, 4), dtype=np.float32)
    G = amd.TAIL_GUARD
    for kind in R.FIELDS:
        acc = acc_of(wp, hp, kind)
        buf = amd.op_v2_final(a, b, w, h, acc, head, np.full(2 * G + w * h * 3, 0xA5, np.uint8))
        assert (buf[:G] == 0xA5).all() and (buf[-G:] == 0xA5).all(), "k2_final wrote outside the frame"
        got, want = buf[G:-G].reshape(h, w, 3), R.final_u8(a, b, acc, head, w, h)
        assert np.array_equal(got, want), "k2_final on the %s field: %d of %d bytes differ" % (kind, int((got != want).sum()), want.size)
        buf = amd.op_v2_final(a, b, w, h, acc, head, np.full(2 * G + wp * hp * 16, 0xA5, np.uint8), float_form=True)
        assert (buf[:G] == 0xA5).all() and (buf[-G:] == 0xA5).all(), "k2_final_float wrote outside the frame"
        same(buf[G:-G].view(np.float32).reshape(hp, wp, 4), R.final_float(a, b, acc, head), "k2_final_float on the %s field" % kind)


@pytest.mark.parametrize("wp,hp", SIZES)
def test_uhd_resamplers_bit_exact(wp, hp):
    a, _ = frames(wp, hp, False)
    same(amd.op_v2_uhd(a, sent(hp // 2, wp // 2, 4)), R.image_half(a), "k2_image_half")
    for kind in ("smooth", "clamp"):
        acc = acc_of(wp, hp, kind)
        same(amd.op_v2_uhd(acc, sent(hp, wp, 4)), R.flow_up2_double(acc), "k2_flow_up2_double")


# ---- stem2_fused_kernel ------------------------------------------------------------------------------------------------------------------------------------
# (S, f4, fscale, route): the seven instantiations <S, IMG, FSCALE, R64> run_v2_ifnet / run_v2_synth reach; the R64 form is the product's pick at scale 1 on u8
# frames for up to 64 output channels
STEMS = [(1, False, False, amd.V2_STEM_PRODUCT), (1, False, False, amd.V2_STEM_NO_R64), (2, False, False, amd.V2_STEM_PRODUCT), (2, False, True, amd.V2_STEM_PRODUCT),
         (1, True, False, amd.V2_STEM_PRODUCT), (2, True, False, amd.V2_STEM_PRODUCT), (2, True, True, amd.V2_STEM_PRODUCT)]
STEM_IDS = ["s1_u8_r64", "s1_u8", "s2_u8", "s2_u8_fscale", "s1_f4", "s2_f4", "s2_f4_fscale"]


@pytest.mark.parametrize("wp,hp", SIZES)
@pytest.mark.parametrize("S,f4,fscale,route", STEMS, ids=STEM_IDS)
def test_stem_one_hot_reads_back_the_block_input(S, f4, fscale, route, wp, hp):
    """(a) output channel j = input channel c at tap (dy, dx), for all 90 (c, tap) in two launches of 48 channels: the block input through the halo tile, its zero
    padding, the hi / lo split, the record swizzle and the matrix pipe - hi + lo of a value is the value to 2^-22 relative (f16-subnormal floor 1.2e-7)."""
    a, b = frames(wp, hp, f4)
    Ho, Wo = hp // S // 2, wp // S // 2
    combos = [(c, t) for t in range(9) for c in range(10)]
    for kind in R.FIELDS:
        X = block_input(wp, hp, kind, f4, S, fscale)
        Xp = np.zeros((X.shape[0] + 2, X.shape[1] + 2, 10), np.float32)
        Xp[1:-1, 1:-1] = X
        for g in range(0, 90, 48):
            wt = np.zeros((48, 10, 3, 3), np.float32)
            want = np.zeros((Ho, Wo, 48), np.float32)
            for j, (c, t) in enumerate(combos[g:g + 48]):
                wt[j, c, t // 3, t % 3] = 1.0
                want[..., j] = Xp[t // 3:t // 3 + 2 * Ho:2, t % 3:t % 3 + 2 * Wo:2, c]
            got = amd.op_v2_stem(route, S, a, b, acc_of(wp, hp, kind), wt, np.zeros(48, np.float32), np.ones(48, np.float32), sent(Ho, Wo, 48), fscale=fscale)
            err = np.abs(got - want) - (3e-7 * np.abs(want) + 1.2e-7)
            assert err.max() <= 0, "%s field, channels %d..: worst excess %g at %s (got %g, want %g)" % (
                kind, g, float(err.max()), np.unravel_index(np.argmax(err), err.shape), got.flat[np.argmax(err)], want.flat[np.argmax(err)])


@pytest.mark.parametrize("wp,hp", SIZES)
@pytest.mark.parametrize("S,f4,fscale,route", STEMS, ids=STEM_IDS)
def test_stem_fused_is_the_unfused_pair(S, f4, fscale, route, wp, hp):
    """(b), (c): random fp16 weights, bias and slopes, 32 / 48 / 80 / 96 output channels (one, two, three subtiles; 80 leaves half a subtile).  The fused launch equals
    k2_assemble + conv_h2s2_kernel byte for byte ("the result is the unfused path's", stem_fused_v2.h), the R64 form equals the plain form, and both lie within the
    stride-2 split-f16 tolerance of tests/test_gpu_kernels.py of the float64 convolution of the block input."""
    a, b = frames(wp, hp, f4)
    Ho, Wo = hp // S // 2, wp // S // 2
    for k, (cout, kind) in enumerate(zip((32, 48, 80, 96), ("smooth", "clamp", "smooth", "shift"))):
        acc = acc_of(wp, hp, kind)
        wt, bias, slope = fp16_layer(cout, 10, 3, 10 * wp + cout)
        ld = cout + (16 if cout == 80 else 0)                 # the schedule passes out_ld = cout; one wider view shows the channels past Cout stay untouched
        fused = amd.op_v2_stem(route, S, a, b, acc, wt, bias, slope, sent(Ho, Wo, ld), fscale=fscale)
        unfused = amd.op_v2_stem(amd.V2_STEM_UNFUSED, S, a, b, acc, wt, bias, slope, sent(Ho, Wo, ld), fscale=fscale)
        assert (fused[..., cout:] == SENT).all() and (unfused[..., cout:] == SENT).all()
        same(fused, unfused, "fused against unfused, %d channels, %s field" % (cout, kind))
        if route == amd.V2_STEM_NO_R64:
            same(amd.op_v2_stem(amd.V2_STEM_PRODUCT, S, a, b, acc, wt, bias, slope, sent(Ho, Wo, ld), fscale=fscale), fused, "R64 against plain, %d channels" % cout)
        want = R.conv3x3_s2_f64(block_input(wp, hp, kind, f4, S, fscale), wt, bias, slope)
        assert np.abs(fused[..., :cout] - want).max() <= 4e-6 * np.abs(want).max() + 1e-6


# ---- conv_img_s2_kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wp,hp", SIZES)
def test_conv_img(wp, hp):
    a, b = frames(wp, hp, False)
    wt, bias, slope = fp16_layer(32, 3, 3, wp)
    o = sent(hp // 2, wp // 2, 32)
    one_a, one_b = amd.op_v2_conv_img(a, None, wt, bias, slope, o), amd.op_v2_conv_img(b, None, wt, bias, slope, o)
    two_a, two_b = amd.op_v2_conv_img(a, b, wt, bias, slope, o, o)
    same(two_a, one_a, "gridDim.y = 2, first frame"); same(two_b, one_b, "gridDim.y = 2, second frame")
    same(amd.op_v2_conv_img(a, None, wt, bias, slope, o, cus=1), one_a, "grid of 8 workgroups")
    ta, tb = amd.op_v2_conv_img(a, b, wt, bias, slope, o, o, cus=1)
    same(ta, one_a, "grid of 4 x 2 workgroups, first frame"); same(tb, one_b, "grid of 4 x 2 workgroups, second frame")
    for img, got in ((a, one_a), (b, one_b)):
        want = R.conv3x3_s2_f64(R.unpack_rgb(img), wt, bias, slope)
        assert np.abs(got - want).max() <= 4e-6 * np.abs(want).max() + 1e-6      # tests/test_gpu_kernels.py, stride-2 split-f16


# ---- launch_conv: second tensor pair, second destination ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,stride,H,W", [(32, 32, 1, 48, 80), (32, 32, 1, 13, 37), (64, 128, 2, 24, 40), (32, 64, 2, 17, 33), (128, 128, 1, 85, 96)])
def test_conv_two_tensors_are_two_launches(cin, cout, stride, H, W):
    """in1 / out1 (the two ContextNet passes per launch): each tensor equals the one-tensor launch byte for byte, and the channels around the layer's slice stay.
    (The 128 -> 128 layer at a size of more than 64 workgroups: below that the ONE-tensor launch is the split-K form, which sums K in four slices - another order,
    another kernel; measured at 9 x 21: 88 % of the floats differ in the last bits, at most 8.6e-6.)"""
    rng = np.random.default_rng(H * W)
    wt, bias, slope = fp16_layer(cout, cin, 3, cin + cout, 0.1)
    x0, x1 = [rng.normal(0, 1, (H, W, cin)).astype(np.float32) for _ in range(2)]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for ld, off in ((cout, 0), (cout + 32, 16)):
        y = sent(Ho, Wo, ld)
        (s0,), (s1,) = amd.op_conv_pair(wt, bias, slope, x0, y, y_coff=off, stride=stride), amd.op_conv_pair(wt, bias, slope, x1, y, y_coff=off, stride=stride)
        p0, p1 = amd.op_conv_pair(wt, bias, slope, x0, y, x1=x1, y1=y, y_coff=off, stride=stride)
        same(p0, s0, "first tensor"); same(p1, s1, "second tensor")
        assert not np.array_equal(s0, s1) and not (s0[..., off:off + cout] == SENT).any()
        assert (p0[..., :off] == SENT).all() and (p0[..., off + cout:] == SENT).all() and (p1[..., :off] == SENT).all() and (p1[..., off + cout:] == SENT).all()


@pytest.mark.parametrize("c,H,W", [(64, 104, 160), (128, 88, 96), (256, 48, 96), (64, 67, 290), (64, 161, 625)])      # the last: 420 workgroups, the 8-row tiles
def test_conv_second_destination_is_a_copy(c, H, W):
    """y2 (F[3], F[5], F[7] of run_v2_synth: the skip stored into the encoder's AND the decoder's concat buffer) at sizes where the product passes it: both views
    hold the one-destination result byte for byte, and both buffers keep their foreign halves."""
    rng = np.random.default_rng(c)
    wt, bias, slope = fp16_layer(c, c, 3, c, 0.05)
    x = rng.normal(0, 1, (H, W, c)).astype(np.float32)
    (s,) = amd.op_conv_pair(wt, bias, slope, x, sent(H, W, 2 * c))
    d0, d2 = amd.op_conv_pair(wt, bias, slope, x, sent(H, W, 2 * c), y2=sent(H, W, 2 * c), y2_coff=c)
    same(d0, s, "primary destination")
    same(d2[..., c:], s[..., :c], "second destination")
    assert (d0[..., c:] == SENT).all() and (d2[..., :c] == SENT).all() and not (s[..., :c] == SENT).any()


def test_transposed_layer_has_one_form():
    """The 4x4 transposed layers go through launch_conv alone: the one-tensor launch is op_deconv4x4's, a second pair or destination is refused."""
    rng = np.random.default_rng(5)
    wt, bias, slope = fp16_layer(32, 128, 4, 9, 0.05)
    x = rng.normal(0, 1, (10, 19, 128)).astype(np.float32)
    (got,) = amd.op_conv_pair(wt, bias, slope, x, sent(20, 38, 32), stride=2, deconv=True)
    same(got, np.ascontiguousarray(np.moveaxis(amd.op_deconv4x4(np.moveaxis(x, -1, 0), wt, bias, slope), 0, -1)), "deconv")
    with pytest.raises(amd.RifeError, match=r"\(-1\)"):
        amd.op_conv_pair(wt, bias, slope, x, sent(20, 38, 32), x1=x, y1=sent(20, 38, 32), stride=2, deconv=True)


def test_what_the_product_would_not_launch_is_refused():
    a, b = frames(32, 32, False)
    acc = acc_of(32, 32, "zero")
    wt, bias, slope = fp16_layer(48, 10, 3, 1)
    refused = pytest.raises(amd.RifeError, match=r"\(-1\)")      # -RIFE_HIP_EINVAL
    with refused:
        amd.op_v2_assemble(8, a, b, acc, sent(4, 4, 16))                               # k2_assemble<8> does not exist
    with refused:
        amd.op_v2_assemble(4, a, b, acc, sent(8, 8, 16), fscale=True)                  # x 1/S is the v3 block at scale 2
    with refused:
        amd.op_v2_flow_accum(8, np.zeros((2, 2, 4), np.float32), np.zeros((16, 16, 4), np.float32))      # <8, false>
    with refused:
        amd.op_v2_stem(amd.V2_STEM_PRODUCT, 1, a, b, acc, wt + np.float32(1e-4), bias, slope, sent(16, 16, 48))      # not fp16
    with refused:
        w100 = np.zeros((100, 10, 3, 3), np.float32)
        amd.op_v2_stem(amd.V2_STEM_PRODUCT, 1, a, b, acc, w100, np.zeros(100, np.float32), np.ones(100, np.float32), sent(16, 16, 100))      # a fourth subtile
    with refused:
        w64, b64, s64 = fp16_layer(64, 64, 3, 2, 0.05)
        amd.op_conv_pair(w64, b64, s64, np.zeros((8, 8, 64), np.float32), sent(8, 8, 128), y2=sent(8, 8, 128), y2_coff=64)      # split-K size: the product copies the skip
