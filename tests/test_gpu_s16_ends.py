"""The kernels at the two ENDS of an S16 trunk, ONE launch at a time against a float64 reference (GPU box only), and the block stems in composition.

  conv_h2s2_kernel<2, true> / <3, true> (stem-1: writes the first S16 tensor of a block)       through rife_hip_op_stem1_s16
  head_h2_kernel<EPI_DECONV_PS, true> / <EPI_DECONV_PS, false> (the PixelShuffle head)          through rife_hip_op_head_ps
  run_assemble + stem-0 + stem-1, stem0_fused_kernel + conv_h2s2_kernel<NS, true>, stem_rs_kernel through rife_hip_v4_tap what = 7

The entry points use the product's layer upload with the flags rife_hip_load sets and the product's launcher.  tests/s16_ends_ref.py is the reference and the case
table; tests/test_s16_ends_ref.py checks every case's precondition and power on the CPU.

  (1) exact inputs, BYTES.  stem-1: the returned tensor equals pack(reference) byte for byte; it went in with a NaN interior and a zero exterior.  head: planes 0 - 5
      equal float32(reference) bit for bit, planes 6 - 7 still hold the pattern they went in with; S16IN = false returns the bytes of S16IN = true.
  (2) stem-1 with the model's slope 0.2 on the exact inputs: |got - want| <= 2^-21 |want| + 2^-24 (test_gpu_trunk_ops.py::test_model_slope: exact accumulator, then
      the slope multiply, the output split, an f16-subnormal lo).
  (3) dense Gaussian inputs over six decades: err.max() <= 4e-6 |want|.max() + 1e-6, the bar of the fp32-tensor forms of these kernels (tests/test_gpu_kernels.py).
  (4) the block stems of a real pass against the oracle's blob, the top of the block's second stride-2 Convolution (name read from flownet.param).  The bar per block
      is 4 x the largest error measured on the MI355X (profiles/s16_ends/README.md), and never more than a tenth of what a lost lo plane does to the same blob on
      the same inputs (stem-0's output rounded to f16 in the PyTorch graph executor).
  (5) refusals: weights that are not fp16 and C = 32 are -RIFE_HIP_EINVAL."""
import importlib
import os

import numpy as np
import pytest
import torch

import s16_ends_ref as ends
import s16_ref
from oracle import pyoracle
from tools import gen_frames, ncnn_param
from torch_graph import TorchNet

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()      # librife_hip_test.so: parity taps, single-kernel entry points and kernel-selection switches (include/rife_hip_test.h)

_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None


def _assert_s16_bytes(got, want_chw, C, H, W):
    want = s16_ref.pack(want_chw.astype(np.float32), H, W)
    ext = s16_ref.exterior_mask(C, H, W)
    assert not got[ext].any(), "%d exterior bytes are not zero" % np.count_nonzero(got[ext])
    if not np.array_equal(got, want):
        gv, wv = s16_ref.value(got, C, H, W), s16_ref.value(want, C, H, W)
        bad = np.argwhere(~((gv == wv) | (np.isnan(gv) & np.isnan(wv))))
        raise AssertionError("%d of %d interior elements differ in value, %d bytes (NaN = never written: %d); first (c, y, x) = %s got %r want %r" % (
            len(bad), gv.size, int((got != want).sum()), int(np.isnan(gv).sum()), bad[:1].tolist(), gv[tuple(bad[0])] if len(bad) else None,
            wv[tuple(bad[0])] if len(bad) else None))


def _stem1(C, Ht, Wt, c, slope):
    return amd.op_stem1_s16(C, Ht, Wt, c["x"], c["w"], c["b"], slope, s16_ref.poisoned(C, Ht, Wt))


def _flow_before(Ht, Wt):
    """the flow tensor before the launch: planes 0 - 5 NaN (every element must be written), planes 6 - 7 a pattern nobody may touch."""
    t = np.full((8, 4 * Ht, 4 * Wt), np.nan, np.float32)
    t[6:] = (np.arange(2 * 16 * Ht * Wt, dtype=np.float32) * 0.5 - 7.0).reshape(2, 4 * Ht, 4 * Wt)
    return t


def _head(C, Ht, Wt, c, s16):
    before = _flow_before(Ht, Wt)
    got = amd.op_head_ps(C, Ht, Wt, s16_ref.pack(c["x"], Ht, Wt) if s16 else c["x"], c["w"], c["b"], before)
    assert np.array_equal(got[6:].view(np.uint32), before[6:].view(np.uint32)), "the head wrote into planes 6 / 7 of the flow tensor"
    return got[:6]


# ---- (1) exact inputs, bytes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ends.stem1_cases(), ids=_ids)
def test_stem1_exact_inputs_bytes(case):
    C, Ht, Wt = case
    e = ends.cached("stem1_exact", C, Ht, Wt)
    _assert_s16_bytes(_stem1(C, Ht, Wt, e, e["slope"]), e["want"], C, Ht, Wt)


@pytest.mark.parametrize("case", ends.head_cases(), ids=_ids)
def test_head_exact_inputs_bytes(case):
    C, Ht, Wt, s16 = case
    e = ends.cached("head_exact", C, Ht, Wt)
    got, want = _head(C, Ht, Wt, e, s16), e["want"].astype(np.float32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%d of %d elements differ (NaN = never written: %d); first (c, y, x) = %s" % (
        int(bad.sum()), bad.size, int(np.isnan(got).sum()), np.argwhere(bad)[:1].tolist())
    if not s16:
        assert np.array_equal(got.view(np.uint32), _head(C, Ht, Wt, e, 1).view(np.uint32)), "S16IN = false and S16IN = true differ on the same values"


# ---- (2) stem-1, the model's slope --------------------------------------------------------------------------------------------------------------------
_REF = {}


@pytest.mark.parametrize("case", ends.stem1_cases(), ids=_ids)
def test_stem1_model_slope(case):
    C, Ht, Wt = case
    e = ends.cached("stem1_exact", C, Ht, Wt)
    if case not in _REF:
        _REF[case] = ends.stem1_layer(e["x"], e["w"], e["b"], 0.2)
    want = _REF[case]
    raw = _stem1(C, Ht, Wt, e, 0.2)
    assert not raw[s16_ref.exterior_mask(C, Ht, Wt)].any()
    err = np.abs(s16_ref.value(raw, C, Ht, Wt) - want)
    print("s16_ends (2) stem-1 %s max err / bar = %.3f" % (_ids(case), (err / (2.0 ** -21 * np.abs(want) + 2.0 ** -24)).max()))
    assert np.all(err <= 2.0 ** -21 * np.abs(want) + 2.0 ** -24)


# ---- (3) dense Gaussian inputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ends.stem1_cases(), ids=_ids)
def test_stem1_dense_gaussian(case):
    C, Ht, Wt = case
    g = ends.cached("stem1_gauss", C, Ht, Wt)
    raw = _stem1(C, Ht, Wt, g, 0.2)
    assert not raw[s16_ref.exterior_mask(C, Ht, Wt)].any()
    err = np.abs(s16_ref.value(raw, C, Ht, Wt) - g["want"])
    print("s16_ends (3) stem-1 %s err.max / |want|.max = %.3e" % (_ids(case), err.max() / np.abs(g["want"]).max()))
    assert err.max() <= 4e-6 * np.abs(g["want"]).max() + 1e-6      # the fp32-tensor form's bar for the same products (tests/test_gpu_kernels.py)


@pytest.mark.parametrize("case", ends.head_cases(), ids=_ids)
def test_head_dense_gaussian(case):
    C, Ht, Wt, s16 = case
    g = ends.cached("head_gauss", C, Ht, Wt)
    err = np.abs(_head(C, Ht, Wt, g, s16).astype(np.float64) - g["want"])
    print("s16_ends (3) head %s err.max / |want|.max = %.3e" % (_ids(case), err.max() / np.abs(g["want"]).max()))
    assert err.max() <= 4e-6 * np.abs(g["want"]).max() + 1e-6


# ---- (4) the block stems in composition ---------------------------------------------------------------------------------------------------------------
# Largest |got - oracle| / |oracle|.max() measured on the MI355X per block over the cases below (profiles/s16_ends/README.md); the bar is 4 x that.
STEMS_MEASURED = {0: 1.23e-6, 1: 1.10e-6, 2: 1.01e-6, 3: 9.3e-7}      # block 3: the larger of stem_rs_kernel (8.2e-7) and the two-kernel sequence (9.3e-7)
BLOCK_C = (192, 128, 96, 64)
BLOCK_S = (8, 4, 2, 1)
STEM_SIZES = [(64, 64), (160, 96), (100, 60)]


def _stem_blobs(modeldir):
    """per block: (top of the first stride-2 Convolution, top of the second) of flownet.param, in file order."""
    tops = [l["tops"][0] for l in ncnn_param.parse(os.path.join(modeldir, "flownet.param")) if l["type"] == "Convolution" and int(l["params"].get(3, 1)) == 2]
    assert len(tops) == 8, tops
    return [(tops[2 * b], tops[2 * b + 1]) for b in range(4)]


@pytest.fixture(scope="module")
def stems(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    old = os.environ.get("RIFE_HIP_STEM_RS")
    os.environ["RIFE_HIP_STEM_RS"] = "0"                                 # read at create time: block 3 on stem0_fused_kernel + conv_h2s2_kernel<2, true>
    try:
        g2 = amd.RIFE(0, rife_v4=True); g2.load(d)
    finally:
        if old is None: del os.environ["RIFE_HIP_STEM_RS"]
        else: os.environ["RIFE_HIP_STEM_RS"] = old
    o = pyoracle.OracleRIFE(rife_v4=True); o.load(d)
    net = TorchNet(os.path.join(d, "flownet.param"), os.path.join(d, "flownet.bin"))
    return dict(rs=g, tiles=g2, oracle=o, net=net, blobs=_stem_blobs(d))


def _lost_lo_effect(net, a, c, t, inj, blob0, blob1):
    """CPU model of a lost lo plane: the block's stem-1 output with stem-0's output rounded to f16, against the same graph left alone.  max |difference|."""
    h, w, _ = a.shape
    wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32

    def chw(img):
        x = np.zeros((3, hp, wp), np.float32)
        x[:, :h, :w] = (img.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1)
        return torch.from_numpy(x)
    ins = {"in0": chw(a), "in1": chw(c), "in2": torch.full((1, hp, wp), np.float32(t))}
    for k, f in enumerate(inj):
        ins["flow%d" % k] = torch.from_numpy(f)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 8))                               # frames of 160x96 at most: a pool sized for a whole machine only waits for itself
    try:
        s0, s1 = net.run(ins, [blob0, blob1])
        (s1r,) = net.run(dict(ins, **{blob0: s0.to(torch.float16).to(torch.float32)}), [blob1])
    finally:
        torch.set_num_threads(threads)
    return float((s1r - s1).abs().max())


STEM_CASES = [(b, w, h, kind, "rs") for b in range(4) for w, h in STEM_SIZES for kind in ("smooth", "noise")] + \
             [(3, w, h, kind, "tiles") for w, h in STEM_SIZES for kind in ("smooth", "noise")]


@pytest.mark.parametrize("case", STEM_CASES, ids=_ids)
def test_block_stems_match_oracle(stems, case):
    b, w, h, kind, eng = case
    a, c = (gen_frames.smooth_pair if kind == "smooth" else gen_frames.noise_pair)(w, h, 21 + b)
    t = 0.5 if kind == "smooth" else 0.4
    wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32
    rng = np.random.default_rng([b, w, h])
    inj = [(rng.standard_normal((6, hp // s, wp // s)) * 0.3).astype(np.float32) for s in BLOCK_S[:b]]      # a few tenths of a pixel
    C, Ht, Wt = BLOCK_C[b], hp // BLOCK_S[b] // 4, wp // BLOCK_S[b] // 4
    blob0, blob1 = stems["blobs"][b]
    want = stems["oracle"].v4_extract(a, c, t, blob1, flows=inj)
    assert want.shape == (C, Ht, Wt)
    raw = stems[eng].v4_tap(a, c, t, 7, b, inj)
    assert np.array_equal(raw, stems[eng].v4_tap(a, c, t, 7, b, inj)), "two calls on one engine return different bytes"
    assert not raw[s16_ref.exterior_mask(C, Ht, Wt)].any(), "the exterior of the first S16 tensor is not zero"
    err = float(np.abs(s16_ref.value(raw, C, Ht, Wt) - want).max()) / float(np.abs(want).max())
    cap = 0.1 * _lost_lo_effect(stems["net"], a, c, t, inj, blob0, blob1) / float(np.abs(want).max())
    print("s16_ends (4) stems %s err / |oracle|.max = %.3e, cap (lost lo / 10) = %.3e, |oracle|.max = %.3g" % (_ids(case), err, cap, float(np.abs(want).max())))
    assert 4 * STEMS_MEASURED[b] <= cap, "the bar does not fit under a tenth of a lost lo plane"
    assert err <= 4 * STEMS_MEASURED[b]


# ---- (5) refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_weights_that_are_not_fp16_are_einval():
    C, Ht, Wt = 64, 4, 32
    t = np.zeros(s16_ref.geom(C, Ht, Wt)[3], np.uint8)
    w = np.zeros((C, C // 2, 3, 3), np.float32); w[5, 7, 1, 2] = 0.1
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*exactly fp16" % amd.EINVAL):
        amd.op_stem1_s16(C, Ht, Wt, np.zeros((C // 2, 2 * Ht, 2 * Wt), np.float32), w, np.zeros(C, np.float32), 0.2, t)
    wh = np.zeros((24, C, 4, 4), np.float32); wh[5, 7, 1, 2] = 0.1
    for x in (t, np.zeros((C, Ht, Wt), np.float32)):
        with pytest.raises(amd.RifeError, match=r"\(-%d\).*exactly fp16" % amd.EINVAL):
            amd.op_head_ps(C, Ht, Wt, x, wh, np.zeros(24, np.float32), np.zeros((8, 4 * Ht, 4 * Wt), np.float32))


def test_channel_counts_without_an_s16_variant_are_einval():
    C, Ht, Wt = 32, 4, 32
    t = np.zeros(s16_ref.geom(C, Ht, Wt)[3], np.uint8)
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*64, 96, 128 and 192" % amd.EINVAL):
        amd.op_stem1_s16(C, Ht, Wt, np.zeros((C // 2, 2 * Ht, 2 * Wt), np.float32), np.zeros((C, C // 2, 3, 3), np.float32), np.zeros(C, np.float32), 0.2, t)
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*64, 96, 128 or 192" % amd.EINVAL):
        amd.op_head_ps(C, Ht, Wt, t, np.zeros((24, C, 4, 4), np.float32), np.zeros(24, np.float32), np.zeros((8, 4 * Ht, 4 * Wt), np.float32))


def test_tap7_refuses_a_block_that_is_off_the_s16_path(modeldirs, monkeypatch):
    """RIFE_HIP_T64=0 (create time) takes every block off the S16 kernels: there is no first S16 tensor to return, and the tap says so by name."""
    monkeypatch.setenv("RIFE_HIP_T64", "0")
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    a, c = gen_frames.smooth_pair(64, 64, 21)
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*does not run on S16 trunk tensors" % amd.EINVAL):
        g.v4_tap(a, c, 0.5, 7, 0, [])
