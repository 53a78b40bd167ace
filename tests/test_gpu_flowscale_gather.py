"""The gather code and the flow updates of flow scale 2 (include/rife_hip.h rife_hip_set_flow_scale) against the oracle DIRECTLY, on injected flows.

At divisor 2 the product runs kernels and instantiations that exist for this mode alone: k_assemble0_s<16, D>, k_assemble<8 | 4 | 2[, 10]>, stem0_fused_kernel<8, 2>,
<4, 2>, <2, 1> and their D = 10 forms, three plain k_flow_update<16, true> / <8, false> / <4, false> launches, and block 3 on stem0_fused_kernel<2, 1> +
conv_h2s2_kernel instead of stem_rs.  tests/test_gpu_flowscale.py sees them behind whole blocks and with the sub-pixel flows of a synthetic model; here the blobs
flow0..flow{b-1} are INJECTED on both sides, at the mode's sizes (frames padded to 64n, block scales 16, 8, 4, 2), as tests/test_gpu_gather.py does at divisor 1.
Expected values: the oracle on the rewritten graph (tests/flowscale_ref.py), blob names from flowscale_ref.stage_blobs.  The flows are
flowscale_ref.injected_flows_scaled: tests/test_flowscale_host.py holds, for every case used here, that between a quarter and nine tenths of the sampling positions
of each frame lie inside the padded frame and that the largest displacement exceeds a quarter of its shorter side - the warps are seen inside the frame AND at
its clamps.

  a  block input (rife_hip_v4_tap what = 0, b = 0..3: k_assemble0_s<16, D>, k_assemble<8 | 4 | 2, D>), RGB8 and RGB10_U16: BIT FOR BIT
  b  the same tensor through the product's fused stem with one-hot weights (what = 1, b = 1..3): |got - want| <= 3e-7 |want| + 1.2e-7 - hi + lo of a value
     (2^-22 relative) plus the f16 subnormal floor, the bound of tests/test_gpu_gather.py
  c  F and M after the plain updates (what = 4, b = 1..3), every padded pixel: BIT FOR BIT against the oracle's blobs after that update
  d  the block stems in composition (what = 7, b = 0..3) against the top of the block's second stride-2 Convolution, as tests/test_gpu_s16_ends.py (4) does at
     divisor 1: two calls return the same bytes, the exterior is zero, err / |oracle|.max <= 4 x the largest value measured on the MI355X per block
     (profiles/flowscale_gather/README.md), and that bar is at most a tenth of what a lost lo plane does to the same blob
  f  what = 2, 3, 5, 6 are kernels of the scale-1 schedule: EINVAL with a message that says so
(e, k_final_scaled where it can see the frame, is in tests/test_gpu_flowscale.py.)

Sizes (flowscale_ref.GATHER_CASES): each the smallest that still reaches its edge - 1x1 (64x64: flow0 is 4x4, up_coeff's in - 2 edge), 65x64 (one column past 64),
100x60, 130x9, 8x300, 333x241, and 640x360 (640x384: the first size at which the scale-8 stem has two 32-wide tiles across)."""
import importlib
import os

import numpy as np
import pytest
import torch

import deep_ref
import flowscale_ref as fr
import s16_ref
from oracle import pyoracle
from tools import gen_frames
from torch_graph import TorchNet

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()      # librife_hip_test.so: the parity taps (include/rife_hip_test.h)

BLOCK_C = (192, 128, 96, 64)
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None


@pytest.fixture(scope="module")
def fs2(modeldirs, tmp_path_factory):
    d = fr.scaled_modeldir(modeldirs["rife-v4.6"], tmp_path_factory.mktemp("v46_fs2_gather"))
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    g.set_flow_scale(2)
    assert g.flow_scale == 2
    o = pyoracle.OracleRIFE(rife_v4=True); o.load(d)
    with open(os.path.join(d, "flownet.param")) as f:
        sb = fr.stage_blobs(f.read())
    net = TorchNet(os.path.join(d, "flownet.param"), os.path.join(d, "flownet.bin"))
    return dict(g=g, oracle=o, blobs=sb, net=net)


def frames(w, h, seed, depth):
    """noise for odd seeds, smooth for even ones; depth 10: (h, w, 3) uint16 codes 0..1023 (RGB10_U16)."""
    if depth == 8:
        return gen_frames.noise_pair(w, h, seed) if seed % 2 else gen_frames.smooth_pair(w, h, seed)
    if seed % 2:
        rng = np.random.default_rng(1000 + seed)
        return rng.integers(0, 1024, (h, w, 3), dtype=np.uint16), rng.integers(0, 1024, (h, w, 3), dtype=np.uint16)
    return deep_ref.deep_pair(w, h, 50 + seed)


_WANT = {}


def block_input(fs2, w, h, seed, depth, b):
    """(frames, injected blobs, timestep, the oracle's block-input blob): computed once, shared by (a) and (b) (do not modify)."""
    key = (w, h, seed, depth, b)
    if key not in _WANT:
        a, c = frames(w, h, seed, depth)
        inj = fr.injected_flows_scaled(w, h, fr.FLOW_SEED + seed, 3)[:b]
        t = 0.3 + 0.1 * b
        name = fs2["blobs"]["block0_in"] if b == 0 else fs2["blobs"]["block_in"][b - 1]
        _WANT[key] = (a, c, inj, t, fr.extract(fs2["oracle"], a, c, t, depth, name, flows=inj))
    return _WANT[key]


# ---- a. block input, bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("b", [0, 1, 2, 3])
@pytest.mark.parametrize("case", fr.GATHER_CASES, ids=_ids)
def test_block_input_bit_exact(fs2, case, b, depth):
    w, h, seed = case
    a, c, inj, t, want = block_input(fs2, w, h, seed, depth, b)
    wp, hp = fr.padded(w, h)
    s = fr.SCALES[b]
    assert want.shape == ((7 if b == 0 else 12), hp // s, wp // s)
    got = fs2["g"].v4_tap(a, c, t, 0, b, inj)
    assert got.shape == want.shape
    assert np.array_equal(got, want), "block %d input at 1/%d, depth %d: %d of %d floats differ, max %g, first (c, y, x) = %s" % (
        b, s, depth, int((got != want).sum()), want.size, float(np.abs(got - want).max()), np.argwhere(got != want)[:1].tolist())


# ---- b. through the fused stem ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("b", [1, 2, 3])
@pytest.mark.parametrize("case", fr.GATHER_CASES, ids=_ids)
def test_block_input_through_the_fused_stem(fs2, case, b, depth):
    w, h, seed = case
    a, c, inj, t, want = block_input(fs2, w, h, seed, depth, b)
    got = fs2["g"].v4_tap(a, c, t, 1, b, inj)
    assert got.shape == want.shape
    err = np.abs(got - want) - (3e-7 * np.abs(want) + 1.2e-7)       # hi + lo of a value: 2^-22 relative, f16 subnormal floor
    assert err.max() <= 0, "fused stem kernel of block %d (scale %d, depth %d): worst excess %g at %s" % (
        b, fr.SCALES[b], depth, float(err.max()), np.unravel_index(np.argmax(err), err.shape))


# ---- c. F and M after the plain updates -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2, 3])
@pytest.mark.parametrize("case", fr.GATHER_CASES, ids=_ids)
def test_flow_updates_write_the_oracles_F_M(fs2, case, b):
    """k_flow_update<16, true>, then <8, false>, then <4, false>: the kernel restates the Interp and the Eltwise term by term, and at divisor 1 the same code is
    bit-identical to the oracle (tests/test_gpu_gather.py, the b == 3 check)."""
    w, h, seed = case
    wp, hp = fr.padded(w, h)
    a, c = frames(w, h, seed, 8)
    inj = fr.injected_flows_scaled(w, h, fr.FLOW_SEED + seed, 3)[:b]
    wantF = fr.extract(fs2["oracle"], a, c, 0.5, 8, fs2["blobs"]["F"][b - 1], flows=inj)
    wantM = fr.extract(fs2["oracle"], a, c, 0.5, 8, fs2["blobs"]["M"][b - 1], flows=inj)
    assert wantF.shape == (4, hp, wp) and wantM.shape == (1, hp, wp)
    got = fs2["g"].v4_tap(a, c, 0.5, 4, b, inj)
    assert got.shape == (5, hp, wp)
    assert np.array_equal(got[:4], wantF), "F after update %d: %d of %d floats differ, max %g, first (c, y, x) = %s" % (
        b - 1, int((got[:4] != wantF).sum()), wantF.size, float(np.abs(got[:4] - wantF).max()), np.argwhere(got[:4] != wantF)[:1].tolist())
    assert np.array_equal(got[4], wantM[0]), "M after update %d: %d of %d floats differ, max %g" % (
        b - 1, int((got[4] != wantM[0]).sum()), wantM.size, float(np.abs(got[4] - wantM[0]).max()))


# ---- d. the block stems in composition --------------------------------------------------------------------------------------------------------------------
# Largest |got - oracle| / |oracle|.max() measured on the MI355X per block over the cases below (profiles/flowscale_gather/README.md); the bar is 4 x that.
STEMS_MEASURED = {0: 1.56e-6, 1: 1.23e-6, 2: 1.06e-6, 3: 9.0e-7}      # block 0: the 333x241 case; the caps measured next to them: 1.6e-5 .. 2.8e-5
STEM_SIZES = [(64, 64), (160, 96), (100, 60)]
STEM_CASES = [(b, w, h, kind) for b in range(4) for w, h in STEM_SIZES for kind in ("smooth", "noise")] + [(b, 333, 241, "scaled") for b in range(4)]


def _lost_lo_effect(net, ins, blob0, blob1):
    """CPU model of a lost lo plane: the block's stem-1 output with stem-0's output rounded to f16, against the same graph left alone.  max |difference|."""
    ins = {k: torch.from_numpy(v) for k, v in ins.items()}
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 8))                               # small frames: a pool sized for a whole machine only waits for itself
    try:
        s0, s1 = net.run(ins, [blob0, blob1])
        (s1r,) = net.run(dict(ins, **{blob0: s0.to(torch.float16).to(torch.float32)}), [blob1])
    finally:
        torch.set_num_threads(threads)
    return float((s1r - s1).abs().max())


@pytest.mark.parametrize("case", STEM_CASES, ids=_ids)
def test_block_stems_match_oracle(fs2, case):
    b, w, h, kind = case
    wp, hp = fr.padded(w, h)
    if kind == "scaled":                                                 # flows that leave the frame: the stems on the block input of (a)
        a, c = gen_frames.smooth_pair(w, h, 21 + b)
        t = 0.5
        inj = fr.injected_flows_scaled(w, h, fr.FLOW_SEED + 6, 3)[:b]
    else:
        a, c = (gen_frames.smooth_pair if kind == "smooth" else gen_frames.noise_pair)(w, h, 21 + b)
        t = 0.5 if kind == "smooth" else 0.4
        rng = np.random.default_rng([b, w, h])
        inj = [(rng.standard_normal((6, hp // s, wp // s)) * 0.3).astype(np.float32) for s in fr.SCALES[:b]]      # a few tenths of a pixel
    C, Ht, Wt = BLOCK_C[b], hp // fr.SCALES[b] // 4, wp // fr.SCALES[b] // 4
    blob0, blob1 = fs2["blobs"]["stems"][b]
    want = fr.extract(fs2["oracle"], a, c, t, 8, blob1, flows=inj)
    assert want.shape == (C, Ht, Wt)
    raw = fs2["g"].v4_tap(a, c, t, 7, b, inj)
    assert np.array_equal(raw, fs2["g"].v4_tap(a, c, t, 7, b, inj)), "two calls on one engine return different bytes"
    assert not raw[s16_ref.exterior_mask(C, Ht, Wt)].any(), "the exterior of the first S16 tensor is not zero"
    err = float(np.abs(s16_ref.value(raw, C, Ht, Wt) - want).max()) / float(np.abs(want).max())
    cap = 0.1 * _lost_lo_effect(fs2["net"], fr.net_inputs(a, c, t, 8, inj), blob0, blob1) / float(np.abs(want).max())
    print("flowscale_gather (d) stems %s err / |oracle|.max = %.3e, cap (lost lo / 10) = %.3e, |oracle|.max = %.3g" % (_ids(case), err, cap, float(np.abs(want).max())))
    assert 4 * STEMS_MEASURED[b] <= cap, "the bar does not fit under a tenth of a lost lo plane"
    assert err <= 4 * STEMS_MEASURED[b]


# ---- f. refusals ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,b,n,word", [(2, 0, 4, "k_final_float"), (3, 2, 2, "flow update"), (5, 3, 3, "stem_rs"), (6, 2, 2, "cascade")])
def test_scale_1_taps_are_einval_at_divisor_2(fs2, what, b, n, word):
    w, h = 100, 60
    a, c = gen_frames.smooth_pair(w, h, 2)
    inj = fr.injected_flows_scaled(w, h, 5, 4)[:n]
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*tap %d.*%s.*flow scale 2" % (amd.EINVAL, what, word)):
        fs2["g"].v4_tap(a, c, 0.5, what, b, inj)
    assert fs2["g"].process(a, c, 0.5).shape == a.shape                  # the engine is unchanged


def test_block0_input_at_divisor_1_is_the_oracles(modeldirs):
    """what = 0, b = 0 is served at both divisors: k_assemble0 / k_assemble0_d10 against the bottom of the stock graph's first stride-2 Convolution, bit for bit."""
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.load(d)
    with open(os.path.join(d, "flownet.param")) as f:
        first = [l for l in (fr._parse(s) for s in f.read().strip("\n").split("\n")[2:] if s.strip()) if l["type"] == "Convolution" and fr._get(l, 3) == "2"][0]
    for (w, h, seed), depth in zip(((100, 60, 3), (333, 241, 6)), (8, 10)):
        a, c = frames(w, h, seed, depth)
        want = deep_ref.extract(o, a, c, 0.4, depth, first["bottoms"][0])
        wp, hp = deep_ref.padded(w, h)
        assert want.shape == (7, hp // 8, wp // 8)
        assert np.array_equal(g.v4_tap(a, c, 0.4, 0, 0, []), want)
