"""The 16 x 16 x 32 products of the conv_rs / conv_rs2 consumer waves, one weight at a time (GPU box only, through rife_hip_op_trunk).

The consumers issue v_mfma_f32_16x16x32_f16 on tiles of 16 output channels x 16 pixels over the 32 input channels of a chunk pair (csrc/rs_frag_geom.h).  A
wrong lane map there moves a product to another channel, pixel or tap; the dense exact case of tests/test_gpu_trunk_ops.py sees that something is wrong, not what.
Here every layer is ONE-HOT: weight 1 at a single (co, ci, tap) with co != ci and tap != centre, bias 0, slope 1, on inputs of s16_ref.exact_case()'s kind, so
the output is x[co] + x[ci] shifted by the tap, exact in fp32 in any order, and the expected BYTES come from s16_ref.trunk_layer.  The (co, ci) pairs straddle the
16-channel (chunk), 32-channel (chunk pair = K of one instruction, and output block N) and tile (channel half) boundaries; the taps are all eight non-centre
ones.  A failure names (co, ci, tap).  RS2 runs two one-hot layers in one launch (the second one the mirrored pair and the opposite tap).  Each case also runs
the fast-precision instantiation: on these inputs the lo planes matter (the expected bytes are then those of hi-only weight taps + the full skip).
Then: conv_rs2 on dense Gaussian input is run-to-run identical."""
import importlib

import numpy as np
import pytest

import s16_ref

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()

C = 64
PAIRS = [(15, 16), (16, 15), (31, 32), (32, 31), (47, 48), (0, 63), (63, 0)]
TAPS = [t for t in range(9) if t != 4]
# (kernel, H, W, cus)
CASES = [("RS", h, w, cus) for h, w in ((7, 33), (8, 32)) for cus in (0, 1)] + [("RS2", 8, 30, 0), ("RS2", 9, 31, 0), ("RS2", 25, 61, 7)]
_X = {}


def _x(H, W):
    """exact_case's activations (on a grid of 2^-12 below 4 at the RS shapes, 2^-10 below 16 at the RS2 shapes; both the hi and the lo plane in use), as values
    and as the packed tensor; computed once per shape"""
    if (H, W) not in _X:
        x = s16_ref.cached_exact_case(C, H, W, 2 if (H, W) not in s16_ref.RS_SHAPES else 1)["x"]
        _X[(H, W)] = (x, s16_ref.pack(x, H, W))
    return _X[(H, W)]


def _one_hot(co, ci, tap):
    w = np.zeros((C, C, 3, 3), np.float32)
    w[co, ci, tap // 3, tap % 3] = 1.0
    return w


def _want(x, ws, fast):
    """the layers in float64 on the {hi, lo} pair the kernel reads; fast: the weight taps see the hi plane only, the skip both (include/rife_hip.h)"""
    cur = np.asarray(x, np.float64)
    for w in ws:
        seen = s16_ref.split(cur.astype(np.float32))[0].astype(np.float64) if fast else cur
        y = s16_ref.trunk_layer(seen, w, np.zeros(C), 1.0) - seen + cur      # conv(seen) + skip(cur); slope 1, bias 0
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
        cur = y
    return cur


@pytest.mark.parametrize("fast", [False, True], ids=["full", "fast"])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_one_hot_layers_bytes(case, flip, fast):
    kernel, H, W, cus = case
    x, xin = _x(H, W)
    bad = []
    for co, ci in PAIRS:
        for tap in TAPS:
            ws = [_one_hot(co, ci, tap)] + ([_one_hot(ci, co, 8 - tap)] if kernel == "RS2" else [])
            n = len(ws)
            got = amd.op_trunk(amd.TRUNK_RS2 if kernel == "RS2" else amd.TRUNK_RS, C, H, W, np.stack(ws) if n > 1 else ws[0], np.zeros((n, C) if n > 1 else C, np.float32),
                               1.0, xin, s16_ref.poisoned(C, H, W), flip=flip, cus=cus, fast=fast)
            want = s16_ref.pack(_want(x, ws, fast).astype(np.float32), H, W)
            if not np.array_equal(got, want):
                gv, wv = s16_ref.value(got, C, H, W), s16_ref.value(want, C, H, W)
                d = np.argwhere(~(gv == wv))
                bad.append("(co %d, ci %d, tap %d): %d of %d elements differ, exterior clean: %s, first (c, y, x) = %s got %r want %r" % (
                    co, ci, tap, len(d), gv.size, not got[s16_ref.exterior_mask(C, H, W)].any(), d[:1].tolist(),
                    gv[tuple(d[0])] if len(d) else None, wv[tuple(d[0])] if len(d) else None))
    assert not bad, "%d of %d one-hot layers wrong:\n%s" % (len(bad), len(PAIRS) * len(TAPS), "\n".join(bad[:12]))


def test_rs2_dense_gaussian_is_run_to_run_identical():
    H, W, cus = 25, 61, 7
    rng = np.random.default_rng([C, H, W])
    g = s16_ref.gauss_case(C, H, W, rng)
    xin = s16_ref.pack(g["x"].astype(np.float32), H, W)
    w2 = np.stack([g["w"], g["w"][::-1, ::-1].copy()])
    b2 = np.stack([g["b"], -g["b"]])
    for flip in (0, 1):
        runs = [amd.op_trunk(amd.TRUNK_RS2, C, H, W, w2, b2, 0.2, xin, s16_ref.poisoned(C, H, W), flip=flip, cus=cus) for _ in range(4)]
        for k in range(1, 4):
            assert np.array_equal(runs[0], runs[k]), "flip %d: run %d differs from run 0 in %d bytes" % (flip, k, int((runs[0] != runs[k]).sum()))
