"""tests/s16_ref.py without a GPU: the S16 layout against the header of csrc/conv_t64.h restated byte by byte, the float64 trunk layer against the CPU oracle,
and the precondition of every exact case the GPU tests (tests/test_gpu_trunk_ops.py) use - the check that the reference ALONE stays where fp32 sums are exact."""
import importlib

import numpy as np
import pytest

import s16_ref
from oracle import pyoracle

amd = importlib.import_module("rife-ncnn-vulkan_amd")


@pytest.mark.parametrize("C,H,W", [(16, 1, 1), (64, 9, 33), (96, 8, 32), (192, 17, 70)])
def test_geometry_is_the_librarys(C, H, W):
    """S16Geom through the test build's entry point (no device needed) == the numpy restatement."""
    assert amd.test_build().op_s16_geom(C, H, W) == s16_ref.geom(C, H, W)


def test_layout_byte_for_byte():
    """Plane [chunk][hi | lo], rows x pitch pixels of 32 bytes, pixel (y, x) at (y + 1, x + 1), channel c of a chunk at byte 2 c: written out per element."""
    C, H, W = 32, 3, 33
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((C, H, W)) * 5).astype(np.float32)
    t = s16_ref.pack(x, H, W)
    pitch, rows, plane, nbytes = s16_ref.geom(C, H, W)
    assert (pitch, rows, plane, nbytes) == (66, 10, 10 * 66 * 32, 4 * 10 * 66 * 32) and t.size == nbytes
    want = np.zeros(nbytes, np.uint8)
    for c in range(C):
        for y in range(H):
            for xx in range(W):
                hi = np.float16(x[c, y, xx])
                lo = np.float16(x[c, y, xx] - np.float32(hi))
                for k, v in enumerate((hi, lo)):
                    o = (2 * (c // 16) + k) * plane + ((y + 1) * pitch + xx + 1) * 32 + (c % 16) * 2
                    want[o:o + 2] = np.frombuffer(v.tobytes(), np.uint8)
    assert np.array_equal(t, want)
    ext = s16_ref.exterior_mask(C, H, W)
    assert ext.sum() == nbytes - C * H * W * 4 and not t[ext].any()
    p = s16_ref.poisoned(C, H, W)
    assert not p[ext].any() and np.all(p[~ext].view(np.uint16) == 0x7e00) and np.isnan(s16_ref.value(p, C, H, W)).all()


def test_pack_unpack_round_trip():
    """hi + lo reproduces x to 2^-22 relative (lo carries 11 bits below hi's 11; |x| >= 1 keeps the absolute error of an f16-subnormal lo, 2^-25, inside that)."""
    C, H, W = 64, 9, 33
    rng = np.random.default_rng(2)
    x = (rng.uniform(1, 1000, (C, H, W)) * rng.choice([-1, 1], (C, H, W))).astype(np.float32)
    t = s16_ref.pack(x, H, W)
    hi, lo = s16_ref.unpack(t, C, H, W)
    assert hi.dtype == lo.dtype == np.float16 and np.array_equal(hi, x.astype(np.float16))
    assert (lo != 0).mean() > 0.9
    got = s16_ref.value(t, C, H, W)
    assert np.all(np.abs(got - x) <= 2.0 ** -22 * np.abs(x))


@pytest.mark.parametrize("C,H,W", [(16, 5, 7), (64, 9, 33)])
def test_trunk_layer_matches_the_oracle(C, H, W):
    rng = np.random.default_rng(C)
    x = rng.standard_normal((C, H, W)).astype(np.float32)
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    want = pyoracle.conv2d(x, w, b, stride=1, pad=1) + x
    want = np.where(want < 0, want * np.float32(0.2), want)
    got = s16_ref.trunk_layer(x, w, b, 0.2)
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 2e-5 * (1.0 + np.abs(w).sum(axis=(1, 2, 3)).max() * np.abs(x).max())      # the oracle's fp32 sums (tests/test_gpu_kernels.py conv_tol)
    assert (got < 0).any() and (got > 0).any()


@pytest.mark.parametrize("kernel,C,H,W,n_layers", sorted(set(s16_ref.exact_cases())))
def test_exact_case_holds_its_precondition(kernel, C, H, W, n_layers):
    """exact_case() asserts its precondition itself; restated here from the arrays it returns, for every (kernel, C, shape) of the GPU tests."""
    e = s16_ref.cached_exact_case(C, H, W, n_layers)
    assert e["w"].shape == (n_layers, C, C, 3, 3) and e["slope"] == 0.25 and len(e["want"]) == n_layers
    assert set(np.unique(e["w"])) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    (hi, lo), g = s16_ref.split(e["x"]), e["g_out"] - 2 * n_layers
    for i in range(n_layers):
        w, b = e["w"][i], e["b"][i]
        cur = hi.astype(np.float64) + lo.astype(np.float64)
        assert np.all((w != 0).sum(axis=0) >= 3)                         # every (tap, input channel) feeds several output channels
        assert not np.array_equal(w, w[:, :, ::-1, :]) and not np.array_equal(w, w[:, :, :, ::-1]) and not np.array_equal(w, w.transpose(0, 1, 3, 2))
        for a in (hi, lo, b):
            s = a.astype(np.float64) * 2.0 ** g
            assert np.array_equal(s, np.round(s))
        assert (lo != 0).mean() > 0.5
        assert s16_ref.abs_sum(cur, w, b) * 2.0 ** g < 2.0 ** 24
        want = s16_ref.trunk_layer(cur, w, b, 0.25)
        assert np.array_equal(want, e["want"][i])
        hi, lo = s16_ref.split(want.astype(np.float32))                  # the stored pair: the next layer's input
        assert np.all((lo == 0) | (np.abs(lo.astype(np.float64)) >= 2.0 ** -14))
        g += 2
        assert (want < 0).mean() > 0.2 and (want > 0).mean() > 0.2 or H * W == 1
