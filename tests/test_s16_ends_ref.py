"""tests/s16_ends_ref.py without a GPU: the float64 stem-1 and head definitions against the CPU oracle, and the precondition and the POWER check of every exact case
tests/test_gpu_s16_ends.py uses - a case that would prove nothing (a partial sum past 2^24 grid steps, an f16-subnormal lo, a lo plane whose loss moves fewer than
half of the outputs) fails here, where no GPU is needed."""
import numpy as np
import pytest

import s16_ends_ref as ends
import s16_ref
from oracle import pyoracle


@pytest.mark.parametrize("C,Ht,Wt", [(16, 3, 5), (64, 5, 33)])
def test_stem1_layer_matches_the_oracle(C, Ht, Wt):
    rng = np.random.default_rng(C)
    x = rng.standard_normal((C // 2, 2 * Ht, 2 * Wt)).astype(np.float32)
    w = (rng.standard_normal((C, C // 2, 3, 3)) / np.sqrt(9 * C // 2)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    want = pyoracle.conv2d(x, w, b, stride=2, pad=1, act_type=2, act_p0=0.2)
    got = ends.stem1_layer(x, w, b, 0.2)
    assert got.dtype == np.float64 and got.shape == want.shape == (C, Ht, Wt)
    assert np.abs(got - want).max() <= 2e-5 * (1.0 + np.abs(w).sum(axis=(1, 2, 3)).max() * np.abs(x).max())      # the oracle's fp32 sums (tests/test_gpu_kernels.py conv_tol)
    assert (got < 0).any() and (got > 0).any()


@pytest.mark.parametrize("C,Ht,Wt", [(16, 3, 5), (64, 9, 33)])
def test_head_ps_matches_the_oracle(C, Ht, Wt):
    rng = np.random.default_rng(C + 1)
    x = rng.standard_normal((C, Ht, Wt)).astype(np.float32)
    w = (rng.standard_normal((24, C, 4, 4)) / np.sqrt(4 * C)).astype(np.float32)
    b = rng.standard_normal(24).astype(np.float32)
    want = pyoracle.pixelshuffle(pyoracle.deconv2d(x, w, b), 2)
    got = ends.head_ps(x, w, b)
    assert got.dtype == np.float64 and got.shape == want.shape == (6, 4 * Ht, 4 * Wt)
    assert np.abs(got - want).max() <= 2e-5 * (1.0 + np.abs(w).sum(axis=(1, 2, 3)).max() * np.abs(x).max())
    # no symmetry the reference could hide behind: a flipped or transposed kernel is another function
    assert np.abs(ends.head_ps(x, w[:, :, ::-1], b) - got).max() > 0.1 and np.abs(ends.head_ps(x, w.transpose(0, 1, 3, 2), b) - got).max() > 0.1


def test_case_table_is_the_issues():
    assert len(ends.stem1_cases()) == 4 * 5 and len(ends.head_cases()) == 4 * 4 + 2 * 4
    assert set(c for c, _, _ in ends.stem1_cases()) == {64, 96, 128, 192}
    assert {(h, w) for _, h, w in ends.stem1_cases()} == {(1, 1), (4, 32), (5, 33), (2, 70), (9, 65)}
    assert {(h, w) for _, h, w, _ in ends.head_cases()} == {(1, 1), (8, 32), (9, 33), (17, 70)}
    assert {c for c, _, _, s in ends.head_cases() if not s} == {192, 64}


@pytest.mark.parametrize("C,Ht,Wt", ends.stem1_cases())
def test_stem1_exact_case_holds_its_precondition_and_has_power(C, Ht, Wt):
    """stem1_exact_case() asserts these itself; restated from the arrays it returns."""
    e = ends.cached("stem1_exact", C, Ht, Wt)
    x, w, b = e["x"], e["w"], e["b"]
    assert x.shape == (C // 2, 2 * Ht, 2 * Wt) and w.shape == (C, C // 2, 3, 3) and b.shape == (C,) and e["slope"] == 0.25
    assert set(np.unique(w)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and np.all((w != 0).sum(axis=0) >= 3)
    assert not np.array_equal(w, w[:, :, ::-1, :]) and not np.array_equal(w, w[:, :, :, ::-1]) and not np.array_equal(w, w.transpose(0, 1, 3, 2))
    hi, lo = s16_ref.split(x)
    for a in (hi, lo, b):
        s = a.astype(np.float64) * 2.0 ** 12
        assert np.array_equal(s, np.round(s))
    assert np.abs(x).max() < 4
    assert ends.stem1_abs_sum(hi, lo, w, b) * 2.0 ** 12 < 2.0 ** 24 and 0 < e["bound"] < 1
    want = ends.stem1_layer(x, w, b, 0.25)
    assert np.array_equal(want, e["want"]) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    ohi, olo = s16_ref.split(want.astype(np.float32))
    assert np.all((olo == 0) | (np.abs(olo.astype(np.float64)) >= 2.0 ** -14))      # the output lo is normal or zero
    # power: the lo plane dropped at the input, zeroed at the output
    assert (ends.stem1_layer(hi.astype(np.float64), w, b, 0.25) != want).mean() > 0.5
    assert (ohi.astype(np.float64) != want).mean() > 0.5
    assert (want < 0).mean() > 0.2 and (want > 0).mean() > 0.2
    print("s16_ends stem-1 exact C=%d %dx%d: density %.2f, bound %.2f of 2^24, lo dropped at the input moves %.3f of the outputs, output lo non-zero %.3f" % (
        C, Ht, Wt, e["density"], e["bound"], e["power_in"], e["power_out"]))


@pytest.mark.parametrize("C,Ht,Wt", sorted(set(c[:3] for c in ends.head_cases())))
def test_head_exact_case_holds_its_precondition_and_has_power(C, Ht, Wt):
    e = ends.cached("head_exact", C, Ht, Wt)
    x, w, b = e["x"], e["w"], e["b"]
    assert x.shape == (C, Ht, Wt) and w.shape == (24, C, 4, 4) and b.shape == (24,)
    assert set(np.unique(w)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and np.all((w != 0).sum(axis=0) >= 3)
    assert not np.array_equal(w, w[:, :, ::-1, :]) and not np.array_equal(w, w[:, :, :, ::-1]) and not np.array_equal(w, w.transpose(0, 1, 3, 2))
    hi, lo = s16_ref.split(x)
    assert np.array_equal(s16_ref.value(s16_ref.pack(x, Ht, Wt), C, Ht, Wt), x)      # the S16 tensor holds exactly these values
    for a in (hi, lo, b):
        s = a.astype(np.float64) * 2.0 ** 12
        assert np.array_equal(s, np.round(s))
    assert np.abs(x).max() < 4 and (lo != 0).mean() > 0.5
    assert ends.head_abs_sum(hi, lo, w, b) * 2.0 ** 12 < 2.0 ** 24 and 0 < e["bound"] < 1
    want = ends.head_ps(x, w, b)
    assert want.shape == (6, 4 * Ht, 4 * Wt) and np.array_equal(want, e["want"]) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert (ends.head_ps(hi.astype(np.float64), w, b) != want).mean() > 0.5
    print("s16_ends head exact C=%d %dx%d: density %.2f, bound %.2f of 2^24, lo dropped moves %.3f of the outputs" % (C, Ht, Wt, e["density"], e["bound"], e["power_in"]))


@pytest.mark.parametrize("kind,C,Ht,Wt", [("stem1_gauss", 96, 5, 33), ("head_gauss", 128, 9, 33), ("stem1_gauss", 64, 1, 1), ("head_gauss", 64, 1, 1)])
def test_dense_cases_are_what_the_kernel_reads(kind, C, Ht, Wt):
    """Activations over six decades that ARE their {hi, lo} pair, fp16 weights, a reference with both signs."""
    g = ends.cached(kind, C, Ht, Wt)
    hi, lo = s16_ref.split(g["x"])
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), g["x"].astype(np.float64))
    assert np.array_equal(g["w"].astype(np.float16).astype(np.float32), g["w"])
    assert np.abs(g["x"]).max() > 100 * np.abs(g["x"][:, :2]).max() or g["x"].shape[1] <= 2
    assert (g["want"] < 0).any() and (g["want"] > 0).any()
