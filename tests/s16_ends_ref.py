"""The two ENDS of an S16 trunk restated in numpy (no GPU): the reference of tests/test_gpu_s16_ends.py, next to tests/s16_ref.py (layout, split, pack).

stem-1 (csrc/conv_mfma.h conv_h2s2_kernel<NS, true>): 3 x 3 stride-2 pad-1 convolution C / 2 -> C on an fp32 NHWC tensor that the kernel splits into {hi, lo}
itself, + bias, LeakyReLU with the multiply in fp32, output split into the first S16 tensor of the block.
head (csrc/head_h2.h head_h2_kernel<EPI_DECONV_PS, S16IN>): 4 x 4 stride-2 pad-1 transposed convolution C -> 24 on the last S16 tensor (or on an fp32 tensor it
splits itself) + bias, PixelShuffle(2) into planes 0 - 5 of the flow tensor [4 Ht][4 Wt][8].

The exact cases follow s16_ref.exact_case(): operands on the grid 2^-12, integer weights, every partial sum of hi- and lo-products below 2^24 grid steps, so fp32
accumulation is exact in any order and the expected bytes are determined.  Every builder asserts its precondition from the arrays it made, and a POWER check: the
same reference on hi alone (the lo plane dropped), and for stem-1 with the output's lo zeroed, must differ from the expected tensor on more than half of the
outputs - a case on which a lost lo plane would go unseen fails here, on the CPU."""
import numpy as np

import s16_ref

G_IN = 12                      # activations k 2^-12 in (-4, 4)
AMP = 4
CHANNELS = (64, 96, 128, 192)
# (Ht, Wt).  stem-1: tiles of 4 x 32 outputs; (9, 65) gives 9 x nz workgroups, so the XCD remap of blockIdx.x has a remainder.  head: tiles of 8 x 32.
STEM1_SHAPES = [(1, 1), (4, 32), (5, 33), (2, 70), (9, 65)]
HEAD_SHAPES = [(1, 1), (8, 32), (9, 33), (17, 70)]
HEAD_F32_CHANNELS = (192, 64)  # head_h2_kernel<EPI_DECONV_PS, false>: the block that leaves the S16 path


def stem1_cases():
    return [(C, h, w) for C in CHANNELS for h, w in STEM1_SHAPES]


def head_cases():
    """(C, Ht, Wt, s16)"""
    return [(C, h, w, 1) for C in CHANNELS for h, w in HEAD_SHAPES] + [(C, h, w, 0) for C in HEAD_F32_CHANNELS for h, w in HEAD_SHAPES]


# ---- float64 definitions -------------------------------------------------------------------------------------------------------------------------------
def conv3x3s2_f64(x, w):
    """3 x 3 convolution, pad 1, stride 2, in float64: x (Cin, 2 Ht, 2 Wt), w (O, Cin, 3, 3) -> (O, Ht, Wt)."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    _, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0
    Ho, Wo = H // 2, W // 2
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    y = np.zeros((w.shape[0], Ho, Wo))
    for ky in range(3):
        for kx in range(3):
            y += np.tensordot(w[:, :, ky, kx], xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], axes=(1, 0))
    return y


def stem1_layer(x, w, b, slope):
    """y = conv3x3 stride 2 (x) + b, then y < 0 ? f32(y) * f32(slope) : y: the epilogue of s16_ref.trunk_layer without the skip.  Returns float64."""
    y = conv3x3s2_f64(x, w) + np.asarray(b, np.float64)[:, None, None] + 0.0
    neg = (y.astype(np.float32) * np.float32(slope)).astype(np.float64)
    return np.where(y < 0, neg, y)


def deconv4x4s2_f64(x, w):
    """4 x 4 transposed convolution, stride 2, pad 1 (ncnn Deconvolution, weights [oc][ic][ky][kx]): out[oc, 2 iy + ky - 1, 2 ix + kx - 1] += w[oc, ic, ky, kx] x[ic, iy, ix]."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    _, H, W = x.shape
    full = np.zeros((w.shape[0], 2 * H + 2, 2 * W + 2))
    for ky in range(4):
        for kx in range(4):
            full[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.tensordot(w[:, :, ky, kx], x, axes=(1, 0))
    return full[:, 1:2 * H + 1, 1:2 * W + 1]


def pixelshuffle2(d):
    """(4 n, H, W) -> (n, 2 H, 2 W): out[c, 2 y + i, 2 x + j] = d[4 c + 2 i + j, y, x]."""
    n, H, W = d.shape[0] // 4, d.shape[1], d.shape[2]
    return d.reshape(n, 2, 2, H, W).transpose(0, 3, 1, 4, 2).reshape(n, 2 * H, 2 * W)


def head_ps(x, w, b):
    """x (C, Ht, Wt), w (24, C, 4, 4), b (24) -> the six planes (6, 4 Ht, 4 Wt) of blob flow{b}, float64."""
    return pixelshuffle2(deconv4x4s2_f64(x, w) + np.asarray(b, np.float64)[:, None, None])


def stem1_abs_sum(hi, lo, w, b):
    """max over outputs of sum |w| (|hi| + |lo|) + |b|: bounds every partial sum the kernel can form, in any order."""
    a = np.abs(hi.astype(np.float64)) + np.abs(lo.astype(np.float64))
    return float((conv3x3s2_f64(a, np.abs(w)) + np.abs(np.asarray(b, np.float64))[:, None, None]).max())


def head_abs_sum(hi, lo, w, b):
    a = np.abs(hi.astype(np.float64)) + np.abs(lo.astype(np.float64))
    return float((deconv4x4s2_f64(a, np.abs(w)) + np.abs(np.asarray(b, np.float64))[:, None, None]).max())


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------------------
DENSITIES = (1.0, 0.75, 0.5, 0.25)      # tried in this order: the weights are as dense as the 2^24 bound allows


def _int_weights(shape, density, rng):
    """integers from {-2, .., 2} \\ {0} at `density` of the places (+-1 and +-2 alike), topped up so that every (input channel, tap) is non-zero for at least three
    output channels."""
    n = int(np.prod(shape))
    v = (rng.choice([-1.0, 1.0], n) * rng.choice([1.0, 2.0], n)).reshape(shape).astype(np.float32)
    w = np.where(rng.random(shape) < density, v, np.float32(0)).astype(np.float32)
    for idx in zip(*np.nonzero((w != 0).sum(axis=0) < 3)):
        col = w[(slice(None),) + idx]
        free = np.nonzero(col == 0)[0]
        add = rng.choice(free, 3 - (shape[0] - free.size), replace=False)
        col[add] = rng.choice([-2.0, -1.0, 1.0, 2.0], add.size)
    return w


def _grid_values(shape, rng):
    return (rng.integers(-AMP * 2 ** G_IN + 1, AMP * 2 ** G_IN, shape) * 2.0 ** -G_IN).astype(np.float32)


def _differs(a, b):
    return float((np.asarray(a) != np.asarray(b)).mean())


def stem1_exact_case(C, Ht, Wt, rng):
    """dict(x fp32 (C / 2, 2 Ht, 2 Wt), w, b, slope 0.25, want float64 (C, Ht, Wt), density, bound (fraction of 2^24), power_in, power_out)."""
    g, slope = G_IN, 0.25
    x = _grid_values((C // 2, 2 * Ht, 2 * Wt), rng)
    hi, lo = s16_ref.split(x)                                                 # the pair the kernel makes of it in LDS
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), x)   # 15 bits: the split loses nothing
    b = (rng.integers(-2 ** g + 1, 2 ** g, C) * 2.0 ** -g).astype(np.float32)
    for density in DENSITIES:
        w = _int_weights((C, C // 2, 3, 3), density, rng)
        bound = stem1_abs_sum(hi, lo, w, b) * 2.0 ** g
        if bound < 2.0 ** 24:
            break
    assert bound < 2.0 ** 24, "|partial sums| reach %.3g grid steps (limit 2^24 = 1.7e7)" % bound
    assert s16_ref._on_grid(hi, g) and s16_ref._on_grid(lo, g) and s16_ref._on_grid(b, g) and s16_ref._on_grid(w, 0)
    assert np.all((w != 0).sum(axis=0) >= 3), "an (input channel, tap) that fewer than three output channels use"
    want = stem1_layer(x, w, b, slope)
    assert s16_ref._on_grid(want, g + 2) and np.array_equal(want.astype(np.float32).astype(np.float64), want)      # an fp32 value, exactly
    ohi, olo = s16_ref.split(want.astype(np.float32))
    assert np.all((olo == 0) | (np.abs(olo.astype(np.float64)) >= s16_ref.MIN_NORMAL_F16)), "an f16-subnormal lo in the output"
    # power: the input's lo dropped / the output's lo zeroed must each move more than half of the outputs
    power_in = _differs(stem1_layer(hi.astype(np.float64), w, b, slope), want)
    power_out = float((olo != 0).mean())
    assert power_in > 0.5, "dropping the input's lo plane changes only %.2f of the outputs" % power_in
    assert power_out > 0.5, "the output's lo is non-zero for only %.2f of the outputs" % power_out
    return dict(x=x, w=w, b=b, slope=slope, want=want, density=density, bound=bound / 2.0 ** 24, power_in=power_in, power_out=power_out)


def head_exact_case(C, Ht, Wt, rng):
    """dict(x fp32 (C, Ht, Wt) = hi + lo exactly, w (24, C, 4, 4), b (24), want float64 (6, 4 Ht, 4 Wt), density, bound, power_in)."""
    g = G_IN
    x = _grid_values((C, Ht, Wt), rng)
    hi, lo = s16_ref.split(x)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), x)
    assert (lo != 0).mean() > 0.5
    b = (rng.integers(-2 ** g + 1, 2 ** g, 24) * 2.0 ** -g).astype(np.float32)
    for density in DENSITIES:
        w = _int_weights((24, C, 4, 4), density, rng)
        bound = head_abs_sum(hi, lo, w, b) * 2.0 ** g
        if bound < 2.0 ** 24:
            break
    assert bound < 2.0 ** 24, "|partial sums| reach %.3g grid steps (limit 2^24 = 1.7e7)" % bound
    assert s16_ref._on_grid(hi, g) and s16_ref._on_grid(lo, g) and s16_ref._on_grid(b, g) and s16_ref._on_grid(w, 0)
    assert np.all((w != 0).sum(axis=0) >= 3)
    want = head_ps(x, w, b)
    assert s16_ref._on_grid(want, g) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    power_in = _differs(head_ps(hi.astype(np.float64), w, b), want)
    assert power_in > 0.5, "dropping the lo plane changes only %.2f of the outputs" % power_in
    return dict(x=x, w=w, b=b, want=want, density=density, bound=bound / 2.0 ** 24, power_in=power_in)


# ---- dense cases (s16_ref.gauss_case): six decades of magnitude, weights N(0, 1 / fan-in) rounded to fp16 ------------------------------------------------
def _through_split(x):
    """fp32 -> the value hi + lo of its {hi, lo} pair, which is what either kernel multiplies; returned as fp32 (asserted exact) so that the kernel's own split
    of it gives the same pair."""
    hi, lo = s16_ref.split(x)
    v = hi.astype(np.float64) + lo.astype(np.float64)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    h2, l2 = s16_ref.split(v32)                      # on a tie f16(v) may pick the other neighbour: another pair, the same value
    assert np.array_equal(h2.astype(np.float64) + l2.astype(np.float64), v)
    return v32


def _gauss_x(shape, rng):
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    x[:, :2] *= 1e-4
    x[:, 2:4] *= 300.0
    return _through_split(x)


def stem1_gauss_case(C, Ht, Wt, rng):
    x = _gauss_x((C // 2, 2 * Ht, 2 * Wt), rng)
    w = (rng.standard_normal((C, C // 2, 3, 3)) / np.sqrt(9 * C // 2)).astype(np.float16).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    return dict(x=x, w=w, b=b, slope=0.2, want=stem1_layer(x, w, b, 0.2))


def head_gauss_case(C, Ht, Wt, rng):
    x = _gauss_x((C, Ht, Wt), rng)
    w = (rng.standard_normal((24, C, 4, 4)) / np.sqrt(4 * C)).astype(np.float16).astype(np.float32)      # four taps of every input channel reach an output
    b = rng.standard_normal(24).astype(np.float32)
    return dict(x=x, w=w, b=b, want=head_ps(x, w, b))


_CACHE = {}


def cached(kind, C, Ht, Wt):
    """kind in stem1_exact / head_exact / stem1_gauss / head_gauss with the seed (kind, C, Ht, Wt): computed once per process and shared (do not modify)."""
    key = (kind, C, Ht, Wt)
    if key not in _CACHE:
        kinds = {"stem1_exact": stem1_exact_case, "head_exact": head_exact_case, "stem1_gauss": stem1_gauss_case, "head_gauss": head_gauss_case}
        _CACHE[key] = kinds[kind](C, Ht, Wt, np.random.default_rng([sorted(kinds).index(kind), C, Ht, Wt]))
    return _CACHE[key]
