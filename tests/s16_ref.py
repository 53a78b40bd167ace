"""The S16 trunk tensor and one residual trunk layer, restated in numpy (no GPU): the reference of tests/test_gpu_trunk_ops.py.

Layout (header of csrc/conv_t64.h): a C-channel tensor is 2 C / 16 planes, ordered [16-channel chunk][hi | lo]; a plane is rows x pitch pixels of
32 bytes (the 16 f16 of the chunk), pixel (y, x) of the H x W grid sits at (y + 1, x + 1), everything else in a plane is zero.  hi = f16(x),
lo = f16(x - hi), both round-to-nearest-even.  pitch = 32 ceil(W / 32) + 2 and rows = 8 ceil(H / 8) + 2 (S16Geom, csrc/engine_dispatch.h; the GPU test
holds geom() against rife_hip_op_s16_geom).

exact_case() makes inputs on which the kernels have NO rounding to do before the output split: every product and every partial sum of hi- and
lo-products is a multiple of one grid step 2^-g' and stays below 2^24 steps, so the fp32 accumulators of the matrix pipe are exact in any
summation order, the bias add is exact, and the slope 0.25 multiply is exact.  The expected hi and lo planes are then determined to the bit.
Outputs must keep lo out of the f16 subnormal range (|lo| >= 2^-14 or lo == 0), which pins the output grid at 2^-14: one layer takes activations
k 2^-12 in (-4, 4), two layers k 2^-10 in (-16, 16) (each layer's slope costs two bits of grid): 14 / 15 bits per activation against the 11 of an f16, so
lo is non-zero for two activations in three.  A finer grid (g = 16, |x| < 1) would put most output lo values into the f16 subnormal range."""
import numpy as np

F16_NAN = 0x7e00
MIN_NORMAL_F16 = 2.0 ** -14


def geom(C, H, W):
    """(pitch, rows, plane_bytes, bytes) of the S16 tensor of a C x H x W trunk."""
    pitch = (W + 31) // 32 * 32 + 2
    rows = (H + 7) // 8 * 8 + 2
    plane = rows * pitch * 32
    return pitch, rows, plane, plane * (C // 8)


def split(x):
    """fp32 -> (hi, lo) f16, round-to-nearest-even: hi = f16(x), lo = f16(x - hi) with the difference taken in fp32 (it is exact there)."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _planes(t, C, H, W):
    pitch, rows, _, nbytes = geom(C, H, W)
    t = np.asarray(t, np.uint8).reshape(-1)
    assert t.size == nbytes, (t.size, nbytes)
    return t.view(np.uint16).reshape(C // 16, 2, rows, pitch, 16)      # [chunk][hi | lo][row][column][channel of the chunk]


def pack(x, H, W):
    """(C, H, W) fp32 -> the raw S16 tensor, a flat uint8 array."""
    x = np.asarray(x, np.float32)
    C = x.shape[0]
    assert x.shape == (C, H, W) and C % 16 == 0
    t = np.zeros(geom(C, H, W)[3], np.uint8)
    p = _planes(t, C, H, W)
    hi, lo = split(x)
    for k, part in enumerate((hi, lo)):
        p[:, k, 1:H + 1, 1:W + 1, :] = part.view(np.uint16).reshape(C // 16, 16, H, W).transpose(0, 2, 3, 1)
    return t


def unpack(t, C, H, W):
    """raw S16 tensor -> (hi, lo), two (C, H, W) f16 arrays (the interior only)."""
    p = _planes(t, C, H, W)
    return tuple(np.ascontiguousarray(p[:, k, 1:H + 1, 1:W + 1, :].transpose(0, 3, 1, 2)).reshape(C, H, W).view(np.float16) for k in (0, 1))


def value(t, C, H, W):
    """hi + lo in float64."""
    hi, lo = unpack(t, C, H, W)
    return hi.astype(np.float64) + lo.astype(np.float64)


def exterior_mask(C, H, W):
    """bool per BYTE of the tensor: True for everything that is not the H x W interior of a plane (borders, columns W .. pitch, rows H .. rows)."""
    pitch, rows, _, nbytes = geom(C, H, W)
    m = np.ones((C // 8, rows, pitch, 32), bool)
    m[:, 1:H + 1, 1:W + 1, :] = False
    return m.reshape(-1)


def poisoned(C, H, W):
    """an output tensor before the launch: the interior full of f16 NaNs, the exterior zero."""
    t = np.zeros(geom(C, H, W)[3], np.uint8)
    _planes(t, C, H, W)[:, :, 1:H + 1, 1:W + 1, :] = F16_NAN
    return t


def conv3x3_f64(x, w):
    """3 x 3 convolution, pad 1, stride 1, in float64: x (C, H, W), w (O, C, 3, 3)."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    y = np.zeros((w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            y += np.tensordot(w[:, :, ky, kx], xp[:, ky:ky + H, kx:kx + W], axes=(1, 0))
    return y


def trunk_layer(x, w, b, slope):
    """y = conv3x3(x, pad 1) + b + x in float64, then y < 0 ? f32(y) * f32(slope) : y with the multiply done in fp32 (the epilogue order of
    csrc/conv_mfma.h around s16_store_chunk: accumulator + bias, activation, split).  Returns float64."""
    x = np.asarray(x, np.float64)
    y = conv3x3_f64(x, w) + np.asarray(b, np.float64)[:, None, None] + x + 0.0
    neg = (y.astype(np.float32) * np.float32(slope)).astype(np.float64)
    return np.where(y < 0, neg, y)


def abs_sum(x, w, b):
    """max over outputs of sum |w| |x| + |b| + |x|: a bound on every partial sum the kernel can form, whatever the order."""
    return float((conv3x3_f64(np.abs(x), np.abs(w)) + np.abs(np.asarray(b, np.float64))[:, None, None] + np.abs(x)).max())


def _on_grid(a, g):
    s = np.asarray(a, np.float64) * 2.0 ** g
    return bool(np.all(s == np.round(s)))


def _sparse_weights(C, nnz, p2, rng):
    """(C, C, 3, 3) from {-2, -1, 0, 1, 2} (a non-zero weight is +-2 with probability p2): about nnz non-zero taps per output channel at random places (no symmetry
    between taps or channels), topped up so that every (tap, input channel) is non-zero for at least three output channels."""
    def values(n):
        return (rng.choice([-1.0, 1.0], n) * np.where(rng.random(n) < p2, 2.0, 1.0)).astype(np.float32)
    w = np.where(rng.random((C, C, 3, 3)) < nnz / (9.0 * C), values(C * C * 9).reshape(C, C, 3, 3), np.float32(0)).astype(np.float32)
    for ci, ky, kx in zip(*np.nonzero((w != 0).sum(axis=0) < 3)):
        free = np.nonzero(w[:, ci, ky, kx] == 0)[0]
        add = rng.choice(free, 3 - (C - free.size), replace=False)
        w[add, ci, ky, kx] = values(add.size)
    return w


def exact_case(C, H, W, rng, n_layers=1):
    """Inputs on which fp32 accumulation is exact in any order, with the expected output tensor(s) determined to the bit.
    Returns dict(x, w [n, C, C, 3, 3], b [n, C], slope, want [per layer, float64], g_out).  Asserts its own precondition from the arrays it made."""
    assert n_layers in (1, 2)
    # one layer: 1 tap in 8, +-1 and +-2 alike.  Two layers: the second layer's sums grow with the first one's gain and both slopes cost grid bits, so the weights
    # are as sparse as "every (tap, input channel) reaches three output channels" allows (27 taps per output channel) and mostly +-1
    g, amp, nnz, p2 = (12, 4, 9 * C // 8, 0.5) if n_layers == 1 else (10, 16, 0, 0.1)
    slope = 0.25
    x = (rng.integers(-amp * 2 ** g + 1, amp * 2 ** g, (C, H, W)) * 2.0 ** -g).astype(np.float32)
    ws, bs, wants = [], [], []
    hi, lo = split(x)                                                        # the pair the kernel reads
    for i in range(n_layers):
        cur = hi.astype(np.float64) + lo.astype(np.float64)
        w = _sparse_weights(C, nnz, p2, rng)
        b = (rng.integers(-2 ** g + 1, 2 ** g, C) * 2.0 ** -g).astype(np.float32)
        # ---- the precondition: operands on the grid 2^-g (x: hi and lo separately), integer weights, and every partial sum below 2^24 grid steps
        nz = float((lo != 0).mean())
        assert nz > 0.5, "layer %d: lo is zero for most activations (%.2f non-zero)" % (i, nz)
        assert i > 0 or np.array_equal(cur, x), "the input is not an {hi, lo} pair"
        assert _on_grid(hi, g) and _on_grid(lo, g) and _on_grid(b, g) and _on_grid(w, 0)
        assert np.all((w != 0).sum(axis=0) >= 3), "a (tap, input channel) that fewer than three output channels use"
        bound = abs_sum(cur, w, b) * 2.0 ** g
        assert bound < 2.0 ** 24, "layer %d: |partial sums| reach %.3g grid steps (limit 2^24 = 1.7e7)" % (i, bound)
        y = trunk_layer(cur, w, b, slope)
        g += 2                                                               # y * 0.25
        assert _on_grid(y, g) and np.array_equal(y.astype(np.float32).astype(np.float64), y)      # an fp32 value, exactly
        hi, lo = split(y.astype(np.float32))                                 # what the kernel stores and the next layer reads
        assert np.all((lo == 0) | (np.abs(lo.astype(np.float64)) >= MIN_NORMAL_F16)), "an f16-subnormal lo in the output"
        ws.append(w); bs.append(b); wants.append(y)
    return dict(x=x, w=np.stack(ws), b=np.stack(bs), slope=slope, want=wants, g_out=g)


def gauss_case(C, H, W, rng):
    """The dense case of tests/test_gpu_kernels.py::test_conv3x3_split_f16_trunk_path_matches_oracle on an S16 tensor: activations N(0, 3) with rows 0 - 1
    scaled by 1e-4 and rows 2 - 3 by 300, rounded through the {hi, lo} pair (the tensor the kernel sees); dense weights N(0, 1 / (9 C)) rounded to fp16."""
    x = (rng.standard_normal((C, H, W)) * 3).astype(np.float32)
    x[:, :2] *= 1e-4
    x[:, 2:4] *= 300.0
    x = value(pack(x, H, W), C, H, W)
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(C * 9)).astype(np.float16).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    return dict(x=x, w=w, b=b, slope=0.2)


# ---- the cases of tests/test_gpu_trunk_ops.py: (kernel, C, H, W, n_layers).  tests/test_s16_ref.py builds every one on the CPU, so that the
# precondition of exact_case() is checked where no GPU is needed.
ROW_SHAPES = {192: [(1, 1), (5, 7), (3, 33), (9, 65)], 128: [(1, 1), (7, 31), (8, 32), (9, 33), (2, 70)], 96: [(1, 1), (7, 31), (8, 32), (9, 33), (2, 70)]}
ROW_BATCH_SHAPE = (5, 33)
T64_SHAPES = [(1, 1), (8, 32), (9, 33), (17, 70)]
T64_BUDGET_SHAPE = (41, 130)
RS_SHAPES = [(7, 1), (7, 33), (8, 32), (23, 65)]
RS2_CASES = [(8, 1, 0), (8, 30, 0), (9, 31, 0), (25, 61, 7), (33, 29, 4)]      # (H, W, cus)
KS_SHAPES = [(5, 7), (9, 33), (17, 70)]
TWO_LAYER = {"T64": (64, 17, 70), "RS": (64, 23, 65), "ROW": (128, 9, 33)}


def exact_cases():
    out = []
    for C, shapes in ROW_SHAPES.items():
        out += [("ROW", C, h, w, 1) for h, w in shapes + ([ROW_BATCH_SHAPE] if C != 192 else [])]
    for C in (64, 96):
        out += [("T64", C, h, w, 1) for h, w in T64_SHAPES + [T64_BUDGET_SHAPE]]
    out += [("RS", 64, h, w, 1) for h, w in RS_SHAPES]
    out += [("RS2", 64, h, w, 2) for h, w, _ in RS2_CASES]
    for C in (128, 96):
        out += [("KS", C, h, w, 1) for h, w in KS_SHAPES]
    out += [(k, c, h, w, 2) for k, (c, h, w) in TWO_LAYER.items()]
    return out


_CACHE = {}


def case_seed(C, H, W, n_layers):
    return [C, H, W, n_layers]


def cached_exact_case(C, H, W, n_layers=1):
    """exact_case() with the seed (C, H, W, n_layers), computed once per process and shared (do not modify the arrays)."""
    key = (C, H, W, n_layers)
    if key not in _CACHE:
        _CACHE[key] = exact_case(C, H, W, np.random.default_rng(case_seed(*key)), n_layers)
    return _CACHE[key]
