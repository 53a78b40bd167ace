"""The S16 trunk kernels ONE launch at a time against a float64 reference (GPU box only): conv_t64_kernel<3, 2> / <2, 3>, conv_rs_kernel, conv_rs2_kernel,
conv_row_kernel<192, 1, 0> / <128, 2, 1> / <96, 2, 2> and conv_ks_kernel through rife_hip_op_trunk, i.e. the product's layer upload and the product's launchers
(grid size, work split, direction flags, LDS attributes are theirs) on raw S16 tensors.  tests/s16_ref.py is the layout and the reference.

Per case:
  (a) exact inputs, BYTES: on the inputs of s16_ref.exact_case() the fp32 accumulators are exact in any summation order, so the whole returned tensor must equal
      pack(reference) byte for byte.  The output buffer goes in with a NaN interior and a zero exterior: every interior element must have been written, every
      exterior byte (borders, columns W .. pitch, rows H .. rows: the next layer's zero padding) must still be zero.
  (b) model slope: the same inputs with slope 0.2; |got - want| <= 2^-21 |want| + 2^-24 on hi + lo.  Derived: the accumulator is exact, what remains is the slope
      multiply (2^-24 relative), the output split (2^-22 relative) and an f16-subnormal lo (2^-25 absolute).
  (c) dense Gaussian inputs over six decades of magnitude, the per-tile kernel's own bar (tests/test_gpu_kernels.py): err.max() <= 4e-6 |want|.max().
      Measured per kernel: profiles/trunk_ops/README.md.
A small CU budget makes a small tensor walk the way a 4K tensor walks on the whole chip: ranges that cross strips (conv_rs), several tiles per workgroup
(conv_t64), segment seams where layer A's rows are recomputed (conv_rs2), multi-row ranges (conv_ks)."""
import importlib

import numpy as np
import pytest

import s16_ref

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()      # librife_hip_test.so: parity taps, single-kernel entry points and kernel-selection switches (include/rife_hip_test.h)

KERNEL = {"T64": amd.TRUNK_T64, "RS": amd.TRUNK_RS, "RS2": amd.TRUNK_RS2, "ROW": amd.TRUNK_ROW, "KS": amd.TRUNK_KS}


def _single_cases():
    """(kernel, C, H, W, flip, cus) of the single-layer, single-tensor launches."""
    out = []
    for C, shapes in s16_ref.ROW_SHAPES.items():
        out += [("ROW", C, h, w, 0, 0) for h, w in shapes]
    for C in (64, 96):
        out += [("T64", C, h, w, flip, 0) for h, w in s16_ref.T64_SHAPES for flip in (0, 1)]
        out += [("T64", C) + s16_ref.T64_BUDGET_SHAPE + (flip, 8) for flip in (0, 1)]      # 30 tiles on 16 / 8 workgroups (launch_t64's floor of 8 CUs)
    out += [("RS", 64, h, w, flip, cus) for h, w in s16_ref.RS_SHAPES for flip in (0, 1) for cus in (0, 1, 3)]
    for C in (128, 96):
        out += [("KS", C, h, w, 0, cus) for h, w in s16_ref.KS_SHAPES for cus in (0, 4)]
    return out


SINGLE = _single_cases()
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None
_REF = {}


def _gauss(C, H, W):
    key = ("gauss", C, H, W)
    if key not in _REF:
        g = s16_ref.gauss_case(C, H, W, np.random.default_rng([C, H, W]))
        g["in"] = s16_ref.pack(g["x"].astype(np.float32), H, W)
        assert np.array_equal(s16_ref.value(g["in"], C, H, W), g["x"])      # the reference sees the tensor the kernel sees
        g["want"] = s16_ref.trunk_layer(g["x"], g["w"], g["b"], 0.2)
        _REF[key] = g
    return _REF[key]


def _model_slope_want(C, H, W):
    key = ("b", C, H, W)
    if key not in _REF:
        e = s16_ref.cached_exact_case(C, H, W, 1)
        _REF[key] = s16_ref.trunk_layer(e["x"], e["w"][0], e["b"][0], 0.2)
    return _REF[key]


def _run(kernel, C, H, W, w, b, slope, x_packed, flip=0, cus=0):
    return amd.op_trunk(KERNEL[kernel], C, H, W, w, b, slope, x_packed, s16_ref.poisoned(C, H, W), flip=flip, cus=cus)


def _assert_bytes(got, want_chw, C, H, W):
    want = s16_ref.pack(want_chw.astype(np.float32), H, W)
    ext = s16_ref.exterior_mask(C, H, W)
    assert not got[ext].any(), "%d exterior bytes are not zero" % np.count_nonzero(got[ext])
    if not np.array_equal(got, want):
        gv, wv = s16_ref.value(got, C, H, W), s16_ref.value(want, C, H, W)
        bad = np.argwhere(~((gv == wv) | (np.isnan(gv) & np.isnan(wv))))
        raise AssertionError("%d of %d interior elements differ (NaN = never written: %d); first (c, y, x) = %s got %r want %r" % (
            len(bad), gv.size, int(np.isnan(gv).sum()), bad[:1].tolist(), gv[tuple(bad[0])] if len(bad) else None, wv[tuple(bad[0])] if len(bad) else None))


@pytest.mark.parametrize("case", SINGLE, ids=_ids)
def test_exact_inputs_bytes(case):
    kernel, C, H, W, flip, cus = case
    e = s16_ref.cached_exact_case(C, H, W, 1)
    got = _run(kernel, C, H, W, e["w"][0], e["b"][0], e["slope"], s16_ref.pack(e["x"], H, W), flip, cus)
    _assert_bytes(got, e["want"][0], C, H, W)


@pytest.mark.parametrize("case", SINGLE, ids=_ids)
def test_model_slope(case):
    kernel, C, H, W, flip, cus = case
    e = s16_ref.cached_exact_case(C, H, W, 1)
    want = _model_slope_want(C, H, W)
    got = s16_ref.value(_run(kernel, C, H, W, e["w"][0], e["b"][0], 0.2, s16_ref.pack(e["x"], H, W), flip, cus), C, H, W)
    err = np.abs(got - want)
    print("trunk_ops (b) %s max err / bar = %.3f" % (_ids(case), (err / (2.0 ** -21 * np.abs(want) + 2.0 ** -24)).max()))
    assert np.all(err <= 2.0 ** -21 * np.abs(want) + 2.0 ** -24)


@pytest.mark.parametrize("case", SINGLE, ids=_ids)
def test_dense_gaussian(case):
    kernel, C, H, W, flip, cus = case
    g = _gauss(C, H, W)
    raw = _run(kernel, C, H, W, g["w"], g["b"], 0.2, g["in"], flip, cus)
    assert not raw[s16_ref.exterior_mask(C, H, W)].any()
    err = np.abs(s16_ref.value(raw, C, H, W) - g["want"])
    print("trunk_ops (c) %s err.max / |want|.max = %.3e" % (_ids(case), err.max() / np.abs(g["want"]).max()))
    assert err.max() <= 4e-6 * np.abs(g["want"]).max()      # the per-tile kernel's bar for the same products (it measures 1.1e-6)


@pytest.mark.parametrize("kernel,flip", [(k, f) for k in ("T64", "RS", "ROW") for f in (0, 1)])
def test_two_layers_ping_pong(kernel, flip):
    """in -> out -> in with alternating direction: the second launch reads what the first wrote, exterior included, and writes over the input."""
    C, H, W = s16_ref.TWO_LAYER[kernel]
    e = s16_ref.cached_exact_case(C, H, W, 2)
    got = _run(kernel, C, H, W, e["w"], e["b"], e["slope"], s16_ref.pack(e["x"], H, W), flip)
    _assert_bytes(got, e["want"][1], C, H, W)


@pytest.mark.parametrize("H,W,cus", s16_ref.RS2_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("flip", [0, 1])
def test_rs2_two_layers_one_launch(H, W, cus, flip):
    """conv_rs2: the exact two-layer reference byte for byte, and the bytes of two conv_rs launches - on the exact inputs and on dense Gaussian ones with the
    model's slope.  25 x 61 on 7 CUs: 3 strips x 2 segments of 12 / 13 rows; 33 x 29 on 4 CUs: 1 strip x 4 segments of 8, 8, 8, 9 rows (rs2_plan)."""
    C = 64
    e = s16_ref.cached_exact_case(C, H, W, 2)
    xin = s16_ref.pack(e["x"], H, W)
    got = _run("RS2", C, H, W, e["w"], e["b"], e["slope"], xin, flip, cus)
    _assert_bytes(got, e["want"][1], C, H, W)
    assert np.array_equal(got, _run("RS", C, H, W, e["w"], e["b"], e["slope"], xin, flip))
    g = _gauss(C, H, W)
    w2 = np.stack([g["w"], g["w"][::-1, ::-1].copy()])
    b2 = np.stack([g["b"], -g["b"]])
    got = _run("RS2", C, H, W, w2, b2, 0.2, g["in"], flip, cus)
    assert not got[s16_ref.exterior_mask(C, H, W)].any()
    assert np.array_equal(got, _run("RS", C, H, W, w2, b2, 0.2, g["in"], flip))


@pytest.mark.parametrize("kernel,C,H,W,cus,nb", [("ROW", 128, 5, 33, 0, 3), ("ROW", 96, 5, 33, 0, 3), ("ROW", 192, 3, 33, 0, 4)] +
                         [("KS", C, h, w, cus, 2) for C in (128, 96) for h, w in s16_ref.KS_SHAPES for cus in (0, 4)])
def test_batched_launch_equals_single_calls(kernel, C, H, W, cus, nb):
    """gridDim.y = nb tensors in one launch: every tensor gets the bytes of its own single call (and tensor 0 the exact reference's)."""
    e = s16_ref.cached_exact_case(C, H, W, 1)
    rng = np.random.default_rng(nb)
    ins = [s16_ref.pack(e["x"], H, W)] + [s16_ref.pack((rng.standard_normal((C, H, W)) * 3).astype(np.float32), H, W) for _ in range(nb - 1)]
    args = (KERNEL[kernel], C, H, W, e["w"][0], e["b"][0], e["slope"])
    got = amd.op_trunk(*args, ins, [s16_ref.poisoned(C, H, W) for _ in ins], cus=cus)
    assert len(got) == nb
    _assert_bytes(got[0], e["want"][0], C, H, W)
    for k in range(nb):
        assert np.array_equal(got[k], amd.op_trunk(*args, ins[k], s16_ref.poisoned(C, H, W), cus=cus)), k


@pytest.mark.parametrize("kernel,C,H,W,n_layers,nb,what", [
    ("RS", 64, 6, 33, 1, 1, "conv_rs needs at least 7 rows"),
    ("RS2", 64, 7, 30, 2, 1, "conv_rs2 does not apply"),
    ("RS2", 64, 16, 30, 1, 1, "two layers"),
    ("T64", 128, 8, 32, 1, 1, "64 and 96"),
    ("RS", 96, 8, 32, 1, 1, "64 channels"),
    ("ROW", 64, 8, 32, 1, 1, "96, 128 and 192"),
    ("KS", 192, 8, 32, 1, 1, "96 and 128"),
    ("ROW", 128, 5, 33, 1, 5, "one to four"),
    ("T64", 64, 8, 32, 1, 2, "batched"),
])
def test_refused_shapes_are_einval(kernel, C, H, W, n_layers, nb, what):
    """What a launcher refuses comes back as -RIFE_HIP_EINVAL from the checks in front of the upload: nothing is launched."""
    w = np.zeros((n_layers, C, C, 3, 3), np.float32)
    t = [np.zeros(s16_ref.geom(C, H, W)[3], np.uint8) for _ in range(nb)]
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*%s" % (amd.EINVAL, what)):
        amd.op_trunk(KERNEL[kernel], C, H, W, w, np.zeros((n_layers, C), np.float32), 0.2, t if nb > 1 else t[0], t if nb > 1 else t[0])


def test_weights_that_are_not_fp16_are_einval():
    C, H, W = 64, 8, 32
    w = np.zeros((C, C, 3, 3), np.float32)
    w[5, 7, 1, 2] = 0.1
    t = np.zeros(s16_ref.geom(C, H, W)[3], np.uint8)
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*exactly fp16" % amd.EINVAL):
        amd.op_trunk(amd.TRUNK_T64, C, H, W, w, np.zeros(C, np.float32), 0.2, t, t)
