"""Fast precision (include/rife_hip.h rife_hip_set_precision) on the GPU.  tests/fastprec_ref.py is the reference; tests/test_fastprec_host.py pins it without a GPU.

A  single launches of the fast instantiations of conv_t64 / conv_rs / conv_rs2 / conv_row through op_trunk(..., fast=True): on the exact inputs of
   tests/s16_ref.py the returned tensor equals fast_exact_case()'s expectation byte for byte (between 91 % and 99 % of it differs from full precision, so a kernel
   that ignores the flag, or one that also drops lo from the skip, cannot pass); walking directions, CU budgets, batched launches; fast=False is
   rife_hip_op_trunk; dense Gaussian inputs against fast_trunk_layer with the bar of test_gpu_trunk_ops.py::test_dense_gaussian (the same arithmetic class:
   exact f16 x f16 products, fp32 sum order).
B  a fast engine end to end against the FULL-PRECISION oracle, a plain engine next to it:
   condition   no channel more than 2 codes from the oracle = 1 code for the model's rounding (tests/test_fastprec_host.py, same inputs) + the engine's own 1 code;
   measured    share of differing channels and max |flow_k - oracle| per stage, each <= 2 x the CPU model's value + the plain engine's own value on that input.
               Factor 2: after the first layers the GPU's and the model's f16 roundings decorrelate (a 1e-6 difference flips a rounding), so the GPU result is
               another draw of the same noise, not the model's bytes; twice the model covers the draw-to-draw spread of a maximum, a wrong kernel lands orders
               of magnitude higher;
   the mode is on: max |flow3(fast) - flow3(plain)| >= a quarter of the model's flow3 value (plain against plain sits near 1e-5);
   identities within fast mode byte for byte, the way back to full precision, refusals, the command line.
   Every figure is printed as a line "fastprec parity: ..." (profiles/fastprec/parity.txt is those lines of one run)."""
import ctypes
import gc
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import deep_ref
import fastprec_ref as fp
import flowscale_ref as fr
import planar_ref as pr
import s16_ref
import yuv_ref as yr
from oracle import pyoracle
from tools import gen_frames

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
tb = amd.test_build()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIFE_HIP = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")
KERNEL = {"T64": amd.TRUNK_T64, "RS": amd.TRUNK_RS, "RS2": amd.TRUNK_RS2, "ROW": amd.TRUNK_ROW}
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None


# ================================================================ A. single launches ================================================================

def _single_cases():
    """(kernel, C, H, W, flip, cus): the single-layer launches of tests/test_gpu_trunk_ops.py without conv_ks."""
    out = []
    for C, shapes in s16_ref.ROW_SHAPES.items():
        out += [("ROW", C, h, w, 0, 0) for h, w in shapes + ([s16_ref.ROW_BATCH_SHAPE] if C != 192 else [])]
    for C in (64, 96):
        out += [("T64", C, h, w, flip, 0) for h, w in s16_ref.T64_SHAPES for flip in (0, 1)]
        out += [("T64", C) + s16_ref.T64_BUDGET_SHAPE + (flip, 8) for flip in (0, 1)]
    out += [("RS", 64, h, w, flip, cus) for h, w in s16_ref.RS_SHAPES for flip in (0, 1) for cus in (0, 1, 3)]
    return out


SINGLE = _single_cases()


def _run(kernel, C, H, W, w, b, slope, x_packed, flip=0, cus=0, fast=True):
    return tb.op_trunk(KERNEL[kernel], C, H, W, w, b, slope, x_packed, s16_ref.poisoned(C, H, W), flip=flip, cus=cus, fast=fast)


def _assert_bytes(got, want_chw, C, H, W):
    want = s16_ref.pack(want_chw.astype(np.float32), H, W)
    ext = s16_ref.exterior_mask(C, H, W)
    assert not got[ext].any(), "%d exterior bytes are not zero" % np.count_nonzero(got[ext])
    if not np.array_equal(got, want):
        gv, wv = s16_ref.value(got, C, H, W), s16_ref.value(want, C, H, W)
        bad = np.argwhere(~((gv == wv) | (np.isnan(gv) & np.isnan(wv))))
        raise AssertionError("%d of %d interior elements differ (NaN = never written: %d); first (c, y, x) = %s got %r want %r" % (
            len(bad), gv.size, int(np.isnan(gv).sum()), bad[:1].tolist(), gv[tuple(bad[0])] if len(bad) else None, wv[tuple(bad[0])] if len(bad) else None))


def test_the_single_cases_cover_every_exact_case():
    want = {(k, C, H, W) for k, C, H, W, n in s16_ref.exact_cases() if k != "KS" and n == 1}
    assert {c[:4] for c in SINGLE} == want


@pytest.mark.parametrize("case", SINGLE, ids=_ids)
def test_exact_inputs_bytes(case):
    kernel, C, H, W, flip, cus = case
    e = fp.fast_exact_case(C, H, W, 1)
    got = _run(kernel, C, H, W, e["w"][0], e["b"][0], e["slope"], s16_ref.pack(e["x"], H, W), flip, cus)
    _assert_bytes(got, e["want"][0], C, H, W)


@pytest.mark.parametrize("kernel,flip", [(k, f) for k in ("T64", "RS", "ROW") for f in (0, 1)])
def test_two_layers_ping_pong(kernel, flip):
    C, H, W = s16_ref.TWO_LAYER[kernel]
    e = fp.fast_exact_case(C, H, W, 2)
    got = _run(kernel, C, H, W, e["w"], e["b"], e["slope"], s16_ref.pack(e["x"], H, W), flip)
    _assert_bytes(got, e["want"][1], C, H, W)


def _gauss(C, H, W):
    g = s16_ref.gauss_case(C, H, W, np.random.default_rng([C, H, W]))
    g["in"] = s16_ref.pack(g["x"].astype(np.float32), H, W)
    g["hi"], g["lo"] = s16_ref.unpack(g["in"], C, H, W)
    assert np.array_equal(g["hi"].astype(np.float64) + g["lo"].astype(np.float64), g["x"])
    return g


@pytest.mark.parametrize("H,W,cus", s16_ref.RS2_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("flip", [0, 1])
def test_rs2_two_layers_one_launch(H, W, cus, flip):
    """conv_rs2's fast form: the exact two-layer expectation byte for byte and the bytes of two fast conv_rs launches, on the exact inputs and on dense Gaussian
    ones with the model's slope (conv_rs's own fast form is held against the float64 reference in test_dense_gaussian)."""
    C = 64
    e = fp.fast_exact_case(C, H, W, 2)
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
    assert not np.array_equal(got, _run("RS2", C, H, W, w2, b2, 0.2, g["in"], flip, cus, fast=False))


@pytest.mark.parametrize("C,H,W,nb", [(128, 5, 33, 3), (96, 5, 33, 3), (192, 3, 33, 4), (128, 5, 33, 4)])
def test_batched_row_launch_equals_single_fast_calls(C, H, W, nb):
    e = fp.fast_exact_case(C, H, W, 1)
    rng = np.random.default_rng(nb)
    ins = [s16_ref.pack(e["x"], H, W)] + [s16_ref.pack((rng.standard_normal((C, H, W)) * 3).astype(np.float32), H, W) for _ in range(nb - 1)]
    args = (amd.TRUNK_ROW, C, H, W, e["w"][0], e["b"][0], e["slope"])
    got = tb.op_trunk(*args, ins, [s16_ref.poisoned(C, H, W) for _ in ins], fast=True)
    assert len(got) == nb
    _assert_bytes(got[0], e["want"][0], C, H, W)
    for k in range(nb):
        assert np.array_equal(got[k], tb.op_trunk(*args, ins[k], s16_ref.poisoned(C, H, W), fast=True)), k


@pytest.mark.parametrize("kernel,C,H,W,n", [("T64", 64, 9, 33, 1), ("T64", 96, 9, 33, 1), ("RS", 64, 23, 65, 1), ("RS2", 64, 25, 61, 2), ("ROW", 192, 3, 33, 1),
                                            ("ROW", 128, 9, 33, 1), ("ROW", 96, 9, 33, 1)])
def test_full_precision_through_the_new_entry_is_op_trunk(kernel, C, H, W, n):
    """rife_hip_op_trunk_prec(..., RIFE_HIP_PRECISION_FULL) against rife_hip_op_trunk itself, byte for byte; and those bytes are the full-precision expectation."""
    e = fp.fast_exact_case(C, H, W, n)
    xin = s16_ref.pack(e["x"], H, W)
    got = _run(kernel, C, H, W, e["w"] if n == 2 else e["w"][0], e["b"] if n == 2 else e["b"][0], e["slope"], xin, fast=False)
    _assert_bytes(got, e["full"][n - 1], C, H, W)
    L = amd.testlib()
    w = np.ascontiguousarray(e["w"][:n], np.float32); b = np.ascontiguousarray(e["b"][:n], np.float32); s = np.full(n, e["slope"], np.float32)
    old = s16_ref.poisoned(C, H, W)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pi = (ctypes.c_void_p * 1)(xin.ctypes.data); po = (ctypes.c_void_p * 1)(old.ctypes.data)
    assert L.rife_hip_op_trunk(0, KERNEL[kernel], C, H, W, n, p(w), p(b), p(s), 0, 0, 1, pi, po) == 0, L.rife_hip_last_error()
    assert np.array_equal(old, got)


@pytest.mark.parametrize("case", [("T64", 64, 17, 70, 1, 0), ("T64", 96, 17, 70, 0, 0), ("RS", 64, 23, 65, 1, 3), ("ROW", 192, 9, 65, 0, 0), ("ROW", 128, 9, 33, 0, 0),
                                  ("ROW", 96, 9, 33, 0, 0)], ids=_ids)
def test_dense_gaussian(case):
    kernel, C, H, W, flip, cus = case
    g = _gauss(C, H, W)
    want = fp.fast_trunk_layer(g["hi"], g["lo"], g["w"], g["b"], 0.2)
    raw = _run(kernel, C, H, W, g["w"], g["b"], 0.2, g["in"], flip, cus)
    assert not raw[s16_ref.exterior_mask(C, H, W)].any()
    err = np.abs(s16_ref.value(raw, C, H, W) - want)
    full = np.abs(s16_ref.trunk_layer(g["x"], g["w"], g["b"], 0.2) - want).max()
    print("fastprec (gauss) %s err.max / |want|.max = %.3e (full precision is %.3e away)" % (_ids(case), err.max() / np.abs(want).max(), full / np.abs(want).max()))
    assert err.max() <= 4e-6 * np.abs(want).max()


def test_conv_ks_has_no_fast_form():
    C, H, W = 128, 5, 7
    t = np.zeros(s16_ref.geom(C, H, W)[3], np.uint8)
    with pytest.raises(amd.RifeError, match=r"\(-%d\).*conv_ks" % amd.ENOSYS):
        tb.op_trunk(amd.TRUNK_KS, C, H, W, np.zeros((C, C, 3, 3), np.float32), np.zeros(C, np.float32), 0.2, t, t, fast=True)


# ================================================================ B. end to end ================================================================

_ENG = {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The module's shared engines (and their workspaces and streams) go when the module is done, like a module-scoped fixture's."""
    yield
    _ENG.clear()
    gc.collect()


def engine(modeldirs, fast, fscale=1, test=False):
    """One engine per (precision, flow scale, build), shared by the module."""
    key = (fast, fscale, test)
    if key not in _ENG:
        g = (tb if test else amd).RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
        if fscale != 1:
            g.set_flow_scale(fscale)
        if fast:
            assert g.precision == amd.PRECISION_FULL
            g.set_precision("fast")
        assert g.precision == (amd.PRECISION_FAST if fast else amd.PRECISION_FULL) and g.flow_scale == fscale
        _ENG[key] = g
    return _ENG[key]


@pytest.fixture(scope="module")
def oracles(modeldirs, tmp_path_factory):
    o1 = pyoracle.OracleRIFE(rife_v4=True); o1.load(modeldirs["rife-v4.6"])
    o2 = pyoracle.OracleRIFE(rife_v4=True); o2.load(fr.scaled_modeldir(modeldirs["rife-v4.6"], tmp_path_factory.mktemp("v46_fs2")))
    return {1: o1, 2: o2}


def _off(got, want):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d > 0).mean())


@pytest.mark.parametrize("inp", fp.B1_INPUTS, ids=lambda i: i[0])
def test_fast_engine_against_the_full_precision_oracle(modeldirs, oracles, tmp_path, inp):
    name, w, h, kind, seed, t, depth, fscale = inp
    a, b = fp.b1_frames(inp)
    ref = fr if fscale == 2 else deep_ref
    model = fp.model_effect(modeldirs["rife-v4.6"], inp, tmp_path / "fs2")
    want = ref.expected_frame(oracles[fscale], a, b, t, depth)
    fast = engine(modeldirs, True, fscale).process(a, b, t)
    plain = engine(modeldirs, False, fscale).process(a, b, t)
    assert fast.shape == want.shape and fast.dtype == want.dtype
    (fmax, fshare), (pmax, pshare) = _off(fast, want), _off(plain, want)
    ferr, perr, dfp = [], [], []
    for k in range(4):
        blob = ref.extract(oracles[fscale], a, b, t, depth, "flow%d" % k)
        ff = engine(modeldirs, True, fscale, test=True).v4_extract_flow(a, b, t, k)
        pf = engine(modeldirs, False, fscale, test=True).v4_extract_flow(a, b, t, k)
        assert ff.shape == pf.shape == blob.shape
        ferr.append(float(np.abs(ff - blob).max())); perr.append(float(np.abs(pf - blob).max())); dfp.append(float(np.abs(ff - pf).max()))
    print("fastprec parity: %-20s codes max fast %d plain %d model %d | differing channels fast %.4f %% plain %.4f %% model %.4f %%" % (
        name, fmax, pmax, model["max_codes"], 100 * fshare, 100 * pshare, 100 * model["share"]))
    for k in range(4):
        print("fastprec parity: %-20s flow%d max |gpu - oracle| fast %.3e plain %.3e | model |fast - full| %.3e | gpu |fast - plain| %.3e" % (
            name, k, ferr[k], perr[k], model["flow"][k], dfp[k]))
    assert pmax <= 1, "the plain engine left its own bound"
    assert fmax <= 2
    assert fshare <= 2 * model["share"] + pshare
    for k in range(4):
        assert ferr[k] <= 2 * model["flow"][k] + perr[k], k
    assert dfp[3] >= model["flow"][3] / 4, "fast precision is not in force"


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


@pytest.mark.parametrize("w,h", [(100, 60), (256, 192)])
def test_every_entry_point_gives_the_bytes_of_process(modeldirs, w, h):
    import torch
    g = engine(modeldirs, True)
    prs = [gen_frames.smooth_pair(w, h, 20 + i) for i in range(4)]
    ts = [0.5, 0.25, 0.7, 0.4]
    want = [g.process(p[0], p[1], t) for p, t in zip(prs, ts)]
    assert not np.array_equal(want[0], engine(modeldirs, False).process(prs[0][0], prs[0][1], ts[0]))
    # the _px call with the RGB8 format
    out = np.empty_like(prs[0][0])
    pa, pb = (np.ascontiguousarray(x) for x in prs[0])
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert g._L.rife_hip_process_px(g._h, vp(pa), vp(pb), w, h, ts[0], vp(out), amd.PIX_RGB8) == 0
    assert np.array_equal(out, want[0])
    # stream mode
    for p, t, wnt in zip(prs, ts, want):
        f0, f1 = g.upload(p[0]), g.upload(p[1])
        assert np.array_equal(g.process_frames(f0, f1, t), wnt)
        f0.release(); f1.release()
    # resident frames: the default stream, a caller's stream, a CU-masked stream of rife_hip_stream_create
    d0 = [_dev(p[0]) for p in prs]; d1 = [_dev(p[1]) for p in prs]
    part = g.stream_create(1, 4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, st.cuda_stream, part):
        outs = [torch.zeros_like(x) for x in d0]
        for i in range(4):
            g.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], outs[i].data_ptr(), stream)
        torch.cuda.synchronize()
        for i in range(4):
            assert np.array_equal(outs[i].cpu().numpy().reshape(h, w, 3), want[i]), (i, stream)
    g.stream_destroy(part)
    # the resident batch call, 1 .. 4 pairs (2 and more: the lockstep groups, one conv_row launch per layer for all pairs)
    for k in range(1, 5):
        outs = [torch.zeros_like(x) for x in d0[:k]]
        g.process_device_batch([x.data_ptr() for x in d0[:k]], [x.data_ptr() for x in d1[:k]], w, h, ts[:k], [o.data_ptr() for o in outs], st.cuda_stream)
        st.synchronize()
        for i in range(k):
            assert np.array_equal(outs[i].cpu().numpy().reshape(h, w, 3), want[i]), (k, i)
    # the host batch
    for o, wnt in zip(g.process_batch([p[0] for p in prs], [p[1] for p in prs], ts), want):
        assert np.array_equal(o, wnt)
    # row-padded planes: an image call
    pad = [np.full((h, w + 5, 3), 0x5a, np.uint8) for _ in range(3)]
    pad[0][:, :w] = prs[0][0]; pad[1][:, :w] = prs[0][1]
    g.process(pad[0][:, :w], pad[1][:, :w], ts[0], outimage=pad[2][:, :w])
    assert np.array_equal(pad[2][:, :w], want[0]) and (pad[2][:, w:] == 0x5a).all()


@pytest.mark.parametrize("w,h", [(100, 60), (256, 192)])
def test_nv12_and_planar_float_calls_are_the_packed_call_on_the_converted_frames(modeldirs, w, h):
    g = engine(modeldirs, True)
    NV12, PF = amd.PIX_NV12, amd.PIX_RGBPF
    c0, c1 = deep_ref.deep_pair(w, h, 61)
    y0, y1 = (yr.rgb10_to_yuv(c, NV12) for c in (c0, c1))
    got = g.process_yuv(y0, y1, w, h, 0.5, NV12)
    r0, r1 = (amd.pack_a2b10g10r10(yr.yuv_to_rgb10(y, w, h, NV12)) for y in (y0, y1))
    want = yr.rgb10_to_yuv(amd.unpack_a2b10g10r10(g.process(r0, r1, 0.5)), NV12)
    assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1))
    a, b = pr.from_rgb10(c0, PF), pr.from_rgb10(c1, PF)
    got = np.stack(g.process_planes(a, b, 0.4, PF))
    mid = g.process(amd.pack_a2b10g10r10(pr.to_rgb10(a, PF)), amd.pack_a2b10g10r10(pr.to_rgb10(b, PF)), 0.4)
    want = pr.from_rgb10(amd.unpack_a2b10g10r10(mid), PF)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    plain = engine(modeldirs, False).process(amd.pack_a2b10g10r10(pr.to_rgb10(a, PF)), amd.pack_a2b10g10r10(pr.to_rgb10(b, PF)), 0.4)
    assert not np.array_equal(mid, plain)


@pytest.mark.parametrize("w,h", [(100, 60), (256, 192)])
def test_reentrant_repeatable_and_timestep_0_1(modeldirs, w, h):
    g = engine(modeldirs, True)
    a, b = gen_frames.smooth_pair(w, h, 9)
    first = g.process(a, b, 0.5)
    assert np.array_equal(g.process(a, b, 0.5), first)
    outs = [None] * 4

    def work(i):
        outs[i] = g.process(a, b, 0.5)
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for x in th: x.start()
    for x in th: x.join()
    assert all(np.array_equal(o, first) for o in outs)
    assert np.array_equal(g.process(a, b, 0.0), a) and np.array_equal(g.process(a, b, 1.0), b)


def test_the_way_back_to_full_precision(modeldirs):
    """After set_precision("full") the bytes are a never-switched engine's; the same after fast -> flow scale 2 -> flow scale 1 -> full.  The setters compose in
    either order."""
    w, h = 256, 192
    a, b = gen_frames.smooth_pair(w, h, 9)
    base = engine(modeldirs, False).process(a, b, 0.5)
    fast = engine(modeldirs, True).process(a, b, 0.5)
    fast2 = engine(modeldirs, True, 2).process(a, b, 0.5)                     # set_flow_scale(2), then set_precision("fast")
    plain2 = engine(modeldirs, False, 2).process(a, b, 0.5)
    assert not np.array_equal(fast, base) and not np.array_equal(fast2, plain2)
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    assert np.array_equal(g.process(a, b, 0.5), base)
    g.set_precision(amd.PRECISION_FAST)
    assert g.precision == amd.PRECISION_FAST and np.array_equal(g.process(a, b, 0.5), fast)
    g.set_precision("full")
    assert g.precision == amd.PRECISION_FULL and np.array_equal(g.process(a, b, 0.5), base)
    g.set_precision("fast")
    g.set_flow_scale(2)                                                      # the other order
    assert (g.precision, g.flow_scale) == (amd.PRECISION_FAST, 2) and np.array_equal(g.process(a, b, 0.5), fast2)
    g.set_flow_scale(1)
    assert np.array_equal(g.process(a, b, 0.5), fast)
    g.set_precision("full")
    assert (g.precision, g.flow_scale) == (amd.PRECISION_FULL, 1) and np.array_equal(g.process(a, b, 0.5), base)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------

def _set(g, n):
    rc = g._L.rife_hip_set_precision(g._h, n)
    return rc, g._L.rife_hip_last_error().decode()


def test_before_load_and_bad_values_are_einval(modeldirs):
    g = amd.RIFE(0, rife_v4=True)
    for n in (amd.PRECISION_FAST, amd.PRECISION_FULL):
        rc, msg = _set(g, n)
        assert rc == -amd.EINVAL and "before load" in msg
    assert g.precision == amd.PRECISION_FULL
    g.load(modeldirs["rife-v4.6"])
    for n in (2, -1, 7):
        rc, msg = _set(g, n)
        assert rc == -amd.EINVAL and "precision" in msg
    with pytest.raises(ValueError):
        g.set_precision("half")
    assert g.precision == amd.PRECISION_FULL
    a, b = gen_frames.smooth_pair(64, 48, 2)
    assert np.array_equal(g.process(a, b, 0.5), engine(modeldirs, False).process(a, b, 0.5))


@pytest.mark.parametrize("fam,kw,word", [("rife-v4", dict(rife_v4=True), "rife-v4 (4.0)"), ("rife-v2.3", dict(rife_v2=True), "rife-v2"),
                                         ("rife-v4.6", dict(rife_v4=True, tta_mode=True), "-x"), ("rife-v4.6", dict(rife_v4=True, tta_temporal_mode=True), "-z")])
def test_other_families_and_modes_are_enosys(modeldirs, fam, kw, word):
    g = amd.RIFE(0, **kw); g.load(modeldirs[fam])
    a, b = gen_frames.smooth_pair(64, 64, 2)
    before = g.process(a, b, 0.5)
    rc, msg = _set(g, amd.PRECISION_FAST)
    assert rc == -amd.ENOSYS and word in msg and "fast precision" in msg, msg
    with pytest.raises(amd.RifeError, match=r"\(-%d\)" % amd.ENOSYS):
        g.set_precision("fast")
    assert g.precision == amd.PRECISION_FULL and _set(g, amd.PRECISION_FULL)[0] == 0
    assert np.array_equal(g.process(a, b, 0.5), before)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------

def test_cli_p_fast_writes_the_fast_frame(modeldirs, tmp_path):
    from PIL import Image
    assert os.path.exists(RIFE_HIP), "rife-hip is not built"
    a, b = gen_frames.smooth_pair(100, 60, 4)
    Image.fromarray(a).save(tmp_path / "a.png"); Image.fromarray(b).save(tmp_path / "b.png")
    base = [RIFE_HIP, "-0", str(tmp_path / "a.png"), "-1", str(tmp_path / "b.png"), "-m", modeldirs["rife-v4.6"]]
    want = {"fast": engine(modeldirs, True).process(a, b, 0.5), "full": engine(modeldirs, False).process(a, b, 0.5)}
    assert not np.array_equal(want["fast"], want["full"])
    for word in ("fast", "full"):
        r = subprocess.run(base + ["-o", str(tmp_path / (word + ".png")), "-p", word], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.asarray(Image.open(tmp_path / (word + ".png")).convert("RGB")), want[word]), word
    r = subprocess.run(base[:-1] + [modeldirs["rife-v4"], "-o", str(tmp_path / "v40.png"), "-p", "fast"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "rife-v4 (4.0)" in r.stderr and not os.path.exists(tmp_path / "v40.png"), (r.returncode, r.stderr)
