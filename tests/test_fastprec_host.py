"""Fast precision (include/rife_hip.h rife_hip_set_precision) without a GPU: the float64 reference of one layer on the exact inputs of tests/s16_ref.py, the
network model (tests/fastprec_ref.FastNet), the size of the effect on the end-to-end inputs of tests/test_gpu_fastprec.py, and the public surface (header,
exported symbols, Python argument checking, the command line's refusals)."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import deep_ref
import fastprec_ref as fp
import flowscale_ref
import s16_ref
from tools import gen_frames, ncnn_param
from torch_graph import TorchNet

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIFE_HIP = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")
CASES = [c for c in s16_ref.exact_cases() if c[0] != "KS"]
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None


# ---- 1. the exact cases -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_cases_hold_their_preconditions_and_differ_from_full_precision(case):
    _, C, H, W, n = case
    e = fp.fast_exact_case(C, H, W, n)                                       # asserts the preconditions on what it computes
    assert len(e["want"]) == len(e["full"]) == n and e["want"][0].shape == (C, H, W)
    share = float((e["want"][0] != e["full"][0]).mean())
    print("fast precision, %s: %.1f %% of the first-layer outputs differ from full precision" % (_ids(case), 100 * share))
    assert share >= 0.90
    # the layer itself: dropping lo from the skip as well, or keeping it in the taps, is another tensor
    hi, lo = s16_ref.split(e["x"])
    assert not np.array_equal(fp.fast_trunk_layer(hi, np.zeros_like(lo), e["w"][0], e["b"][0], 0.25), e["want"][0])
    assert np.array_equal(s16_ref.trunk_layer(hi.astype(np.float64) + lo.astype(np.float64), e["w"][0], e["b"][0], 0.25), e["full"][0])


def test_fast_layer_is_the_full_layer_where_lo_is_zero():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16, 5, 7)).astype(np.float16)
    w = (rng.standard_normal((16, 16, 3, 3)) / 12).astype(np.float16).astype(np.float32)
    b = rng.standard_normal(16).astype(np.float32)
    assert np.array_equal(fp.fast_trunk_layer(x, np.zeros_like(x), w, b, 0.2), s16_ref.trunk_layer(x.astype(np.float64), w, b, 0.2))


# ---- 2. FastNet -----------------------------------------------------------------------------------------------------------------------------------------

def _paths(d):
    return os.path.join(d, "flownet.param"), os.path.join(d, "flownet.bin")


def test_trunk_convolutions_are_found_structurally(modeldirs, tmp_path):
    stock = ncnn_param.parse(_paths(modeldirs["rife-v4.6"])[0])
    names = fp.trunk_convolutions(stock)
    assert len(names) == len(set(names)) == 32
    by_name = {l["name"]: l for l in stock}
    assert sorted(int(by_name[n]["params"][0]) for n in names) == [64] * 8 + [96] * 8 + [128] * 8 + [192] * 8
    scaled = flowscale_ref.scaled_modeldir(modeldirs["rife-v4.6"], tmp_path / "fs2")
    assert fp.trunk_convolutions(ncnn_param.parse(_paths(scaled)[0])) == names
    assert fp.trunk_convolutions(ncnn_param.parse(_paths(modeldirs["rife-v4"])[0])) == []
    with pytest.raises(ValueError):
        fp.FastNet(*_paths(modeldirs["rife-v4"]))


def test_fastnet_without_rounding_is_torchnet_bit_for_bit(modeldirs):
    a, b = gen_frames.smooth_pair(96, 64, 3)
    ins = {k: torch.from_numpy(v) for k, v in deep_ref.net_inputs(a, b, 0.4, 8).items()}
    blobs = ["flow0", "flow1", "flow2", "flow3", "out0"]
    want = TorchNet(*_paths(modeldirs["rife-v4.6"])).run(ins, blobs)
    got = fp.FastNet(*_paths(modeldirs["rife-v4.6"]), rounding=False).run(ins, blobs)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    fast = fp.FastNet(*_paths(modeldirs["rife-v4.6"])).run(ins, blobs)
    assert not torch.equal(fast[0], want[0])                                 # the rounding is really applied, from block 0 on


# ---- 3. the model of the effect on the end-to-end inputs of the GPU test ------------------------------------------------------------------------------------

@pytest.mark.parametrize("inp", fp.B1_INPUTS, ids=lambda i: i[0])
def test_model_of_the_effect_stays_within_one_code(modeldirs, tmp_path, inp):
    """A condition on the choice of inputs: the GPU test's bound of 2 codes is this 1 code plus the engine's own."""
    m = fp.model_effect(modeldirs["rife-v4.6"], inp, tmp_path / "fs2")
    print("fast precision model, %s: max %d codes (%.3f before quantisation), %.3f %% of the channels differ, max |d flow0..3| = %s" % (
        inp[0], m["max_codes"], m["float_codes"], 100 * m["share"], " ".join("%.2e" % f for f in m["flow"])))
    assert m["max_codes"] <= 1
    assert m["share"] > 0 and all(f > 0 for f in m["flow"])                  # the model is not the identity on this input


# ---- 4. the public surface ---------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_python_lists_the_calls():
    with open(os.path.join(ROOT, "include", "rife_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+rife_hip_set_precision\s*\(\s*rife_hip_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint\s+rife_hip_precision\s*\(\s*const\s+rife_hip_t\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"enum\s*\{\s*RIFE_HIP_PRECISION_FULL\s*=\s*0\s*,\s*RIFE_HIP_PRECISION_FAST\s*=\s*1\s*\}", header)
    assert (amd.PRECISION_FULL, amd.PRECISION_FAST) == (0, 1)
    assert "rife_hip_set_precision" in amd.C_ABI_SYMBOLS and "rife_hip_precision" in amd.C_ABI_SYMBOLS
    assert callable(getattr(amd.RIFE, "set_precision", None)) and isinstance(amd.RIFE.precision, property)
    with open(os.path.join(ROOT, "include", "rife_hip_test.h")) as f:
        test_header = f.read()
    assert re.search(r"\bint\s+rife_hip_op_trunk_prec\s*\([^;]*int\s+precision\s*\)\s*;", test_header)
    assert re.search(r"\bint\s+rife_hip_op_trunk\s*\([^;]*void\s*\*\s*const\s*\*\s*out_s16\s*\)\s*;", test_header)      # the old signature stays
    assert "rife_hip_op_trunk_prec" in amd.TEST_ABI_SYMBOLS
    with open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "rife.h")) as f:
        shim = f.read()
    assert re.search(r"\bint\s+set_precision\s*\(\s*int\s+\w+\s*\)\s*;", shim) and re.search(r"\bint\s+precision\s*\(\s*\)\s*const\s*;", shim)


def test_both_libraries_export_the_calls():
    for path, test_surface in ((amd.LIB_PATH, False), (amd.TEST_LIB_PATH, True)):
        L = ctypes.CDLL(path)
        assert hasattr(L, "rife_hip_set_precision") and hasattr(L, "rife_hip_precision"), path
        assert hasattr(L, "rife_hip_op_trunk_prec") == test_surface, path
    shim = ctypes.CDLL(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "librife.so"))
    assert hasattr(shim, "_ZN4RIFE13set_precisionEi") and hasattr(shim, "_ZNK4RIFE9precisionEv")


def _engineless():
    """A RIFE object without an engine: what the Python layer checks itself, and what the C calls answer for a null engine."""
    g = amd.RIFE.__new__(amd.RIFE)
    g._L = amd.lib(); g._h = None
    return g


@pytest.mark.parametrize("bad", ["FAST", "half", "", 2, -1, 1.0, True, None, b"fast"])
def test_python_refuses_anything_but_the_two_words_and_constants(bad):
    with pytest.raises(ValueError):
        _engineless().set_precision(bad)


def test_null_engine_is_einval_and_reads_full():
    g = _engineless()
    assert g.precision == amd.PRECISION_FULL
    for ok in ("full", "fast", amd.PRECISION_FULL, amd.PRECISION_FAST, np.int32(1)):
        with pytest.raises(amd.RifeError, match=r"\(-%d\)" % amd.EINVAL):
            g.set_precision(ok)
    L = amd.lib()
    assert L.rife_hip_set_precision(None, 7) == -amd.EINVAL and L.rife_hip_last_error()
    assert L.rife_hip_precision(None) == 0


def test_op_trunk_refuses_an_unknown_precision_and_conv_ks_without_a_device():
    L = amd.testlib()
    C, H, W = 128, 5, 33
    t = np.zeros(s16_ref.geom(C, H, W)[3], np.uint8)
    w = np.zeros((C, C, 3, 3), np.float32); b = np.zeros(C, np.float32); s = np.full(1, 0.2, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pi = (ctypes.c_void_p * 1)(t.ctypes.data); po = (ctypes.c_void_p * 1)(t.ctypes.data)
    assert L.rife_hip_op_trunk_prec(0, amd.TRUNK_ROW, C, H, W, 1, p(w), p(b), p(s), 0, 0, 1, pi, po, 2) == -amd.EINVAL
    assert b"precision" in L.rife_hip_last_error()
    assert L.rife_hip_op_trunk_prec(0, amd.TRUNK_KS, C, H, W, 1, p(w), p(b), p(s), 0, 0, 1, pi, po, amd.PRECISION_FAST) == -amd.ENOSYS
    assert b"conv_ks" in L.rife_hip_last_error()


# ---- 5. the command line -------------------------------------------------------------------------------------------------------------------------------------

def _pair(tmp_path):
    from PIL import Image
    a, b = gen_frames.smooth_pair(64, 48, 4)
    Image.fromarray(a).save(tmp_path / "a.png"); Image.fromarray(b).save(tmp_path / "b.png")
    return ["-0", str(tmp_path / "a.png"), "-1", str(tmp_path / "b.png")]


def test_cli_refusals_exit_255_and_write_nothing(modeldirs, tmp_path):
    assert os.path.exists(RIFE_HIP), "rife-hip is not built"
    base = _pair(tmp_path)
    for name, extra, word in (("bogus.png", ["-m", modeldirs["rife-v4.6"], "-p", "bogus"], "full or fast"),
                              ("v23.png", ["-m", modeldirs["rife-v2.3"], "-p", "fast"], "rife-v4.6 only"),
                              ("x.png", ["-m", modeldirs["rife-v4.6"], "-p", "fast", "-x"], "-x"),
                              ("z.png", ["-m", modeldirs["rife-v4.6"], "-p", "fast", "-z"], "-z")):
        r = subprocess.run([RIFE_HIP] + base + ["-o", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 255 and word in r.stderr and "precision" in r.stderr, (name, r.returncode, r.stderr)
        assert not os.path.exists(tmp_path / name)


def test_cli_accepts_p_full_and_lists_the_option(modeldirs, tmp_path):
    """-p full passes the argument checks: whatever ends the run on a box without a device, it is not the precision."""
    assert os.path.exists(RIFE_HIP), "rife-hip is not built"
    r = subprocess.run([RIFE_HIP] + _pair(tmp_path) + ["-o", str(tmp_path / "o.png"), "-m", modeldirs["rife-v4.6"], "-p", "full"], capture_output=True, text=True, timeout=120)
    assert "precision" not in r.stderr, r.stderr
    assert (r.returncode == 0 and os.path.exists(tmp_path / "o.png")) or "gpu device" in r.stderr, (r.returncode, r.stderr)
    h = subprocess.run([RIFE_HIP, "-h"], capture_output=True, text=True, timeout=120)
    assert re.search(r"^\s+-p precision\s+full \(default\) or fast", h.stderr, re.M)
