"""Motion export (include/rife_hip.h rife_hip_motion_t), the part that needs no device: rife_hip_motion_check through ctypes on the PRODUCT library, every rule by
name; the argument checks of the three motion calls, which come before "no device"; the Python surface; tests/sanitize/motion_check_main.cpp, a program of its own
under ASan + UBSan over csrc/motion_check.h; and the conditions the GPU tests rest on, checked against the CPU oracle ALONE - a frame rebuilt with
motion_ref.reconstruct() from the oracle's flow and mask blobs equals the oracle's own quantised out0 outside the boundary set, and that set stays under the cap."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as mr
import tail_ref as tr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 33, 47


def check(m, w=W, h=H):
    L = amd.lib()
    rc = L.rife_hip_motion_check(ctypes.byref(m) if m is not None else None, w, h)
    return rc, L.rife_hip_last_error().decode()


def refused(m, word, w=W, h=H):
    rc, msg = check(m, w, h)
    assert rc == -amd.EINVAL and word in msg, (rc, msg)


def good(fmt, w=W, h=H, pad=48):
    """A descriptor over two host buffers with `pad` bytes of row padding each (numpy allocations are 16-byte aligned)."""
    es = 2 if fmt == amd.MOTION_F16 else 4
    fb = np.zeros((h, w * 4 * es + pad), np.uint8); mb = np.zeros((h, w * es + pad), np.uint8)
    assert fb.ctypes.data % 16 == 0 and mb.ctypes.data % 16 == 0
    m = amd.motion_desc(fb.ctypes.data, mb.ctypes.data, fmt, fb.strides[0], mb.strides[0])
    m._keep = (fb, mb)
    return m, es


def test_header_numbers_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    assert re.search(r"#define RIFE_HIP_MOTION_F32 0\b", hdr) and re.search(r"#define RIFE_HIP_MOTION_F16 1\b", hdr)
    assert (amd.MOTION_F32, amd.MOTION_F16) == (mr.MOTION_F32, mr.MOTION_F16) == (0, 1)
    for s in ("rife_hip_motion_check", "rife_hip_process_motion", "rife_hip_process_device_motion", "rife_hip_process_frames_motion"):
        assert s in amd.C_ABI_SYMBOLS and hasattr(amd.lib(), s)
    assert "rife_hip_op_tail_motion" in amd.TEST_ABI_SYMBOLS
    assert ctypes.sizeof(amd.rife_hip_motion) == 40      # two pointers, two size_t, an int and its padding: the struct of the header on this ABI


@pytest.mark.parametrize("fmt", [mr.MOTION_F32, mr.MOTION_F16], ids=["f32", "f16"])
def test_motion_check_rules(fmt):
    m, es = good(fmt)
    assert check(m) == (0, check(m)[1])
    px = 4 * es
    b, _ = good(fmt); b.flow = None; b.flow_pitch = 0; assert check(b)[0] == 0                      # flow not wanted
    b, _ = good(fmt); b.mask = None; b.mask_pitch = 0; assert check(b)[0] == 0                      # mask not wanted
    b, _ = good(fmt); b.flow = None; b.mask = None; refused(b, "both NULL")
    b, _ = good(fmt); b.format = 2; refused(b, "unknown motion format")
    b, _ = good(fmt); b.format = -1; refused(b, "unknown motion format")
    b, _ = good(fmt); b.flow_pitch = W * px - px; refused(b, "flow: the pitch (%d) is smaller than the row bytes (%d)" % (W * px - px, W * px))
    b, _ = good(fmt); b.mask_pitch = W * es - es; refused(b, "mask: the pitch (%d) is smaller than the row bytes (%d)" % (W * es - es, W * es))
    b, _ = good(fmt); b.flow_pitch += es; refused(b, "flow: the pitch is not a multiple of %d bytes" % px)
    b, _ = good(fmt); b.mask_pitch += 1; refused(b, "mask: the pitch is not a multiple of %d bytes" % es)
    b, _ = good(fmt); b.flow += es; refused(b, "flow: the pointer is not aligned to %d bytes" % px)
    b, _ = good(fmt); b.mask += 1; refused(b, "mask: the pointer is not aligned to %d bytes" % es)
    refused(m, "bad frame size", w=0)
    refused(m, "bad frame size", h=-1)
    refused(None, "null motion descriptor")
    # a tight descriptor is fine too
    t = amd.motion_desc(m.flow, m.mask, fmt, W * px, W * es)
    assert check(t)[0] == 0


@pytest.mark.parametrize("fmt", [mr.MOTION_F32, mr.MOTION_F16], ids=["f32", "f16"])
def test_the_4_gb_bound(fmt):
    """h * pitch < 2^32: the kernels address the buffers with 32-bit byte offsets, like the frame."""
    m, es = good(fmt)
    px = 4 * es
    under = (2 ** 32 - 1) // H // px * px
    over = under + px
    assert under * H < 2 ** 32 <= over * H
    b = amd.motion_desc(m.flow, m.mask, fmt, under, m.mask_pitch); assert check(b)[0] == 0
    b = amd.motion_desc(m.flow, m.mask, fmt, over, m.mask_pitch); refused(b, "flow: h * pitch reaches 2^32")
    munder = (2 ** 32 - 1) // H // es * es
    b = amd.motion_desc(m.flow, m.mask, fmt, m.flow_pitch, munder); assert check(b)[0] == 0
    b = amd.motion_desc(m.flow, m.mask, fmt, m.flow_pitch, munder + es); refused(b, "mask: h * pitch reaches 2^32")
    b = amd.motion_desc(m.flow, m.mask, fmt, 2 ** 32, m.mask_pitch); refused(b, "flow: h * pitch reaches 2^32", h=1)


def test_argument_checks_come_before_the_device():
    """-EINVAL for every argument fault of the three calls, with or without a device (no engine is needed to get there); a sound call on a box without a
    device then gets -ENODEV, on a box with one the null engine is the next -EINVAL."""
    L = amd.lib()
    m, _ = good(mr.MOTION_F32)
    a = np.zeros((H, W, 3), np.uint8); o = np.zeros_like(a)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    bad, _ = good(mr.MOTION_F32); bad.flow_pitch = 8
    nothing = amd.motion_desc(None, None, mr.MOTION_F32)
    for call in (lambda mo, px=amd.PIX_RGB8, i0=p(a), w=W: L.rife_hip_process_motion(None, i0, p(a), w, H, 0.5, p(o), px, mo),
                 lambda mo, px=amd.PIX_RGB8, i0=p(a), w=W: L.rife_hip_process_device_motion(None, i0, p(a), w, H, 0.5, p(o), px, mo, None)):
        assert call(ctypes.byref(bad)) == -amd.EINVAL and "flow: the pitch" in L.rife_hip_last_error().decode()
        assert call(ctypes.byref(nothing)) == -amd.EINVAL and "both NULL" in L.rife_hip_last_error().decode()
        assert call(None) == -amd.EINVAL and "null motion descriptor" in L.rife_hip_last_error().decode()
        assert call(ctypes.byref(m), px=3) == -amd.EINVAL and "unknown pixel format" in L.rife_hip_last_error().decode()
        assert call(ctypes.byref(m), i0=None) == -amd.EINVAL and "null pointer" in L.rife_hip_last_error().decode()
        assert call(ctypes.byref(m), w=0) == -amd.EINVAL
        rc = call(ctypes.byref(m))
        assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL), (rc, L.rife_hip_last_error().decode())      # -RIFE_HIP_ENODEV / "null engine"
    assert L.rife_hip_process_frames_motion(None, None, None, 0.5, p(o), None) == -amd.EINVAL and "null motion descriptor" in L.rife_hip_last_error().decode()
    assert L.rife_hip_process_frames_motion(None, None, None, 0.5, p(o), ctypes.byref(m)) == -amd.EINVAL and "null frame pointer" in L.rife_hip_last_error().decode()


def test_python_surface_refuses_before_any_library_call():
    class NoEngine(amd.RIFE):
        def __init__(self):      # no device needed: the checks below never reach the library
            self._L, self._h = None, None
    r = NoEngine()
    a = np.zeros((H, W, 3), np.uint8)
    with pytest.raises(ValueError, match="np.float32 or np.float16"):
        r.process_motion(a, a, 0.5, dtype=np.float64)
    with pytest.raises(ValueError, match="both unwanted"):
        r.process_motion(a, a, 0.5, flow=False, mask=False)
    with pytest.raises(ValueError, match="flow must be a writable float32 array of shape"):
        r.process_motion(a, a, 0.5, flow=np.zeros((H, W, 4), np.float16))
    with pytest.raises(ValueError, match="mask must be"):
        r.process_motion(a, a, 0.5, mask=np.zeros((H, W + 1), np.float32))
    # row-padded arrays and views are described in place, without a copy
    big = np.zeros((H, W + 5, 4), np.float16); mk = np.zeros((H + 2, W + 3), np.float16)
    d, f, m = amd._motion_host(W, H, np.float16, big[:, :W], mk[1:H + 1, 2:W + 2])
    assert d.flow == big.ctypes.data and d.flow_pitch == (W + 5) * 8 and d.mask == mk.ctypes.data + (W + 3) * 2 + 4 and d.mask_pitch == (W + 3) * 2 and d.format == 1
    amd.motion_check(d, W, H)
    d, f, m = amd._motion_host(W, H, np.float32, None, False)
    assert f.shape == (H, W, 4) and f.dtype == np.float32 and m is None and not d.mask
    del r._L, r._h


def test_half_rounding_and_the_admissible_halves():
    """numpy's float16 cast is round to nearest even (ties: 1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9), and mask_half_ok admits the RNE half of the reference and
    of its neighbours within 2^-20 - one half, or two where the interval straddles a rounding boundary - and nothing else."""
    assert mr.half(np.float32(1 + 2.0 ** -11)) == np.float16(1) and mr.half(np.float32(1 + 3 * 2.0 ** -11)) == np.float16(1 + 2.0 ** -9)
    want = np.array([0.5, 0.25 + 2.0 ** -13, 0.7310585786300049])      # exact, on a boundary of the binade [0.25, 0.5) (step 2^-12), generic
    assert mr.mask_half_ok(want.astype(np.float16), want).all()
    assert mr.mask_half_ok(np.array([0.25, 0.25 + 2.0 ** -12], np.float16), want[1]).all()      # both neighbours of the boundary
    up = np.nextafter(want.astype(np.float16), np.float16(2)); dn = np.nextafter(want.astype(np.float16), np.float16(-2))
    assert not mr.mask_half_ok(np.array([up[0], up[2]]), want[[0, 2]]).any() and not mr.mask_half_ok(np.array([dn[0], dn[2]]), want[[0, 2]]).any()


def test_expected_is_exact_for_the_grid_cases():
    """flow = F + d of a planted case is on the 2^-10 grid and exact in fp32: the byte-for-byte bar is derived, not measured."""
    for w, h in [(1, 1), (100, 60)]:
        c = tr.cached("planted", w, h, 8)
        flow, mask = mr.expected(c, w, h)
        assert flow.shape == (h, w, 4) and mask.shape == (h, w)
        assert np.array_equal(flow * 2 ** tr.G, np.rint(flow * 2 ** tr.G)) and np.array_equal(flow.astype(np.float32).astype(np.float64), flow)
        f32 = c["F"][:h, :w] + np.moveaxis(c["d"][:4].astype(np.float32), 0, -1)[:h, :w]      # the kernels' fp32 add
        assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), flow)
        # the frame tail_ref expects IS the frame rebuilt from the expected motion
        val, amax = mr.reconstruct(flow, mask, c["p0"], c["p1"], 8)
        assert np.allclose(val, c["ref"]["val"], rtol=0, atol=1e-9) and np.array_equal(amax, c["ref"]["amax"])


def test_blobs_are_found_structurally(modeldirs, tmp_path):
    import flowscale_ref
    from conftest import REFERENCE
    stock = os.path.join(REFERENCE, "models", "rife-v4.6", "flownet.param")
    if os.path.exists(stock):
        assert mr.motion_blobs(open(stock).read()) == ("327", "332")      # the stock graph's names, where the stock graph is at hand
    text = open(os.path.join(modeldirs["rife-v4.6"], "flownet.param")).read()
    f1, m1 = mr.motion_blobs(text)
    text2 = open(os.path.join(flowscale_ref.scaled_modeldir(modeldirs["rife-v4.6"], tmp_path / "s2"), "flownet.param")).read()
    f2, m2 = mr.motion_blobs(text2)
    for t, f, m in ((text, f1, m1), (text2, f2, m2)):
        lines = [l.split() for l in t.splitlines()]
        assert sum(1 for l in lines if l and l[0] == "Sigmoid" and l[-1] == m) == 1                       # the mask is the Sigmoid's output
        prod = [l for l in lines if len(l) > 4 and f in l[4 + int(l[2]):4 + int(l[2]) + int(l[3])]]
        assert len(prod) == 1 and prod[0][0] in ("BinaryOp", "Eltwise"), prod                                # the flow is the sum that closes block 3's update
    assert m2 == m1      # the rewrite keeps the tail's names; its sum is an Eltwise with coefficients (1, 2)


@pytest.mark.parametrize("name", sorted(mr.E2E))
def test_oracle_frame_is_rebuilt_from_the_oracle_motion(name, modeldirs, tmp_path_factory):
    """The reference alone: reconstruct() from the oracle's flow and mask blobs and the input codes gives the oracle's quantised out0 outside the boundary set
    tau = 2^-6 amax, and the set stays under tail_ref.CAP - the condition item 3 of tests/test_gpu_motion.py applies to the engine's motion and frame."""
    o = mr.oracle_motion(name, modeldirs["rife-v4.6"], tmp_path_factory.getbasetemp())
    _, w, h, scale, _ = mr.E2E[name]
    assert o["flow"].shape == (h, w, 4) and o["mask"].shape == (h, w) and o["frame"].shape == (h, w, 3)
    assert 0.0 < o["mask"].min() and o["mask"].max() < 1.0 and np.abs(o["flow"]).max() > 0.5, "a case without motion checks nothing"
    val, amax = mr.rebuilt((o["a"], o["b"]), o["flow"], o["mask"], o["pad"])
    ok, frac = mr.frame_matches(o["frame"], val, amax, 8)
    print("%s %dx%d scale %d: boundary set %.4f of the codes, max |flow| %.2f px" % (name, w, h, scale, frac, np.abs(o["flow"]).max()))
    assert frac < tr.CAP, frac
    assert ok


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "sanitize", "motion_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_function_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "motion_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"motion_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 200 and int(m.group(2)) == 0, p.stdout[-500:]
    print(p.stdout.splitlines()[-1])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_makefile_builds_the_same_program_and_the_stub():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../motion-check-asan:"):].split("\n", 2)
    assert "motion_check_main.cpp" in rule[0] and "motion_check.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1]
    assert "../motion-check-asan" in mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
    san_src = mk[mk.index("SAN_SRC ="):mk.index("SAN_DEP =")]
    assert "stub_engine_motion.cpp" in san_src
