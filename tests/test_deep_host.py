"""Deep colour without a GPU: the expected-value recipe of tests/deep_ref.py pinned against the oracle's own 8-bit path, the new C-ABI entry points' argument
checks, the Python mirror's dtype / shape refusals, and the C++ class shim's Mat dispatch."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import deep_ref
from conftest import ROOT
from oracle import pyoracle
from tools import gen_frames

amd = importlib.import_module("rife-ncnn-vulkan_amd")
EINVAL, ENODEV = -1, -2


@pytest.mark.parametrize("w,h", [(100, 60), (256, 160)])
def test_recipe_reproduces_the_oracle_at_depth_8(modeldirs, w, h):
    """planes code * (1 / 255.f) -> flownet `out0` -> * 255.f + 0.5f == OracleRIFE.process() with the GPU crop rule, bit for bit: the helper that produces the
    10-bit expectations is the reference's arithmetic with another scale."""
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(modeldirs["rife-v4.6"])
    a, b = gen_frames.smooth_pair(w, h, 5)
    for t in (0.5, 0.3):
        assert np.array_equal(deep_ref.expected_frame(o, a, b, t, depth=8), o.process(a, b, t))


def test_test_frames_are_truly_10_bit():
    for (w, h) in ((100, 60), (640, 360)):
        a, b = deep_ref.deep_pair(w, h, 9)
        assert a.dtype == np.uint16 and a.shape == (h, w, 3) and a.max() <= 1023
        for f in (a, b):
            assert (f & 3).astype(bool).mean() >= 0.70
        assert not np.array_equal(a, b)
    a8 = deep_ref.to_depth8(a)
    assert a8.dtype == np.uint8 and np.abs(a8.astype(np.float64) * (1023 / 255.0) - a).max() <= 2.01


def test_frame_bytes():
    L = amd.lib()
    assert L.rife_hip_frame_bytes(640, 360, amd.PIX_RGB8) == 640 * 360 * 3
    assert L.rife_hip_frame_bytes(640, 360, amd.PIX_RGB10_U16) == 640 * 360 * 6
    assert L.rife_hip_frame_bytes(640, 360, amd.PIX_A2B10G10R10) == 640 * 360 * 4
    assert L.rife_hip_frame_bytes(7680, 4320, amd.PIX_RGB10_U16) == 7680 * 4320 * 6
    for bad in (3, -1, 99):
        assert L.rife_hip_frame_bytes(640, 360, bad) == 0
    assert L.rife_hip_frame_bytes(0, 360, 1) == 0 and L.rife_hip_frame_bytes(640, -1, 2) == 0
    assert amd.frame_bytes(33, 47, amd.PIX_A2B10G10R10) == 33 * 47 * 4


@pytest.mark.parametrize("which", ["product", "test"])
def test_px_entry_points_check_their_arguments(which):
    """Unknown pixfmt, null pointers and w, h <= 0 are -RIFE_HIP_EINVAL whatever else is passed; with valid arguments and no HIP device the calls fail with
    -RIFE_HIP_ENODEV (there is no CPU path behind them), with a device and no engine with -RIFE_HIP_EINVAL."""
    L = amd.lib() if which == "product" else amd.testlib()
    buf = np.zeros(64 * 6, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    fr = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 1)(buf.ctypes.data)
    ts = (ctypes.c_float * 1)(0.5)
    calls = {
        "process_px": lambda px=1, a=p, b=p, o=p, w=4, h=4: L.rife_hip_process_px(None, a, b, w, h, 0.5, o, px),
        "process_device_px": lambda px=1, a=p, b=p, o=p, w=4, h=4: L.rife_hip_process_device_px(None, a, b, w, h, 0.5, o, px, None),
        "frame_upload_px": lambda px=1, a=p, b=p, o=p, w=4, h=4: L.rife_hip_frame_upload_px(None, a, w, h, px, ctypes.byref(fr) if o else None),
        "process_device_batch_px": lambda px=1, a=p, b=p, o=p, w=4, h=4: L.rife_hip_process_device_batch_px(None, 1, arr, arr, ts, arr, w, h, px, None),
    }
    nodev = L.rife_hip_device_count() <= 0
    for name, f in calls.items():
        for bad in (3, -1, 7):
            assert f(px=bad) == EINVAL, (name, bad)
            assert b"pixel format" in L.rife_hip_last_error()
        assert f(w=0) == EINVAL and f(h=-3) == EINVAL, name
        if name != "process_device_batch_px":
            assert f(a=None) == EINVAL, name
        if name in ("process_px", "process_device_px"):
            assert f(b=None) == EINVAL and f(o=None) == EINVAL, name
        if name == "frame_upload_px":
            assert f(o=None) == EINVAL
        for px in (0, 1, 2):
            assert f(px=px) == (ENODEV if nodev else EINVAL), (name, px)      # valid arguments, no engine
        if nodev:
            assert b"no HIP device" in L.rife_hip_last_error()


def test_python_mirror_refuses_frames_that_match_no_format():
    """Raised by the mirror itself, before any library call: the engine object below has no library handle at all."""
    g = amd.RIFE.__new__(amd.RIFE)
    g._L = None; g._h = None; g._taps = False
    u = np.zeros((8, 8, 3), np.uint16); p = np.zeros((8, 8), np.uint32)
    bad = [(np.zeros((8, 8), np.uint16), None), (np.zeros((8, 8, 4), np.uint16), None), (np.zeros((8, 8, 3), np.uint32), None), (np.zeros((8,), np.uint32), None),
           (u, amd.PIX_A2B10G10R10), (p, amd.PIX_RGB10_U16), (np.zeros((8, 8, 3), np.uint8), amd.PIX_RGB10_U16), (np.zeros((8, 8, 3), np.float32), amd.PIX_A2B10G10R10),
           (u, 3), (u, -1), (np.zeros((0, 8, 3), np.uint16), None)]
    for arr, px in bad:
        with pytest.raises(ValueError):
            g.process(arr, arr, 0.5, pixfmt=px)
        with pytest.raises(ValueError):
            g.upload(arr, pixfmt=px)
    with pytest.raises(ValueError):
        g.process(u, p, 0.5)                                             # the two frames differ in format
    with pytest.raises(ValueError):
        g.process(u, np.zeros((8, 9, 3), np.uint16), 0.5)
    with pytest.raises(ValueError):
        g.process(u, u, 0.5, outimage=np.zeros((8, 8, 3), np.uint8))     # the output has the inputs' format
    for px in (3, -1):
        with pytest.raises(ValueError):
            g.process_device(1, 2, 8, 8, 0.5, 3, pixfmt=px)
        with pytest.raises(ValueError):
            g.process_device_batch([1], [2], 8, 8, [0.5], [3], pixfmt=px)
    f0 = amd.Frame(None, 8, 8, L=object(), pixfmt=amd.PIX_RGB10_U16); f1 = amd.Frame(None, 8, 8, L=object(), pixfmt=amd.PIX_RGB8)
    f0._f = f1._f = 1
    with pytest.raises(ValueError):
        g.process_frames(f0, f1, 0.5)
    f0._f = f1._f = None
    assert np.array_equal(amd.unpack_a2b10g10r10(amd.pack_a2b10g10r10(u + 700)), u + 700)
    assert np.all(amd.pack_a2b10g10r10(u + 5000) == np.uint32(0xffffffff))        # clamped to 1023, alpha 3


SHIM_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "rife.h"
#include "rife_hip.h"
int main() {
    RIFE r(0, false, false, false, 1, false, true);
    std::vector<uint16_t> a(8 * 8 * 3, 100), b(8 * 8 * 3, 200), o16(8 * 8 * 3, 7);
    std::vector<unsigned char> o8(8 * 8 * 3, 7), a8(8 * 8 * 3, 1);
    ncnn::Mat m0(8, 8, (void*)a.data(), (size_t)6, 3), m1(8, 8, (void*)b.data(), (size_t)6, 3);
    ncnn::Mat out8(8, 8, (void*)o8.data(), (size_t)3, 3), out16(8, 8, (void*)o16.data(), (size_t)6, 3), in8(8, 8, (void*)a8.data(), (size_t)3, 3);
    int rc = r.process(m0, m1, 0.5f, out8);                  // 10-bit inputs, 8-bit output Mat
    printf("mixed_out %d\n", rc);
    rc = r.process(m0, in8, 0.5f, out16);                    // the inputs differ
    printf("mixed_in %d\n", rc);
    rc = r.process(in8, in8, 0.5f, out16);                   // 8-bit inputs, 10-bit output Mat
    printf("mixed_out8 %d\n", rc);
    rc = r.process(m0, m1, 0.5f, out16);                     // all agree: reaches the engine (no device here: ENODEV; on a GPU box: before load())
    printf("agree %d\n", rc);
    ncnn::Mat t0;
    rc = r.process(m0, m1, 0.0f, t0);                        // timestep 0 rebinds, as for 8-bit Mats
    printf("rebind %d %d %d\n", rc, t0.data == m0.data, (int)t0.elemsize);
    printf("untouched %d %d\n", o8[0], o16[0]);
    return 0;
}
"""


def test_cpp_class_shim_compiles_and_refuses_mixed_depths(tmp_path):
    src = tmp_path / "deep_shim.cpp"
    src.write_text(SHIM_SRC)
    csrc = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc")
    exe = str(tmp_path / "deep_shim")
    libdir = os.path.join(ROOT, "rife-ncnn-vulkan_amd")
    c = subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-lrife", "-lrife_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-800:]
    out = dict(l.split(" ", 1) for l in p.stdout.splitlines())
    assert out["mixed_out"] == str(EINVAL) and out["mixed_in"] == str(EINVAL) and out["mixed_out8"] == str(EINVAL), p.stdout
    assert int(out["agree"]) < 0 and int(out["agree"]) != EINVAL or amd.device_count() > 0, p.stdout
    assert out["rebind"] == "0 1 6", p.stdout
    assert out["untouched"] == "7 7", p.stdout
    assert "pixel format" in p.stderr
