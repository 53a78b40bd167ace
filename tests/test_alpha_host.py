"""RGBA frames without a GPU: the new pixel format at the C boundary, the expected-value recipe of tests/alpha_ref.py pinned on the oracle alone, the Python
mirror's refusals and the C++ class shim's Mat dispatch."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import alpha_ref
import deep_ref
from conftest import ROOT
from oracle import pyoracle
from tools import gen_frames

amd = importlib.import_module("rife-ncnn-vulkan_amd")
EINVAL, ENODEV = -1, -2
RGBA = 4


def test_the_format_number():
    assert amd.PIX_RGBA8 == RGBA
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    assert "#define RIFE_HIP_PIX_RGBA8        4" in hdr and "3 is reserved" in hdr


def test_frame_bytes():
    L = amd.lib()
    assert L.rife_hip_frame_bytes(640, 360, RGBA) == 640 * 360 * 4
    assert L.rife_hip_frame_bytes(1, 1, RGBA) == 4 and L.rife_hip_frame_bytes(7680, 4320, RGBA) == 7680 * 4320 * 4
    assert L.rife_hip_frame_bytes(0, 360, RGBA) == 0 and L.rife_hip_frame_bytes(640, -1, RGBA) == 0
    assert L.rife_hip_frame_bytes(640, 360, 3) == 0 and L.rife_hip_frame_bytes(640, 360, 5) == 0
    assert amd.frame_bytes(33, 47, amd.PIX_RGBA8) == 33 * 47 * 4
    assert amd.testlib().rife_hip_frame_bytes(33, 47, RGBA) == 33 * 47 * 4


@pytest.mark.parametrize("which", ["product", "test"])
def test_px_entry_points_take_the_format(which):
    """With format 4 the four _px calls pass the argument checks: null pointers and w, h <= 0 are -RIFE_HIP_EINVAL, valid arguments reach "no HIP device"
    (-RIFE_HIP_ENODEV; with a device and no engine: -RIFE_HIP_EINVAL with a message that is not about the pixel format)."""
    L = amd.lib() if which == "product" else amd.testlib()
    buf = np.zeros(64 * 4, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    fr = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 1)(buf.ctypes.data)
    ts = (ctypes.c_float * 1)(0.5)
    calls = {
        "process_px": lambda a=p, b=p, o=p, w=4, h=4: L.rife_hip_process_px(None, a, b, w, h, 0.5, o, RGBA),
        "process_device_px": lambda a=p, b=p, o=p, w=4, h=4: L.rife_hip_process_device_px(None, a, b, w, h, 0.5, o, RGBA, None),
        "frame_upload_px": lambda a=p, b=p, o=p, w=4, h=4: L.rife_hip_frame_upload_px(None, a, w, h, RGBA, ctypes.byref(fr) if o else None),
        "process_device_batch_px": lambda a=p, b=p, o=p, w=4, h=4: L.rife_hip_process_device_batch_px(None, 1, arr, arr, ts, arr, w, h, RGBA, None),
    }
    nodev = L.rife_hip_device_count() <= 0
    for name, f in calls.items():
        assert f(w=0) == EINVAL and f(h=-3) == EINVAL, name
        if name != "process_device_batch_px":
            assert f(a=None) == EINVAL, name
        assert f() == (ENODEV if nodev else EINVAL), name
        assert b"pixel format" not in L.rife_hip_last_error(), (name, L.rife_hip_last_error())
        if nodev:
            assert b"no HIP device" in L.rife_hip_last_error()


# ---- the recipe's own pins (oracle only) ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle(modeldirs):
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(modeldirs["rife-v4.6"])
    return o


@pytest.mark.parametrize("w,h", [(64, 64), (100, 60), (160, 96)])
def test_injecting_the_oracles_own_flows_reproduces_out0(oracle, w, h):
    """With flow0 .. flow3 injected `out0` is bit for bit the plain run's: it then depends on in0 / in1 through the two warps and the blend only.  And the
    depth-8 recipe quantises to OracleRIFE.process()."""
    a, b = alpha_ref.rgb_pair(w, h, 5)
    for t in (0.5, 0.3):
        flows = alpha_ref.colour_flows(oracle, a, b, t)
        plain = deep_ref.extract(oracle, a, b, t, 8, "out0")
        assert np.array_equal(deep_ref.extract(oracle, a, b, t, 8, "out0", flows=flows), plain)
        assert np.array_equal(deep_ref.quantise(plain, w, h, 8), oracle.process(a, b, t))


@pytest.mark.parametrize("w,h", [(64, 64), (100, 60), (160, 96)])
def test_the_alpha_run_gives_three_equal_channels(oracle, w, h):
    a, b = alpha_ref.rgba_pair(w, h, 6, "smooth")
    flows = alpha_ref.colour_flows(oracle, a[..., :3].copy(), b[..., :3].copy(), 0.4)
    out = alpha_ref.alpha_out0(oracle, a[..., 3], b[..., 3], 0.4, flows)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


@pytest.mark.parametrize("w,h", [(64, 64), (160, 96)])
@pytest.mark.parametrize("ch", [0, 1, 2])
def test_alpha_equal_to_a_colour_plane_gives_that_colour_plane(oracle, w, h, ch):
    """At 32n sizes (no padding, so no padding rule): alpha := a colour plane gives out0[0] of the alpha run == that plane of the colour run, bit for bit."""
    a, b = alpha_ref.rgb_pair(w, h, 7)
    flows = alpha_ref.colour_flows(oracle, a, b, 0.5)
    colour = deep_ref.extract(oracle, a, b, 0.5, 8, "out0", flows=flows)
    al = alpha_ref.alpha_out0(oracle, a[..., ch], b[..., ch], 0.5, flows)
    assert np.array_equal(al[0], colour[ch])


@pytest.mark.parametrize("w,h", [(100, 60), (33, 47), (1, 1), (333, 241)])
def test_edge_replicated_alpha_keeps_opaque_frames_opaque(oracle, w, h):
    """The padding rule of include/rife_hip.h and the measurement behind it: opaque in gives 255 everywhere with edge-replicated alpha; with ZERO-padded alpha
    (printed, not asserted: it is the defect the rule avoids) flows of a few pixels reach into the padding."""
    a, b = alpha_ref.rgba_pair(w, h, 8, 255)
    want = alpha_ref.expected_rgba(oracle, a, b, 0.5)
    assert np.all(want[..., 3] == 255)
    assert np.array_equal(want[..., :3], oracle.process(a[..., :3].copy(), b[..., :3].copy(), 0.5))
    clear = alpha_ref.expected_rgba(oracle, *alpha_ref.rgba_pair(w, h, 8, 0), 0.5)
    assert np.all(clear[..., 3] == 0)
    rgb0, rgb1 = a[..., :3].copy(), b[..., :3].copy()
    flows = alpha_ref.colour_flows(oracle, rgb0, rgb1, 0.5)
    ones = np.full((h, w, 3), 255, np.uint8)
    zp = deep_ref.quantise(deep_ref.extract(oracle, ones, ones, 0.5, 8, "out0", flows=flows), w, h, 8)[..., 0]
    print("zero-padded alpha %dx%d: %.2f %% of the pixels below 255, minimum %d" % (w, h, 100.0 * float((zp < 255).mean()), int(zp.min())))


def test_test_mattes_move_and_are_what_they_say():
    for hard in (False, True):
        m0, m1 = alpha_ref.matte_pair(160, 96, 3, hard)
        assert m0.dtype == np.uint8 and m0.shape == (96, 160) and not np.array_equal(m0, m1)
        if hard:
            assert set(np.unique(m0)) <= {0, 255} and 0.05 < (m0 == 255).mean() < 0.95
        else:
            assert len(np.unique(m0)) > 64
    a, b = alpha_ref.rgba_pair(64, 48, 1)
    assert a.shape == (48, 64, 4) and a.dtype == np.uint8 and a.flags.c_contiguous


# ---- Python mirror -----------------------------------------------------------------------------------------------------------------------------

def test_python_mirror_refuses_frames_that_match_no_format():
    """Raised by the mirror itself, before any library call: the engine object below has no library handle at all."""
    g = amd.RIFE.__new__(amd.RIFE)
    g._L = None; g._h = None; g._taps = False
    r = np.zeros((8, 8, 4), np.uint8); c = np.zeros((8, 8, 3), np.uint8); u = np.zeros((8, 8, 3), np.uint16)
    bad = [(c, amd.PIX_RGBA8), (r, amd.PIX_RGB10_U16), (r, amd.PIX_A2B10G10R10), (np.zeros((8, 8, 4), np.uint16), amd.PIX_RGBA8), (np.zeros((8, 8, 4), np.float32), amd.PIX_RGBA8),
           (np.zeros((8, 8), np.uint8), amd.PIX_RGBA8), (np.zeros((0, 8, 4), np.uint8), None), (r, 3), (r, 5)]
    for arr, px in bad:
        with pytest.raises(ValueError):
            g.process(arr, arr, 0.5, pixfmt=px)
        with pytest.raises(ValueError):
            g.upload(arr, pixfmt=px)
    for other in (c, u, np.zeros((8, 9, 4), np.uint8)):
        with pytest.raises(ValueError):
            g.process(r, other, 0.5)                                     # the two frames differ in format or size
    with pytest.raises(ValueError):
        g.process(c, r, 0.5)                                             # RGB first, RGBA second: refused too
    for out in (c.copy(), np.zeros((8, 8, 4), np.uint16), np.zeros((8, 8, 4), np.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            g.process(r, r, 0.5, outimage=out)                           # the output has the inputs' format
    f0 = amd.Frame(None, 8, 8, L=object(), pixfmt=amd.PIX_RGBA8); f1 = amd.Frame(None, 8, 8, L=object(), pixfmt=amd.PIX_RGB8)
    f0._f = f1._f = 1
    with pytest.raises(ValueError):
        g.process_frames(f0, f1, 0.5)
    f1.pixfmt = amd.PIX_RGBA8
    with pytest.raises(ValueError):
        g.process_frames(f0, f1, 0.5, outimage=np.zeros((8, 8, 3), np.uint8))
    f0._f = f1._f = None
    assert amd._pix_of(r) == amd.PIX_RGBA8 and amd._pix_of(c) is None and amd._pix_of(r, amd.PIX_RGBA8) == amd.PIX_RGBA8


# ---- C++ class shim ------------------------------------------------------------------------------------------------------------------------------

SHIM_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "rife.h"
#include "rife_hip.h"
int main() {
    RIFE r(0, false, false, false, 1, false, true);
    std::vector<unsigned char> a(8 * 8 * 4, 100), b(8 * 8 * 4, 200), o4(8 * 8 * 4, 7), o3(8 * 8 * 3, 7), a3(8 * 8 * 3, 1);
    std::vector<uint16_t> o16(8 * 8 * 3, 7);
    ncnn::Mat m0(8, 8, (void*)a.data(), (size_t)4, 4), m1(8, 8, (void*)b.data(), (size_t)4, 4);
    ncnn::Mat out3(8, 8, (void*)o3.data(), (size_t)3, 3), out4(8, 8, (void*)o4.data(), (size_t)4, 4), out16(8, 8, (void*)o16.data(), (size_t)6, 3), in3(8, 8, (void*)a3.data(), (size_t)3, 3);
    int rc = r.process(m0, m1, 0.5f, out3);                  // RGBA inputs, RGB output Mat
    printf("mixed_out %d\n", rc);
    rc = r.process(m0, in3, 0.5f, out4);                     // the inputs differ
    printf("mixed_in %d\n", rc);
    rc = r.process(in3, in3, 0.5f, out4);                    // RGB inputs, RGBA output Mat
    printf("mixed_out3 %d\n", rc);
    rc = r.process(m0, m1, 0.5f, out16);                     // RGBA inputs, 10-bit output Mat
    printf("mixed_out16 %d\n", rc);
    rc = r.process(m0, m1, 0.5f, out4);                      // all agree: reaches the engine (no device here: ENODEV; on a GPU box: before load())
    printf("agree %d\n", rc);
    ncnn::Mat t0, t1;
    rc = r.process(m0, m1, 0.0f, t0);                        // timestep 0 / 1 rebind, as for RGB Mats
    printf("rebind0 %d %d %d %d\n", rc, t0.data == m0.data, (int)t0.elemsize, t0.elempack);
    rc = r.process(m0, m1, 1.0f, t1);
    printf("rebind1 %d %d %d %d\n", rc, t1.data == m1.data, (int)t1.elemsize, t1.elempack);
    printf("untouched %d %d %d\n", o3[0], o4[0], (int)o16[0]);
    printf("bytes %zu\n", rife_hip_frame_bytes(8, 8, RIFE_HIP_PIX_RGBA8));
    return 0;
}
"""


def test_cpp_class_shim_compiles_and_refuses_mixed_formats(tmp_path):
    src = tmp_path / "alpha_shim.cpp"
    src.write_text(SHIM_SRC)
    csrc = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc")
    exe = str(tmp_path / "alpha_shim")
    libdir = os.path.join(ROOT, "rife-ncnn-vulkan_amd")
    c = subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-lrife", "-lrife_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-800:]
    out = dict(l.split(" ", 1) for l in p.stdout.splitlines())
    for k in ("mixed_out", "mixed_in", "mixed_out3", "mixed_out16"):
        assert out[k] == str(EINVAL), p.stdout
    assert int(out["agree"]) < 0 and int(out["agree"]) != EINVAL or amd.device_count() > 0, p.stdout
    assert out["rebind0"] == "0 1 4 4" and out["rebind1"] == "0 1 4 4", p.stdout
    assert out["untouched"] == "7 7 7", p.stdout
    assert out["bytes"] == "256", p.stdout
    assert "pixel format" in p.stderr
