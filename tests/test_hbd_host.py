"""High bit depth (include/rife_hip.h "high bit depth"), the part that needs no device: the symbols and the header; rife_hip_hbd_check through ctypes on the PRODUCT
library, every rule by its words; the argument checks of the two calls, which come before "no HIP device" whatever the engine handle is; the numpy definition of the
proxy sample (tests/hbd_ref.py reduce10); the Python surface; and tests/sanitize/hbd_check_main.cpp, a program of its own under ASan + UBSan over csrc/hbd_check.h."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import hbd_ref as hr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 34, 18


def image(pixfmt=amd.PIX_I420P10, w=W, h=H, pad=3):
    ps = hr.planes(w, h, pixfmt, 12, 1, pitch_pad=pad)[0]
    return amd.planes_image(tuple(ps), w, h, pixfmt)


def check(img, depth):
    L = amd.lib()
    rc = L.rife_hip_hbd_check(ctypes.byref(img) if img is not None else None, depth)
    return rc, L.rife_hip_last_error().decode()


def refused(img, depth, word):
    rc, msg = check(img, depth)
    assert rc == -amd.EINVAL and word in msg and "high bit depth" in msg, (rc, msg)


def test_symbols_and_header():
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    for s in ("rife_hip_hbd_check", "rife_hip_process_hbd", "rife_hip_process_device_hbd"):
        assert s in amd.C_ABI_SYMBOLS and hasattr(amd.lib(), s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert "rife_hip_op_hbd_to_rgb10" in amd.TEST_ABI_SYMBOLS and "rife_hip_op_hbd_to_rgb10" not in amd.C_ABI_SYMBOLS
    assert re.search(r"\brife_hip_op_hbd_to_rgb10\s*\(", open(os.path.join(ROOT, "include", "rife_hip_test.h")).read())
    assert not hasattr(amd.lib(), "rife_hip_op_hbd_to_rgb10")
    assert "rife_hip_op_apply_yuv" in amd.TEST_ABI_SYMBOLS and "rife_hip_op_apply_yuv" not in amd.C_ABI_SYMBOLS and not hasattr(amd.lib(), "rife_hip_op_apply_yuv")
    assert re.search(r"\brife_hip_op_apply_yuv\s*\(", open(os.path.join(ROOT, "include", "rife_hip_test.h")).read()) and callable(amd.op_apply_yuv)
    # the switch of the fused launch lives in the one switch table, behind ab(): the product does not read it
    sw = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "engine_switches.h")).read()
    assert 's.apply_yuv = not_off(ab("RIFE_HIP_APPLY_YUV"));' in sw
    # the section states the definition operation by operation, and the clause it delivers is gone from the sets section's "Out of scope"
    assert "c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023)" in hdr and "c = min(v, 1023)" in hdr
    assert "Out of scope: making the proxy" not in hdr
    assert hdr.index("rife_hip_process_device_apply_sets(") < hdr.index("---- high bit depth") < hdr.index("rife_hip_hbd_check(") < hdr.index("rife_hip_last_error(void)")


@pytest.mark.parametrize("pixfmt", hr.BASES, ids=lambda p: hr.NAME[p])
def test_hbd_check_rules(pixfmt):
    for depth in range(10, 17):
        for w, h in ((1, 1), (2, 2), (3, 5), (W, H)):
            for pad in (0, 5):
                assert check(image(pixfmt, w, h, pad), depth)[0] == 0, (depth, w, h, pad, check(image(pixfmt, w, h, pad), depth))
    if pixfmt != amd.PIX_RGBP10:
        for csp in (amd.CSP_BT709, amd.CSP_BT601, amd.CSP_BT2020NCL):
            assert check(image(pixfmt | csp), 12)[0] == 0
        refused(image(pixfmt | amd.CSP_FULL), 12, "full-range YUV is served at 8 bits only")      # as for every 10-bit format
    else:
        g = image(pixfmt); g.pixfmt |= amd.CSP_BT601
        refused(g, 12, "a colour description")
    g = image(pixfmt)
    for depth in (9, 17, 0, -1, 8):
        refused(g, depth, "the depth (%d) is not in 10..16" % depth)
    b = image(pixfmt); b.pitch[1] = 2; refused(b, 12, "plane 1: the pitch (2) is smaller than the row bytes")
    b = image(pixfmt); b.pitch[0] = -b.pitch[0]; refused(b, 12, "plane 0: the pitch is negative")
    b = image(pixfmt); b.pitch[2] += 1; refused(b, 12, "plane 2: the pitch is not a multiple of the element size (2)")
    b = image(pixfmt); b.plane[0] += 1; refused(b, 12, "plane 0: the pointer is not aligned to the element size (2)")
    b = image(pixfmt); b.plane[2] = None; refused(b, 12, "plane 2 is NULL")
    b = image(pixfmt); b.w = 0; refused(b, 12, "bad frame size")
    b = image(pixfmt); b.h = 1 << 20; b.pitch[0] = b.pitch[1] = b.pitch[2] = 4096; refused(b, 12, "rows * pitch reaches 2^32 bytes")      # only the descriptor is read
    refused(None, 12, "null image descriptor")


def test_other_formats_are_named():
    u8 = np.zeros((H, W), np.uint8); c8 = np.zeros(((H + 1) // 2, (W + 1) // 2), np.uint8)
    others = [amd.planes_image((u8, c8, c8), W, H, amd.PIX_I420), amd.planes_image((u8, np.zeros(((H + 1) // 2, 2 * ((W + 1) // 2)), np.uint8)), W, H, amd.PIX_NV12),
              amd.planes_image((np.zeros((H, W), np.uint16), np.zeros(((H + 1) // 2, 2 * ((W + 1) // 2)), np.uint16)), W, H, amd.PIX_P010),
              amd.planes_image((u8, u8, u8), W, H, amd.PIX_I444), amd.planes_image((u8, u8, u8), W, H, amd.PIX_RGBP8),
              amd.planes_image(tuple(np.zeros((3, H, W), np.float32)), W, H, amd.PIX_RGBPF), amd.planes_image(tuple(np.zeros((3, H, W), np.float16)), W, H, amd.PIX_RGBPH),
              amd.image_of(np.zeros((H, W, 3), np.uint16)[:, :W - 1]), amd.image_of(np.zeros((H, W + 1), np.uint32)[:, :W])]
    for im in others:
        refused(im, 12, "pixel format %d is not a high-bit-depth layout" % (im.pixfmt & 0xff))
    g = image(); g.pixfmt = 52
    refused(g, 12, "unknown pixel format")


def test_argument_checks_come_before_the_device():
    """-EINVAL for every argument fault of the two calls, with or without a device and whatever the engine handle is (null here: no engine is needed to get there); a
    sound call on a box without a device then gets -ENODEV, on a box with one the null engine is the next -EINVAL."""
    L = amd.lib()
    err = lambda: L.rife_hip_last_error().decode()
    br = lambda d: ctypes.byref(d) if d is not None else None
    calls = {
        "host": lambda a, b, o, depth=12: L.rife_hip_process_hbd(None, br(a), br(b), 0.5, br(o), depth),
        "device": lambda a, b, o, depth=12: L.rife_hip_process_device_hbd(None, br(a), br(b), 0.5, br(o), depth, None),
    }
    for name, call in calls.items():
        for pixfmt in hr.BASES:
            a, b, o = image(pixfmt), image(pixfmt, pad=0), image(pixfmt, pad=9)
            assert call(None, b, o) == -amd.EINVAL and "image 0: null image descriptor" in err() and "high bit depth" in err(), (name, err())
            assert call(a, None, o) == -amd.EINVAL and "image 1: null image descriptor" in err()
            assert call(a, b, None) == -amd.EINVAL and "image out: null image descriptor" in err()
            assert call(a, b, o, 9) == -amd.EINVAL and "image 0: the depth (9) is not in 10..16" in err()
            assert call(a, b, o, 17) == -amd.EINVAL and "the depth (17)" in err()
            bad = image(pixfmt); bad.pitch[1] = 2
            assert call(a, bad, o) == -amd.EINVAL and "image 1: plane 1: the pitch (2) is smaller" in err()
            bad = image(pixfmt); bad.plane[2] = None
            assert call(a, b, bad) == -amd.EINVAL and "image out: plane 2 is NULL" in err()
            assert call(a, b, image(pixfmt, W + 1, H)) == -amd.EINVAL and "the images of one call differ in size" in err()
            other = hr.BASES[(hr.BASES.index(pixfmt) + 1) % 4]
            assert call(a, image(other), o) == -amd.EINVAL and "the images of one call differ in pixel format or colour description" in err()
            if pixfmt != amd.PIX_RGBP10:
                assert call(a, b, image(pixfmt | amd.CSP_BT2020NCL)) == -amd.EINVAL and "differ in pixel format or colour description" in err()
                assert call(image(pixfmt | amd.CSP_FULL), b, o) == -amd.EINVAL and "image 0: full-range YUV" in err()
            u8 = np.zeros((H, W), np.uint8)
            i444 = amd.planes_image((u8, u8, u8), W, H, amd.PIX_I444)
            assert call(i444, i444, i444) == -amd.EINVAL and "image 0: pixel format 49 is not a high-bit-depth layout" in err()
            rc = call(a, b, o)
            assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL), (name, rc, err())      # -RIFE_HIP_ENODEV / "null engine"
            assert ("no HIP device" in err()) if amd.device_count() < 1 else ("null engine" in err())


def test_reduce10():
    """a check of the REFERENCE (tests/hbd_ref.py), which the GPU tests compare the library with: it needs no library and passes without one.  The library's own
    statement of the reduction (csrc/hbd_check.h reduce10) is walked over every sample value by the stand-alone program below, the device's (csrc/hbd.h hbd_code) by
    tests/test_gpu_hbd.py against this function."""
    codes = np.arange(1024, dtype=np.uint32)
    every = np.arange(65536, dtype=np.uint32)
    for depth in range(10, 17):
        assert np.array_equal(hr.reduce10(codes << (depth - 10), depth), codes), "not the identity on c << (depth - 10) at depth %d" % depth
        r = hr.reduce10(every, depth).astype(np.int64)
        assert (np.diff(r) >= 0).all(), "not monotone at depth %d" % depth
        assert r.max() == 1023 and r[65535] == 1023 and r[(1 << depth) - 1] == 1023 and r[0] == 0, "does not saturate at 1023 at depth %d" % depth
        # the definition, spelled out in Python integers on every stored value
        want = [min((v + (1 << (depth - 11))) >> (depth - 10), 1023) if depth > 10 else min(v, 1023) for v in range(0, 65536, 7)]
        assert r[::7].tolist() == want
        # half of the divisor rounds up, one below it rounds down
        if depth > 10:
            half = 1 << (depth - 11)
            assert hr.reduce10(np.array([5 * 2 * half + half - 1, 5 * 2 * half + half]), depth).tolist() == [5, 6]
    assert hr.reduce10(np.array([1023, 1024, 4095], np.uint16), 10).tolist() == [1023, 1023, 1023]
    with pytest.raises(ValueError):
        hr.reduce10(codes, 9)


def test_reference_helpers():
    """likewise a check of the reference's helpers: what hbd_ref.expected hands to the existing sets call is what the header's table says"""
    for pixfmt in hr.BASES:
        shp = hr.plane_shapes(35, 17, pixfmt)
        assert shp[0] == (17, 35) and shp[1] == shp[2] == {amd.PIX_I420P10: (9, 18), amd.PIX_I422P10: (17, 18), amd.PIX_I444P10: (17, 35), amd.PIX_RGBP10: (17, 35)}[pixfmt]
        p0, p1 = hr.planes(35, 17, pixfmt, 12, 3, pitch_pad=5, offset=1)
        assert [p.shape for p in p0] == shp and all(p.dtype == np.uint16 and p.ctypes.data % 4 == 2 for p in p0)
        assert max(int(p.max()) for p in p0) > 4095, "no sample above maxval"
        f = hr.proxy_frame(p0, 12)
        assert f.dtype == np.uint16 and f.size * 2 == amd.frame_bytes(35, 17, pixfmt) and f.max() <= 1023
        out = tuple(np.zeros(s, np.uint16) for s in shp)
        sets = hr.make_sets(p0, p1, 12, pixfmt, out)
        assert len(sets) == (2 if pixfmt in hr.SHIFT else 1)
        for s in sets:
            amd.apply_set_check(s, 35, 17)
            assert s.p0.contents.maxval == 4095 and s.p0.contents.sample == amd.SAMPLE_U16 and (s.wp, s.hp) == (0, 0)
        assert sum(s.out.contents.n for s in sets) == 3 and sets[-1].out.contents.plane[sets[-1].out.contents.n - 1] == out[2].ctypes.data
        if pixfmt in hr.SHIFT:
            assert (sets[1].shift_x, sets[1].shift_y) == hr.SHIFT[pixfmt] and (sets[0].shift_x, sets[0].shift_y) == (0, 0)


def test_python_surface():
    p0, p1 = hr.planes(W, H, amd.PIX_I422P10, 12, 5, pitch_pad=3)
    im = amd.planes_image(tuple(p0), W, H, amd.PIX_I422P10 | amd.CSP_BT2020NCL)
    assert im.pitch[0] == (W + 3) * 2 and im.plane[1] == p0[1].ctypes.data      # views are taken as they are
    amd.hbd_check(im, 12)
    with pytest.raises(amd.RifeError, match=r"\(-1\).*the depth \(18\) is not in 10\.\.16"):
        amd.hbd_check(im, 18)
    for name in ("process_hbd", "process_device_hbd"):
        assert callable(getattr(amd.RIFE, name))
    assert callable(amd.op_hbd_to_rgb10)
    src = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "rife.h")).read()
    assert re.search(r"int process_hbd\(const rife_hip_image_t& in0, const rife_hip_image_t& in1, float timestep, const rife_hip_image_t& out, int depth\) const;", src)


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "sanitize", "hbd_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "hbd_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"hbd_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 5000 and int(m.group(2)) == 0, p.stdout[-500:]
    print(p.stdout.splitlines()[-1])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_makefile_builds_the_same_program():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../hbd-check-asan:"):].split("\n", 2)
    for dep in ("hbd_check_main.cpp", "hbd_check.h", "apply_set_check.h", "apply_check.h", "motion_check.h", "image_check.h"):
        assert dep in rule[0], dep
    for f in SAN[2:]:
        assert f in rule[1]
    line = mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
    assert "../hbd-check-asan" in line and "hbd-check-asan" in mk[mk.index("\nclean:"):]
