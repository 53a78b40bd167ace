"""16-bit packed RGB and RGBA (include/rife_hip.h "16-bit packed RGB and RGBA"), the part that needs no device: the symbols and the header; rife_hip_packed_check through
ctypes on the PRODUCT library, every rule by its words; the agreement of the three images and the argument checks of the two calls, which come before "no HIP device"
whatever the engine handle is; the numpy reference's helpers (tests/packed_ref.py); the Python surface; and tests/sanitize/packed_check_main.cpp, a program of its own
under ASan + UBSan over csrc/packed_check.h.  (The codecs of `rife-hip -b 16` and its start-up refusals: tests/test_cli_packed.py.)"""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import packed_ref as pr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 34, 18


def image(ch=4, w=W, h=H, depth=12, pad=3):
    return amd.packed_of(pr.frames(w, h, ch, depth, 1, w * ch + pad)[0], depth)


def check(img):
    L = amd.lib()
    rc = L.rife_hip_packed_check(ctypes.byref(img) if img is not None else None)
    return rc, L.rife_hip_last_error().decode()


def refused(img, word):
    rc, msg = check(img)
    assert rc == -amd.EINVAL and word in msg and msg.startswith("high bit depth: "), (rc, msg)


def test_symbols_and_header():
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    for s in ("rife_hip_packed_check", "rife_hip_process_hbd_packed", "rife_hip_process_device_hbd_packed"):
        assert s in amd.C_ABI_SYMBOLS and hasattr(amd.lib(), s) and re.search(r"\b%s\s*\(" % s, hdr), s
    thdr = open(os.path.join(ROOT, "include", "rife_hip_test.h")).read()
    for s in ("rife_hip_op_packed_to_rgb10", "rife_hip_op_apply_packed"):
        assert s in amd.TEST_ABI_SYMBOLS and s not in amd.C_ABI_SYMBOLS and not hasattr(amd.lib(), s) and re.search(r"\b%s\s*\(" % s, thdr), s
    # no new pixfmt number: 3 and 5..15 stay unknown
    for px in (3, 5, 15):
        im = amd.device_image(4, 4, px, [(4096, 64)])
        assert amd.lib().rife_hip_image_check(ctypes.byref(im)) == -amd.EINVAL
    # the section states the definition and what it leaves out, after the hbd section
    assert hdr.index("rife_hip_process_device_hbd(") < hdr.index("---- 16-bit packed RGB and RGBA") < hdr.index("rife_hip_packed_check(") < hdr.index("rife_hip_last_error(void)")
    sec = hdr[hdr.index("---- 16-bit packed RGB and RGBA"):hdr.index("rife_hip_packed_check(")]
    for words in ("c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023)", "Alpha never reaches the network", "Opaque in (A = maxval everywhere) gives maxval everywhere",
                  "a public apply-only call on packed frames", "packed float or u8 frames", "BGR(A) channel order", "resident packed frames (stream mode) and the batch calls",
                  "MSB-aligned samples", 'the words "high bit depth"'):
        assert words in sec, words
    st = amd.rife_hip_packed
    assert [f[0] for f in st._fields_] == ["w", "h", "channels", "depth", "data", "pitch"] and ctypes.sizeof(st) == 32


@pytest.mark.parametrize("ch", (3, 4))
def test_packed_check_rules(ch):
    for depth in range(10, 17):
        for w, h in ((1, 1), (2, 2), (3, 5), (W, H)):
            for pad in (0, 5):
                assert check(image(ch, w, h, depth, pad))[0] == 0, (depth, w, h, pad, check(image(ch, w, h, depth, pad)))
    new = lambda: image(ch)
    b = new(); b.w = 0; refused(b, "bad image size")
    b = new(); b.h = -2; refused(b, "bad image size")
    for c in (0, 1, 2, 5, -1):
        b = new(); b.channels = c; refused(b, "the channel count (%d) is not 3 (R G B) or 4 (R G B A)" % c)
    for depth in (9, 17, 0, -1, 8):
        b = new(); b.depth = depth; refused(b, "the depth (%d) is not in 10..16" % depth)
    b = new(); b.data = None; refused(b, "null data pointer")
    b = new(); b.data += 1; refused(b, "the data pointer is not aligned to 2 bytes")
    b = new(); b.pitch = 0; refused(b, "the pitch is not positive")
    b = new(); b.pitch = -b.pitch; refused(b, "the pitch is not positive")
    b = new(); b.pitch = W * ch * 2 - 2; refused(b, "the pitch is smaller than a row of w * channels * 2 bytes")
    b = new(); b.pitch += 1; refused(b, "the pitch is not a multiple of 2 bytes")
    b = new(); b.pitch = (1 << 31); refused(b, "the pitch exceeds INT32_MAX")                                    # only the descriptor is read
    b = new(); b.w = 1 << 14; b.h = (1 << 13) + 1; b.pitch = b.w * ch * 2; refused(b, "image too large (more than 2^27 pixels)")
    b = new(); b.w = 1; b.h = 1 << 20; b.pitch = 4096; refused(b, "rows * pitch reaches 2^32 bytes")
    b = new(); b.w = 1; b.h = 1 << 20; b.pitch = 4094; assert check(b)[0] == 0                                   # one short of 2^32
    refused(None, "null descriptor")


def test_argument_checks_come_before_the_device():
    """-EINVAL for every argument fault of the two calls, with or without a device and whatever the engine handle is (null here: no engine is needed to get there); a
    sound call on a box without a device then gets -ENODEV, on a box with one the null engine is the next -EINVAL."""
    L = amd.lib()
    err = lambda: L.rife_hip_last_error().decode()
    br = lambda d: ctypes.byref(d) if d is not None else None
    calls = {
        "host": lambda a, b, o: L.rife_hip_process_hbd_packed(None, br(a), br(b), 0.5, br(o)),
        "device": lambda a, b, o: L.rife_hip_process_device_hbd_packed(None, br(a), br(b), 0.5, br(o), None),
    }
    for name, call in calls.items():
        for ch in (3, 4):
            a, b, o = image(ch), image(ch, pad=0), image(ch, pad=9)
            assert call(None, b, o) == -amd.EINVAL and err().startswith("high bit depth: image 0: null descriptor"), (name, err())
            assert call(a, None, o) == -amd.EINVAL and err().startswith("high bit depth: image 1: null descriptor")
            assert call(a, b, None) == -amd.EINVAL and err().startswith("high bit depth: image out: null descriptor")
            bad = image(ch); bad.depth = 9
            assert call(bad, b, o) == -amd.EINVAL and "image 0: the depth (9) is not in 10..16" in err()
            bad = image(ch); bad.pitch = 2
            assert call(a, bad, o) == -amd.EINVAL and "image 1: the pitch is smaller than a row" in err()
            bad = image(ch); bad.data = None
            assert call(a, b, bad) == -amd.EINVAL and "image out: null data pointer" in err()
            # the three images agree in w, h, channels and depth
            assert call(a, image(ch, W + 1, H), o) == -amd.EINVAL and "image 0 and image 1 differ in size" in err()
            assert call(a, b, image(ch, W, H + 1)) == -amd.EINVAL and "image 0 and image out differ in size" in err()
            assert call(a, image(7 - ch), o) == -amd.EINVAL and "image 0 and image 1 differ in channels" in err()
            assert call(a, b, image(7 - ch)) == -amd.EINVAL and "image 0 and image out differ in channels" in err()
            assert call(a, image(ch, depth=16), o) == -amd.EINVAL and "image 0 and image 1 differ in depth" in err()
            assert call(a, b, image(ch, depth=10)) == -amd.EINVAL and "image 0 and image out differ in depth" in err()
            rc = call(a, b, o)
            assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL), (name, rc, err())      # -RIFE_HIP_ENODEV / "null engine"
            assert ("no HIP device" in err()) if amd.device_count() < 1 else ("null engine" in err())


def test_reference_helpers():
    """a check of the REFERENCE (tests/packed_ref.py), which the GPU tests compare the library with: it needs no library call beyond the descriptors"""
    for ch in (3, 4):
        a, b = pr.frames(35, 17, ch, 12, 3, 35 * ch + 6, 1)
        assert a.shape == (17, 35, ch) and a.dtype == np.uint16 and a.ctypes.data % 4 == 2 and a.strides == ((35 * ch + 6) * 2, ch * 2, 2)
        assert int(a[..., :3].max()) > 4095, "no sample above maxval"
        planes = pr.deinterleave(a)
        assert len(planes) == ch and all(p.flags.c_contiguous and np.array_equal(p, a[:, :, k]) for k, p in enumerate(planes))
        assert np.array_equal(pr.interleave(planes), a) and pr.interleave(planes).flags.c_contiguous
        f = pr.proxy_frame(a, 12)
        assert f.dtype == np.uint16 and f.size * 2 == amd.frame_bytes(35, 17, amd.PIX_RGBP10) and f.max() <= 1023
        assert np.array_equal(f[:35 * 17].reshape(17, 35), pr.reduce10(a[:, :, 0], 12))
        o = pr.blank_like(a)
        assert o.shape == a.shape and o.strides == a.strides and o.ctypes.data % 4 == 2 and (o == pr.SENTINEL).all() and pr.untouched(o)
        o[...] = 7
        assert pr.untouched(o)
        pr.big(o)[0, 0] = 7
        assert not pr.untouched(o)
        if ch == 4:
            assert (pr.frames(8, 8, 4, 16, 1, opaque=True)[0][..., 3] == 65535).all()
    r0, r1 = pr.random_frames(9, 5, 3, np.random.default_rng(1), pr.tight_pitch(9, 3, 8, pad=4))
    assert r0.strides[0] == 64 and r0.ctypes.data % 64 == 0 and (r0 != r1).any()


def test_python_surface():
    a, b = pr.frames(W, H, 4, 12, 5, W * 4 + 3)
    d = amd.packed_of(a, 12)
    assert (d.w, d.h, d.channels, d.depth, d.pitch, d.data) == (W, H, 4, 12, (W * 4 + 3) * 2, a.ctypes.data)      # views are taken as they are
    amd.packed_check(a, 12)
    amd.packed_check(d, 12)
    with pytest.raises(amd.RifeError, match=r"\(-1\).*the depth \(18\) is not in 10\.\.16"):
        amd.packed_check(a, 18)
    for bad in (a.astype(np.uint8), a[:, :, :2], a[:, ::2], a[..., 0], np.zeros((0, 4, 3), np.uint16), [1, 2]):
        with pytest.raises(ValueError, match="uint16 array of shape"):
            amd.packed_of(bad, 12)
    ro = a.copy(); ro.flags.writeable = False
    with pytest.raises(ValueError, match="a writable uint16 array"):
        amd.packed_of(ro, 12, "out", writable=True)
    g = amd.RIFE.__new__(amd.RIFE)      # the argument checks of the method come before the engine is looked at
    with pytest.raises(ValueError, match="in1: a uint16 array"):
        amd.RIFE.process_hbd_packed(g, a, a.astype(np.float32), 0.5, 12)
    for name in ("process_hbd_packed", "process_device_hbd_packed"):
        assert callable(getattr(amd.RIFE, name))
    assert callable(amd.op_packed_to_rgb10) and callable(amd.op_apply_packed) and callable(amd.packed_desc)
    src = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "rife.h")).read()
    assert re.search(r"int process_hbd_packed\(const rife_hip_packed_t& in0, const rife_hip_packed_t& in1, float timestep, const rife_hip_packed_t& out\) const;", src)


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "sanitize", "packed_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "packed_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"packed_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 4000 and int(m.group(2)) == 0, p.stdout[-500:]
    print(p.stdout.splitlines()[-1])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_makefile_builds_the_same_program():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../packed-check-asan:"):].split("\n", 2)
    for dep in ("packed_check_main.cpp", "packed_check.h", "rife_hip.h"):
        assert dep in rule[0], dep
    for f in SAN[2:]:
        assert f in rule[1]
    line = mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
    assert "../packed-check-asan" in line and "packed-check-asan" in mk[mk.index("\nclean:"):]
