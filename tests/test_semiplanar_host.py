"""Semi-planar high bit depth (include/rife_hip.h "semi-planar high bit depth"), the part that needs no device: the symbols, the header and the struct's layout;
rife_hip_semiplanar_check through ctypes on the PRODUCT library, every rule by its words; the agreement of the three images and the argument checks of the two calls,
which come before "no HIP device" whatever the engine handle is; the numpy reference's helpers (tests/semiplanar_ref.py); the Python surface; and
tests/sanitize/semiplanar_check_main.cpp, a program of its own under ASan + UBSan over csrc/semiplanar_check.h."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import semiplanar_ref as sr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 34, 18


def image(chroma=1, w=W, h=H, depth=12, pad=3, csp=0):
    y, c = sr.surfaces(w, h, chroma, depth, 1, pad)[0]
    return amd.semiplanar_of(y, c, depth, chroma, csp)


def check(img):
    L = amd.lib()
    rc = L.rife_hip_semiplanar_check(ctypes.byref(img) if img is not None else None)
    return rc, L.rife_hip_last_error().decode()


def refused(img, word):
    rc, msg = check(img)
    assert rc == -amd.EINVAL and word in msg and msg.startswith("high bit depth: "), (rc, msg)


def test_symbols_header_and_struct():
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    for s in ("rife_hip_semiplanar_check", "rife_hip_process_hbd_semiplanar", "rife_hip_process_device_hbd_semiplanar"):
        assert s in amd.C_ABI_SYMBOLS and hasattr(amd.lib(), s) and re.search(r"\b%s\s*\(" % s, hdr), s
    thdr = open(os.path.join(ROOT, "include", "rife_hip_test.h")).read()
    for s in ("rife_hip_op_sp_to_rgb10", "rife_hip_op_apply_sp"):
        assert s in amd.TEST_ABI_SYMBOLS and s not in amd.C_ABI_SYMBOLS and not hasattr(amd.lib(), s) and re.search(r"\b%s\s*\(" % s, thdr) and s not in hdr, s
    # no new pixfmt number: the semi-planar slots stay unknown formats, and the hbd check keeps refusing P010 by name
    for px in (34, 50, 20):
        im = amd.device_image(4, 4, px, [(4096, 64), (8192, 64)])
        assert amd.lib().rife_hip_image_check(ctypes.byref(im)) == -amd.EINVAL
    im = amd.planes_image((np.zeros((4, 4), np.uint16), np.zeros((2, 4), np.uint16)), 4, 4, amd.PIX_P010)
    assert amd.lib().rife_hip_hbd_check(ctypes.byref(im), 10) == -amd.EINVAL and "pixel format 18" in amd.lib().rife_hip_last_error().decode()
    # the section sits after the packed one, states the definition and what it leaves out
    assert hdr.index("rife_hip_process_device_hbd_packed(") < hdr.index("---- semi-planar high bit depth") < hdr.index("rife_hip_semiplanar_check(") < hdr.index("rife_hip_last_error(void)")
    sec = hdr[hdr.index("---- semi-planar high bit depth"):hdr.index("rife_hip_semiplanar_check(")]
    for words in ("s = 16 - depth", "split(img)", "join(planes << s)", "RIFE_HIP_PIX_I420P10 | csp", "RIFE_HIP_PIX_I422P10 | csp", "(v >> s) << s",
                  "c = min((v + (1 << (depth - 11))) >> (depth - 10), 1023)", 'the words "high bit depth"', 'before "no HIP device"',
                  "4:4:4 semi-planar (P410 / P416)", "Cr, Cb order (NV21-like)", "LSB-aligned semi-planar and MSB-aligned planar samples", "8-bit NV12 / NV16",
                  "a public apply-only call", "resident semi-planar frames (stream mode) and the batch calls", "the command line", "must not overlap"):
        assert words in sec, words
    # the hbd section no longer lists what this section delivers
    hbd = hdr[hdr.index("---- high bit depth"):hdr.index("rife_hip_hbd_check(")]
    assert "Out of scope: semi-planar or MSB-aligned samples" not in hbd and "semi-planar high bit depth" in hbd
    # the struct as the header declares it: five ints, then pointer / pitch pairs
    decl = hdr[hdr.index("typedef struct rife_hip_semiplanar {"):hdr.index("} rife_hip_semiplanar_t;")]
    names = re.findall(r"\b(?:int|void\*|ptrdiff_t)\s+([a-z_, ]+);", decl)
    assert [n.strip() for part in names for n in part.split(",")] == ["w", "h", "chroma", "csp", "depth", "y", "pitch_y", "cbcr", "pitch_c"]
    st = amd.rife_hip_semiplanar
    assert [f[0] for f in st._fields_] == ["w", "h", "chroma", "csp", "depth", "y", "pitch_y", "cbcr", "pitch_c"]
    assert ctypes.sizeof(st) == 56 and [getattr(st, f).offset for f, _ in st._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48]


@pytest.mark.parametrize("chroma", (1, 2))
def test_semiplanar_check_rules(chroma):
    for depth in range(10, 17):
        for w, h in ((1, 1), (2, 2), (3, 5), (W, H)):
            for pad in (0, 5):
                for csp in (amd.CSP_BT709, amd.CSP_BT601, amd.CSP_BT2020NCL):
                    assert check(image(chroma, w, h, depth, pad, csp))[0] == 0, (depth, w, h, pad, csp, check(image(chroma, w, h, depth, pad, csp)))
    new = lambda: image(chroma)
    cw = (W + 1) // 2
    b = new(); b.w = 0; refused(b, "bad image size")
    b = new(); b.h = -2; refused(b, "bad image size")
    b = new(); b.chroma = 3; refused(b, "4:4:4 semi-planar (P410 / P416) is not served")
    for c in (0, 4, -1):
        b = new(); b.chroma = c; refused(b, "the chroma mode (%d) is not 1 (4:2:0) or 2 (4:2:2)" % c)
    b = new(); b.csp = amd.CSP_FULL; refused(b, "RIFE_HIP_CSP_FULL")
    b = new(); b.csp = amd.CSP_FULL | amd.CSP_BT601; refused(b, "full-range YUV is served at 8 bits only")
    for c in (3 << 8, 1, 1 << 13, 4 << 8):
        b = new(); b.csp = c; refused(b, "the colour description (%d) is not RIFE_HIP_CSP_BT709, _BT601 or _BT2020NCL" % c)
    for depth in (9, 17, 0, -1, 8):
        b = new(); b.depth = depth; refused(b, "the depth (%d) is not in 10..16" % depth)
    b = new(); b.y = None; refused(b, "null y pointer")
    b = new(); b.cbcr = None; refused(b, "null cbcr pointer")
    b = new(); b.y += 1; refused(b, "the y pointer is not aligned to 2 bytes")
    b = new(); b.cbcr += 1; refused(b, "the cbcr pointer is not aligned to 2 bytes")
    b = new(); b.pitch_y = 0; refused(b, "the y pitch is not positive")
    b = new(); b.pitch_c = -b.pitch_c; refused(b, "the cbcr pitch is not positive")
    b = new(); b.pitch_y = 2 * W - 2; refused(b, "the y pitch is smaller than a row of w * 2 bytes")
    b = new(); b.pitch_c = 4 * cw - 2; refused(b, "the cbcr pitch is smaller than a row of ((w + 1) / 2) * 4 bytes")
    b = new(); b.pitch_y = 2 * W; b.pitch_c = 4 * cw; assert check(b)[0] == 0                                      # the tight pitches
    b = image(chroma, W - 1, H); b.pitch_c = 4 * cw - 4; refused(b, "the cbcr pitch is smaller")                   # odd w: the last pair is whole
    b = new(); b.pitch_y += 1; refused(b, "the y pitch is not a multiple of 2 bytes")
    b = new(); b.pitch_c += 1; refused(b, "the cbcr pitch is not a multiple of 2 bytes")
    b = new(); b.pitch_y = 1 << 31; refused(b, "the y pitch exceeds INT32_MAX")                                    # only the descriptor is read
    b = new(); b.pitch_c = 1 << 31; refused(b, "the cbcr pitch exceeds INT32_MAX")
    b = new(); b.w = 1 << 14; b.h = (1 << 13) + 1; b.pitch_y = b.pitch_c = b.w * 2; refused(b, "image too large (more than 2^27 pixels)")
    b = new(); b.w = 1; b.h = 1 << 20; b.pitch_y = 4096; b.pitch_c = 4; refused(b, "the y plane: rows * pitch reaches 2^32 bytes")
    b = new(); b.w = 1; b.h = 1 << 21; b.pitch_y = 2; b.pitch_c = 4096; refused(b, "the cbcr plane: rows * pitch reaches 2^32 bytes")
    b = new(); b.w = 1; b.h = 1 << 20; b.pitch_y = 4094; b.pitch_c = 4; assert check(b)[0] == 0                   # one short of 2^32
    refused(None, "null descriptor")


def test_argument_checks_come_before_the_device():
    """-EINVAL for every argument fault of the two calls, with or without a device and whatever the engine handle is (null here: no engine is needed to get there); a
    sound call on a box without a device then gets -ENODEV, on a box with one the null engine is the next -EINVAL."""
    L = amd.lib()
    err = lambda: L.rife_hip_last_error().decode()
    br = lambda d: ctypes.byref(d) if d is not None else None
    calls = {
        "host": lambda a, b, o: L.rife_hip_process_hbd_semiplanar(None, br(a), br(b), 0.5, br(o)),
        "device": lambda a, b, o: L.rife_hip_process_device_hbd_semiplanar(None, br(a), br(b), 0.5, br(o), None),
    }
    for name, call in calls.items():
        for chroma in (1, 2):
            a, b, o = image(chroma), image(chroma, pad=0), image(chroma, pad=9)
            assert call(None, b, o) == -amd.EINVAL and err().startswith("high bit depth: image 0: null descriptor"), (name, err())
            assert call(a, None, o) == -amd.EINVAL and err().startswith("high bit depth: image 1: null descriptor")
            assert call(a, b, None) == -amd.EINVAL and err().startswith("high bit depth: image out: null descriptor")
            bad = image(chroma); bad.depth = 9
            assert call(bad, b, o) == -amd.EINVAL and "image 0: the depth (9) is not in 10..16" in err()
            bad = image(chroma); bad.pitch_c = 2
            assert call(a, bad, o) == -amd.EINVAL and "image 1: the cbcr pitch is smaller than a row" in err()
            bad = image(chroma); bad.y = None
            assert call(a, b, bad) == -amd.EINVAL and "image out: null y pointer" in err()
            bad = image(chroma); bad.chroma = 3
            assert call(a, b, bad) == -amd.EINVAL and "image out: chroma 3: 4:4:4 semi-planar" in err()
            bad = image(chroma); bad.csp = amd.CSP_FULL
            assert call(bad, b, o) == -amd.EINVAL and "image 0: RIFE_HIP_CSP_FULL" in err()
            # the three images agree in w, h, chroma, csp and depth
            assert call(a, image(chroma, W + 1, H), o) == -amd.EINVAL and "image 0 and image 1 differ in size" in err()
            assert call(a, b, image(chroma, W, H + 1)) == -amd.EINVAL and "image 0 and image out differ in size" in err()
            assert call(a, image(3 - chroma), o) == -amd.EINVAL and "image 0 and image 1 differ in chroma" in err()
            assert call(a, b, image(3 - chroma)) == -amd.EINVAL and "image 0 and image out differ in chroma" in err()
            assert call(a, image(chroma, csp=amd.CSP_BT601), o) == -amd.EINVAL and "image 0 and image 1 differ in csp" in err()
            assert call(a, b, image(chroma, csp=amd.CSP_BT2020NCL)) == -amd.EINVAL and "image 0 and image out differ in csp" in err()
            assert call(a, image(chroma, depth=16), o) == -amd.EINVAL and "image 0 and image 1 differ in depth" in err()
            assert call(a, b, image(chroma, depth=10)) == -amd.EINVAL and "image 0 and image out differ in depth" in err()
            rc = call(a, b, o)
            assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL), (name, rc, err())      # -RIFE_HIP_ENODEV / "null engine"
            assert ("no HIP device" in err()) if amd.device_count() < 1 else ("null engine" in err())


def test_reference_helpers():
    """a check of the REFERENCE (tests/semiplanar_ref.py), which the GPU tests compare the library with: it needs no library call beyond the descriptors"""
    rng = np.random.default_rng(5)
    for chroma in (1, 2):
        for depth in (10, 12, 16):
            s = 16 - depth
            w, h = 35, 17
            ch, cw2 = sr.chroma_shape(w, h, chroma)
            assert (ch, cw2) == ((9 if chroma == 1 else 17), 36)
            a, b = sr.surfaces(w, h, chroma, depth, 3, pad=6, offset=1)
            assert a[0].shape == (h, w) and a[1].shape == (ch, cw2) and a[0].dtype == np.uint16 and a[0].ctypes.data % 4 == 2 and a[1].ctypes.data % 4 == 2
            assert a[0].strides == ((w + 7) * 2, 2) and a[1].strides == ((cw2 + 7) * 2, 2) and any((p != q).any() for p, q in zip(a, b))
            if s:
                assert (a[0] & ((1 << s) - 1)).any() and (a[1] & ((1 << s) - 1)).any(), "no garbage in the low bits"
            planes = sr.split(a, depth)
            assert [p.shape for p in planes] == [(h, w), (ch, cw2 // 2), (ch, cw2 // 2)] and all(p.flags.c_contiguous and int(p.max()) <= (1 << depth) - 1 for p in planes)
            assert np.array_equal(planes[1], a[1][:, 0::2] >> s) and np.array_equal(planes[2], a[1][:, 1::2] >> s)
            # split and join are inverse on codes, and garbage low bits vanish
            j = sr.join(planes, depth)
            assert np.array_equal(j[0], (a[0] >> s) << s) and np.array_equal(j[1], (a[1] >> s) << s) and all(p.flags.c_contiguous for p in j)
            assert all(np.array_equal(p, q) for p, q in zip(sr.split(j, depth), planes))
            codes = [rng.integers(0, 1 << depth, p.shape, dtype=np.uint32).astype(np.uint16) for p in planes]
            assert all(np.array_equal(p, q) for p, q in zip(sr.split(sr.join(codes, depth), depth), codes))
            assert not any((p & ((1 << s) - 1)).any() for p in sr.join(codes, depth))
            clean = sr.surfaces(w, h, chroma, depth, 3, low_bits=False)[0]
            assert all(np.array_equal(p, q) for p, q in zip(sr.split(clean, depth), planes)), "the low bits changed the codes"
            o = sr.blank_like(a)
            assert all(p.shape == q.shape and p.strides == q.strides and p.ctypes.data % 4 == 2 and (p == sr.SENTINEL).all() for p, q in zip(o, a)) and sr.untouched(o)
            o[0][...] = 7; o[1][...] = 9
            assert sr.untouched(o)
            sr.big(o[1])[0, 0] = 7
            assert not sr.untouched(o)
    assert sr.pixfmt(1) == amd.PIX_I420P10 and sr.pixfmt(2, amd.CSP_BT2020NCL) == amd.PIX_I422P10 | amd.CSP_BT2020NCL
    r0, r1 = sr.random_surfaces(9, 5, 1, rng, pad=4, multiple=8)
    assert r0[0].strides[0] == 32 and r0[1].strides[0] == 32 and r0[0].ctypes.data % 64 == 0 and (r0[0] != r1[0]).any()
    odd = sr.surface(9, 5, 2, pad=2, offset=1, odd=True)
    assert odd[0].strides[0] == 26 and odd[1].strides[0] == 26 and odd[1].shape == (5, 10)


def test_python_surface():
    (y, c), (y1, c1) = sr.surfaces(W, H, 1, 12, 5, pad=3)
    d = amd.semiplanar_of(y, c, 12, 1, amd.CSP_BT601)
    assert (d.w, d.h, d.chroma, d.csp, d.depth, d.pitch_y, d.pitch_c, d.y, d.cbcr) == (W, H, 1, amd.CSP_BT601, 12, (W + 3) * 2, (W + 3) * 2, y.ctypes.data, c.ctypes.data)
    amd.semiplanar_check(y, c, W, H, 1, 12)
    amd.semiplanar_check(y, c, W, H, 1, 12, amd.CSP_BT2020NCL)
    amd.semiplanar_check(d)
    with pytest.raises(amd.RifeError, match=r"\(-1\).*the depth \(18\) is not in 10\.\.16"):
        amd.semiplanar_check(y, c, W, H, 1, 18)
    with pytest.raises(amd.RifeError, match=r"\(-1\).*RIFE_HIP_CSP_FULL"):
        amd.semiplanar_check(y, c, W, H, 1, 12, amd.CSP_FULL)
    with pytest.raises(ValueError, match="the luma array is not"):
        amd.semiplanar_check(y, c, W + 1, H, 1, 12)
    c2 = np.zeros(sr.chroma_shape(W, H, 2), np.uint16)
    amd.semiplanar_check(y, c2, W, H, 2, 12)
    for by, bc, chroma in ((y.astype(np.uint8), c, 1), (y, c.astype(np.float32), 1), (y, c2, 1), (y, c, 2), (y, c[:, :-2], 1), (y[:, ::2], c, 1), (y, c[:, ::2], 1), (y[0], c, 1),
                           (np.zeros((0, 4), np.uint16), np.zeros((0, 4), np.uint16), 1), ([1, 2], c, 1), (y, c, 3)):
        with pytest.raises(ValueError, match=r"uint16 array of shape \(h, w\) and one of shape \(ch, 2 \* cw\)"):
            amd.semiplanar_of(by, bc, 12, chroma)
    ro = c.copy(); ro.flags.writeable = False
    with pytest.raises(ValueError, match="out: a writable uint16 array"):
        amd.semiplanar_of(y, ro, 12, 1, 0, "out", writable=True)
    g = amd.RIFE.__new__(amd.RIFE)      # the argument checks of the method come before the engine is looked at
    with pytest.raises(ValueError, match="in1: a uint16 array"):
        amd.RIFE.process_hbd_semiplanar(g, (y, c), (y1, c1.astype(np.float32)), 0.5, 12, 1)
    with pytest.raises(ValueError, match=r"in1: a pair \(y, cbcr\)"):
        amd.RIFE.process_hbd_semiplanar(g, (y, c), y1, 0.5, 12, 1)
    with pytest.raises(ValueError, match="out: a writable uint16 array"):
        amd.RIFE.process_hbd_semiplanar(g, (y, c), (y1, c1), 0.5, 12, 1, out=(y.copy(), ro))
    for name in ("process_hbd_semiplanar", "process_device_hbd_semiplanar"):
        assert callable(getattr(amd.RIFE, name))
    assert callable(amd.op_sp_to_rgb10) and callable(amd.op_apply_sp) and callable(amd.semiplanar_desc)
    src = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "rife.h")).read()
    assert re.search(r"int process_hbd_semiplanar\(const rife_hip_semiplanar_t& in0, const rife_hip_semiplanar_t& in1, float timestep, const rife_hip_semiplanar_t& out\) const;", src)


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "sanitize", "semiplanar_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "semiplanar_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"semiplanar_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 4000 and int(m.group(2)) == 0, p.stdout[-500:]
    print(p.stdout.splitlines()[-1])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_makefile_builds_the_same_program():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../semiplanar-check-asan:"):].split("\n", 2)
    for dep in ("semiplanar_check_main.cpp", "semiplanar_check.h", "rife_hip.h"):
        assert dep in rule[0], dep
    for f in SAN[2:]:
        assert f in rule[1]
    line = mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
    assert "../semiplanar-check-asan" in line and "semiplanar-check-asan" in mk[mk.index("\nclean:"):]
