"""Planar RGB (RIFE_HIP_PIX_RGBP8 / RGBP10 / RGBPH / RGBPF), the part that needs no device: the format numbers in the header, the Python mirror and
tests/planar_ref.py; rife_hip_frame_bytes / rife_hip_image_row_bytes / rife_hip_image_check through ctypes on the PRODUCT library; the identities of the
specification, exhaustive over the 1024 codes and the 256 bytes; the float conversion on the inputs where a fused multiply-add would give another code; and
tests/sanitize/planar_check_main.cpp, a program of its own under ASan + UBSan over the check and size functions."""
import ctypes
import importlib
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import planar_ref as pr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 1), (3, 5), (33, 47), (640, 360)]
CODES = np.arange(1024, dtype=np.int32)


def _id(px):
    return pr.NAMES[px]


def check(img):
    L = amd.lib()
    rc = L.rife_hip_image_check(ctypes.byref(img))
    return rc, L.rife_hip_last_error().decode()


def refused(img, word):
    rc, msg = check(img)
    assert rc == -1 and word in msg, (rc, msg)      # -RIFE_HIP_EINVAL


def good(px, w=33, h=47, pad=8):
    """A descriptor over three host planes in allocations of their own, with `pad` bytes of row padding each."""
    bufs = [np.zeros((h, w * pr.elem(px) + pad), np.uint8) for _ in range(3)]
    im = amd.device_image(w, h, px, [(b.ctypes.data, b.strides[0]) for b in bufs])
    im._keep = bufs
    return im


# ---- format numbers -----------------------------------------------------------------------------------------------------------------------------------

def test_format_numbers():
    want = (65, 67, 69, 71)
    assert pr.FORMATS == want == (amd.PIX_RGBP8, amd.PIX_RGBP10, amd.PIX_RGBPH, amd.PIX_RGBPF)
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    for name, v in zip(("RGBP8", "RGBP10", "RGBPH", "RGBPF"), want):
        assert re.search(r"#define RIFE_HIP_PIX_%s\s+%d\b" % (name, v), hdr), name
    # 16 * class + 2 * k + planar, class 4
    for k, (px, dt, es) in enumerate(zip(want, (np.uint8, np.uint16, np.float16, np.float32), (1, 2, 2, 4))):
        assert px == 16 * 4 + 2 * k + 1
        assert np.dtype(pr.dtype(px)) == np.dtype(amd.planar_rgb_dtype(px)) == np.dtype(dt) and pr.elem(px) == es == amd._ELEM[px]
    for bad in (amd.PIX_RGB8, amd.PIX_I444, 64, 66, 72, amd.PIX_RGBPF | amd.CSP_BT601):
        with pytest.raises(ValueError):
            amd.planar_rgb_dtype(bad)
    for px in want:                                   # the yuv_* helpers stay YUV-only
        with pytest.raises(ValueError):
            amd.yuv_dtype(px)
        with pytest.raises(ValueError):
            amd.yuv_frame_bytes(33, 47, px)


@pytest.mark.parametrize("px", [64, 66, 68, 70, 72, 73])
def test_neighbouring_numbers_stay_unknown(px):
    """The even slots of class 4 (packed float RGB and the like) and everything from 72 up."""
    assert amd.frame_bytes(33, 47, px) == 0
    for p in range(3):
        assert amd.image_row_bytes(33, px, p) == 0
    im = good(pr.PIX_RGBPF); im.pixfmt = px
    refused(im, "unknown pixel format")


# ---- frame bytes and row bytes, C against numpy -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("px", pr.FORMATS, ids=_id)
def test_frame_bytes_and_row_bytes(px, size):
    w, h = size
    es = pr.elem(px)
    frame = np.zeros((3, h, w), pr.dtype(px))
    assert amd.frame_bytes(w, h, px) == pr.frame_bytes(w, h, px) == frame.nbytes == 3 * w * h * es
    rb = [amd.image_row_bytes(w, px, p) for p in range(4)]
    assert rb == [frame[0, 0].nbytes] * 3 + [0] == [w * es] * 3 + [0]
    assert sum(rb) * h == amd.frame_bytes(w, h, px)
    assert amd.frame_bytes(0, h, px) == 0 and amd.frame_bytes(w, -1, px) == 0 and amd.image_row_bytes(0, px, 0) == 0
    # a tight image is accepted: the planes of the (3, h, w) array
    im = amd.device_image(w, h, px, [(frame[p].ctypes.data, frame.strides[1]) for p in range(3)])
    assert check(im)[0] == 0, check(im)


# ---- image rules ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.FORMATS, ids=_id)
def test_image_rules(px):
    w, h = 33, 47
    es = pr.elem(px)
    assert check(good(px))[0] == 0                                     # padded planes in three allocations
    for p in range(3):
        rb = amd.image_row_bytes(w, px, p)
        im = good(px); im.pitch[p] = rb - es
        refused(im, "plane %d: the pitch (%d) is smaller than the row bytes (%d)" % (p, rb - es, rb))
        im = good(px); im.pitch[p] = rb                                # the smallest pitch that passes
        assert check(im)[0] == 0
        im = good(px); im.plane[p] = None
        refused(im, "plane %d is NULL" % p)
        if es > 1:
            im = good(px); im.pitch[p] = rb + 64 + 1
            refused(im, "not a multiple of the element size (%d)" % es)
            im = good(px); im.plane[p] = im.plane[p] + 1
            refused(im, "not aligned to the element size (%d)" % es)
        else:
            im = good(px); im.pitch[p] = rb + 65; im.plane[p] = im.plane[p] + 1
            assert check(im)[0] == 0
        if es == 4:                                                    # half an element: fine for u16 / half, not for float
            im = good(px); im.pitch[p] = rb + 64 + 2
            refused(im, "not a multiple of the element size (4)")
            im = good(px); im.plane[p] = im.plane[p] + 2
            refused(im, "not aligned to the element size (4)")
        if es == 2:
            im = good(px); im.pitch[p] = rb + 2; im.plane[p] = im.plane[p] + 2
            assert check(im)[0] == 0
    for csp in (amd.CSP_BT601, amd.CSP_BT2020NCL, amd.CSP_FULL, amd.CSP_FULL | amd.CSP_BT601):
        im = good(px); im.pixfmt = px | csp
        refused(im, "colour description")
    im = good(px); im.pixfmt = px | (1 << 13)
    refused(im, "unknown pixel format")


def test_plane_tuples_of_the_mirror():
    w, h = 33, 47
    for px in pr.FORMATS:
        dt = pr.dtype(px)
        es = pr.elem(px)
        r = np.zeros((h, 64), dt)[:, :w]; g = np.zeros((h, 40), dt)[:, :w]; b = np.zeros((h, w), dt)
        im = amd.planes_image((r, g, b), w, h, px)
        assert [im.pitch[i] for i in range(3)] == [64 * es, 40 * es, w * es] and check(im)[0] == 0
        chw = np.zeros((3, h, w), dt)                                   # one (3, h, w) array stands for its planes
        im = amd.planes_image(chw, w, h, px)
        assert [im.plane[i] for i in range(3)] == [chw[i].ctypes.data for i in range(3)] and check(im)[0] == 0
        with pytest.raises(ValueError):
            amd.planes_image((r, g), w, h, px)
        with pytest.raises(ValueError):
            amd.planes_image((r, g, np.zeros((h, w), np.int16)), w, h, px)
        with pytest.raises(ValueError):
            amd.planes_image((r, g, np.zeros((h, w + 1), dt)), w, h, px)
        with pytest.raises(ValueError):
            amd.planes_image((r, g, b), w, h, px | amd.CSP_BT601)
    # image_of() does not guess a planar layout from a transposed view
    hwc = np.zeros((h, w, 3), np.uint8)
    assert amd.image_of(hwc.transpose(2, 0, 1)) is None and amd.image_of(np.zeros((3, h, w), np.float32)) is None


# ---- the identities of the specification, exhaustive -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("px", pr.FORMATS, ids=_id)
def test_every_code_survives_the_round_trip(px):
    """to10(from10(c)) == c for all 1024 codes: what makes the canonical form idempotent and lets the 1-code contract carry across."""
    s = pr.from10(CODES, px)
    assert s.dtype == pr.dtype(px)
    if px == pr.PIX_RGBP8:
        # from10 drops two bits: the identity holds on the codes to10 produces (bit replication), and c >> 2 is within one of any neighbour's
        produced = pr.to10(np.arange(256, dtype=np.uint8), px)
        assert np.array_equal(pr.to10(pr.from10(produced, px), px), produced)
        assert np.abs(np.diff(pr.from10(CODES, px).astype(np.int32))).max() == 1
    else:
        assert np.array_equal(pr.to10(s, px), CODES)
    assert np.array_equal(pr.canonical(pr.canonical(s, px), px), pr.canonical(s, px))


def test_eight_bit_values_come_back():
    v = np.arange(256, dtype=np.uint8)
    c = pr.to10(v, pr.PIX_RGBP8)
    assert np.array_equal(c, (v.astype(np.int32) << 2) | (v >> 6)) and c[0] == 0 and c[255] == 1023
    assert np.array_equal(pr.from10(c, pr.PIX_RGBP8), v)                               # u8 -> 10 -> u8 is the identity
    assert np.array_equal(pr.canonical(v, pr.PIX_RGBP8), v)
    # an 8-bit value carried as the float v / 255.f comes back as a float that rounds to v
    f = (v.astype(np.float32) / np.float32(255)).astype(np.float32)
    back = pr.canonical(f, pr.PIX_RGBPF)
    assert back.dtype == np.float32
    assert np.array_equal(np.rint(back.astype(np.float64) * 255.0).astype(np.int32), v.astype(np.int32))
    # a 10-bit code carried as float or half c / 1023 is read as c
    assert np.array_equal(pr.to10((CODES / 1023.0).astype(np.float32), pr.PIX_RGBPF), CODES)
    assert np.array_equal(pr.to10((CODES / 1023.0).astype(np.float16), pr.PIX_RGBPH), CODES)


def test_ten_bit_samples_above_1023_and_float_specials():
    big = np.array([0, 1023, 1024, 4095, 65535], np.uint16)
    assert pr.to10(big, pr.PIX_RGBP10).tolist() == [0, 1023, 1023, 1023, 1023]
    assert pr.canonical(big, pr.PIX_RGBP10).tolist() == [0, 1023, 1023, 1023, 1023]
    sp = np.array([np.nan, -np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1.0, 1.5, 3e38, 1e-30, 0.5 / 1023 - 1e-9, 0.5 / 1023 + 1e-9], np.float32)
    want = [0, 0, 1023, 0, 0, 0, 0, 1023, 1023, 1023, 0, 0, 1]
    assert pr.to10(sp, pr.PIX_RGBPF).tolist() == want
    canon = pr.canonical(sp, pr.PIX_RGBPF)
    assert not np.isnan(canon).any() and canon[0] == 0.0 and canon[2] == 1.0            # NaN comes back as 0, +inf as 1
    sh = np.array([np.nan, np.inf, -np.inf, -1.0, 1.0, 2.0, 65504.0, 6e-8], np.float16)
    assert pr.to10(sh, pr.PIX_RGBPH).tolist() == [0, 1023, 0, 0, 1023, 1023, 1023, 0]
    sn = np.array([0x7fa00000, 0xffa00000], np.uint32).view(np.float32)                  # signalling NaNs, both signs
    assert pr.to10(sn, pr.PIX_RGBPF).tolist() == [0, 0]


def test_division_is_not_a_multiplication_by_the_reciprocal():
    """(float)c / 1023.f and c * (1 / 1023.f) differ in 24 of the 1024 codes: from10 is the division."""
    div = pr.code_float(CODES)
    mul = (CODES.astype(np.float32) * (np.float32(1) / np.float32(1023))).astype(np.float32)
    assert int((div != mul).sum()) == 24
    # division correctly rounded: no float32 neighbour is nearer the rational c / 1023
    for c in range(1024):
        q = Fraction(int(c), 1023)
        d = abs(Fraction(float(div[c])) - q)
        for nb in (np.nextafter(div[c], np.float32(-1)), np.nextafter(div[c], np.float32(2))):
            assert d <= abs(Fraction(float(nb)) - q), c


# ---- the float conversion where contraction would show ------------------------------------------------------------------------------------------------------

def _two_step_exact(x):
    """The two-step formula with each step rounded to float32 ONCE from an exact value (a double holds x * 1023 and p + 0.5 exactly: 24 + 10 and 25 bits)."""
    x64 = np.minimum(np.maximum(x.astype(np.float64), 0.0), 1.0)
    p = (x64 * 1023.0).astype(np.float32)
    s = (p.astype(np.float64) + 0.5).astype(np.float32)
    return s.astype(np.int32)


def _fused(x):
    """What a contracted multiply-add would give: x * 1023 + 0.5 rounded once."""
    x64 = np.minimum(np.maximum(x.astype(np.float64), 0.0), 1.0)
    return (x64 * 1023.0 + 0.5).astype(np.float32).astype(np.int32)


def test_half_code_boundaries_follow_the_two_step_formula():
    b = pr.boundary_floats()
    assert b.shape == (1023, 3) and b.dtype == np.float32 and (np.diff(b, axis=1) > 0).all()
    got = pr.to10(b, pr.PIX_RGBPF)
    assert np.array_equal(got, _two_step_exact(b))
    k = np.arange(1023)[:, None]
    assert ((got == k) | (got == k + 1)).all()
    # for the record: how many of these inputs a fused multiply-add (one rounding) would convert differently.  Measured 0 of 3069, and 0 in 50 million random
    # values: p + 0.5 is exact (p and the sum share a binade, or the sum's is coarser and rounds where the fused form rounds), so the two forms agree in the
    # code even where they differ in the last bit of the sum.  The specification stays the two-step form; the kernels are compiled without contraction.
    print("boundary set: %d of %d inputs where a fused multiply-add differs" % (int((_fused(b) != got).sum()), b.size))
    # the same through half: every half value widens exactly, so all 65536 bit patterns are the exhaustive set (NaN reads as 0, the infinities clamp)
    allh = np.arange(65536, dtype=np.uint16).view(np.float16)
    wide = allh.astype(np.float32)
    finite = np.where(np.isnan(wide), np.float32(0), np.clip(wide, np.float32(-1), np.float32(2))).astype(np.float32)
    assert np.array_equal(pr.to10(allh, pr.PIX_RGBPH), _two_step_exact(finite))


@pytest.mark.parametrize("px", pr.FORMATS, ids=_id)
def test_frames_pack_and_convert(px):
    rng = np.random.default_rng(3)
    for (w, h) in [(1, 1), (3, 5), (33, 47)]:
        codes = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
        f = pr.from_rgb10(codes, px)
        assert f.shape == (3, h, w) and f.dtype == pr.dtype(px) and f.flags.c_contiguous and f.nbytes == pr.frame_bytes(w, h, px)
        back = pr.to_rgb10(f, px)
        assert back.shape == (h, w, 3) and back.dtype == np.uint16
        if px == pr.PIX_RGBP8:
            assert np.array_equal(back >> 2, codes >> 2)
        else:
            assert np.array_equal(back, codes)
        assert np.array_equal(pr.pack(*pr.split(f), px), f)


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------

SRC = os.path.join(ROOT, "tests", "sanitize", "planar_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_and_size_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "planar_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"planar_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) > 500 and int(m.group(2)) == 0, p.stdout[-500:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]


def test_the_makefile_builds_the_same_program_under_the_sanitizers():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../planar-check-asan:"):].split("\n", 2)
    assert "planar_check_main.cpp" in rule[0] and "image_check.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1], f
    assert "../planar-check-asan" in mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
