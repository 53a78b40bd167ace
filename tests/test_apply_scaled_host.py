"""Apply motion at another resolution (include/rife_hip.h rife_hip_apply_set_t), the part that needs no device: rife_hip_apply_set_check through ctypes on the PRODUCT
library, every rule by its words; the argument checks of the four sets calls, which come before "no device"; the struct and the symbols; the Python surface;
tests/sanitize/apply_set_check_main.cpp, a program of its own under ASan + UBSan over csrc/apply_set_check.h; and the conditions the GPU tests
(tests/test_gpu_apply_scaled.py) rest on, checked against the reference alone - every dense case's boundary share is under the cap, every planted case is exact in
float32 numpy, and the planted resampled motion is the same in float32 and float64."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import apply_ref as ar
import apply_scaled_ref as asr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MW, MH = 33, 47
_DT = {amd.SAMPLE_U8: np.uint8, amd.SAMPLE_U16: np.uint16, amd.SAMPLE_F16: np.float16, amd.SAMPLE_F32: np.float32}
_sid = lambda s: asr.SHIFT_ID[tuple(s)]


def planes(sample, w, h, n=2, pad=6):
    a = np.zeros((n, h, w + pad), _DT[sample])
    return tuple(a[k, :, :w] for k in range(n))


def good(shift, sample=amd.SAMPLE_U16, mw=MW, mh=MH, which=0, **kw):
    w, h = asr.plane_sizes(tuple(shift), mw, mh)[which]
    return amd.apply_set(planes(sample, w, h), planes(sample, w, h), shift, out=planes(sample, w, h), **kw)


def check(s, mw=MW, mh=MH):
    L = amd.lib()
    rc = L.rife_hip_apply_set_check(ctypes.byref(s) if s is not None else None, mw, mh)
    return rc, L.rife_hip_last_error().decode()


def refused(s, word, mw=MW, mh=MH):
    rc, msg = check(s, mw, mh)
    assert rc == -amd.EINVAL and word in msg, (rc, msg)


def test_struct_symbols_and_header():
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    # three pointers, then four ints: 40 bytes on this ABI
    assert re.search(r"const rife_hip_planes_t\* p0; const rife_hip_planes_t\* p1; const rife_hip_planes_t\* out;\s*int shift_x, shift_y;[^}]*int wp, hp;[^}]*\} rife_hip_apply_set_t;", hdr, re.S)
    S = amd.rife_hip_apply_set
    assert ctypes.sizeof(S) == 40 and (S.p0.offset, S.p1.offset, S.out.offset, S.shift_x.offset, S.shift_y.offset, S.wp.offset, S.hp.offset) == (0, 8, 16, 24, 28, 32, 36)
    names = ("rife_hip_apply_set_check", "rife_hip_apply_device_motion_sets", "rife_hip_apply_motion_sets", "rife_hip_process_apply_sets", "rife_hip_process_device_apply_sets")
    for s in names:
        assert s in amd.C_ABI_SYMBOLS and hasattr(amd.lib(), s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert "rife_hip_op_apply_scaled" in amd.TEST_ABI_SYMBOLS and "rife_hip_op_apply_scaled" not in amd.C_ABI_SYMBOLS
    assert re.search(r"\brife_hip_op_apply_scaled\s*\(", open(os.path.join(ROOT, "include", "rife_hip_test.h")).read())
    assert not hasattr(amd.lib(), "rife_hip_op_apply_scaled")
    # the clause this section delivers is gone from the apply section's "Out of scope"
    assert "planes at another resolution than the motion" not in hdr


@pytest.mark.parametrize("shift", [(0, 0)] + asr.SHIFTS, ids=_sid)
def test_set_check_rules(shift):
    for sample in (0, 1, 2, 3):
        for mw, mh in asr.TINY + asr.SIZES[:1]:
            for which in range(len(asr.plane_sizes(shift, mw, mh))):
                g = good(shift, sample, mw, mh, which)
                assert check(g, mw, mh)[0] == 0, (shift, sample, mw, mh, check(g, mw, mh))
    g = good(shift)
    w, h = g.p0.contents.w, g.p0.contents.h
    # the size must fit THIS motion
    refused(g, "does not fit a motion of %d x %d at shift (%d, %d)" % (MW + 2, MH, shift[0], shift[1]), MW + 2, MH)
    refused(g, "does not fit a motion of", MW, MH + 2)
    refused(g, "bad motion size", 0, MH)
    refused(g, "bad motion size", MW, -3)
    # the extent, in plane pixels
    for ext in ((w, h), ar.padded(w, h, 64), asr.frame_extent(shift, MW, MH)):
        assert check(good(shift, extent=ext))[0] == 0, ext
    refused(good(shift, extent=(w - 1, h)), "the extent (%d x %d) is neither 0, 0 nor at least the plane size" % (w - 1, h))
    refused(good(shift, extent=(w, 0)), "the extent")
    refused(good(shift, extent=(2 ** 14, 2 ** 13 + 1)), "the extent is too large")
    # the descriptors: the rules of rife_hip_planes_check, by set member
    b = good(shift); b.p1.contents.pitch[0] = 2; refused(b, "planes 1: plane 0: the pitch (2) is smaller")
    b = good(shift); b.out.contents.maxval = 1023; refused(b, "the three plane sets differ in w, h, n, sample or maxval")
    b = good(shift); b.p0.contents.n = 1; refused(b, "the three plane sets differ")
    b = good(shift); b.p0 = None; refused(b, "planes 0: null planes descriptor")
    b = good(shift); b.out = None; refused(b, "planes out: null planes descriptor")
    refused(None, "null set")


def test_shift_pairs():
    for sx in (-2, -1, 0, 1, 2):
        for sy in (-2, -1, 0, 1, 2):
            g = good((0, 0)); g.shift_x, g.shift_y = sx, sy
            if (sx, sy) in [(0, 0)] + asr.SHIFTS:
                continue
            refused(g, "the shift pair (%d, %d) is not one of (0, 0), (-1, -1), (-1, 0), (1, 1)" % (sx, sy))
    # explicit on purpose: at mw = 1 a plane of width 1 fits shift 0 and shift -1
    for shift in ((0, 0), (-1, -1), (-1, 0)):
        one = amd.apply_set(planes(1, 1, 1), planes(1, 1, 1), shift, out=planes(1, 1, 1))
        assert check(one, 1, 1)[0] == 0
    # the up shift takes 2 m and 2 m - 1, nothing else; the down shifts (m + 1) / 2
    for w, ok in ((2 * MW - 2, False), (2 * MW - 1, True), (2 * MW, True), (2 * MW + 1, False)):
        s = amd.apply_set(planes(1, w, 2 * MH), planes(1, w, 2 * MH), (1, 1), out=planes(1, w, 2 * MH))
        assert (check(s)[0] == 0) == ok, w
        if not ok:
            refused(s, "which takes planes of %d or %d x %d or %d" % (2 * MW - 1, 2 * MW, 2 * MH - 1, 2 * MH))
    s = amd.apply_set(planes(1, MW // 2, MH), planes(1, MW // 2, MH), (-1, 0), out=planes(1, MW // 2, MH))
    refused(s, "which takes planes of %d x %d" % ((MW + 1) // 2, MH))
    # a (-1, 0) set is not a (-1, -1) set
    g = good((-1, 0)); g.shift_y = -1; refused(g, "does not fit a motion of")


def _motion(w=MW, h=MH, fmt=0):
    dt = np.float32 if fmt == 0 else np.float16
    f = np.zeros((h, w, 4), dt); m = np.zeros((h, w), dt)
    d = amd.motion_desc(f.ctypes.data, m.ctypes.data, fmt, f.strides[0], m.strides[0])
    d._keep = (f, m)
    return d


def test_argument_checks_come_before_the_device():
    """-EINVAL for every argument fault of the four sets calls, with or without a device (no engine is needed to get there); a sound call on a box without a device
    then gets -ENODEV, on a box with one the null engine is the next -EINVAL."""
    L = amd.lib()
    err = lambda: L.rife_hip_last_error().decode()
    br = lambda d: ctypes.byref(d) if d is not None else None
    a = np.zeros((MH, MW, 3), np.uint8); o = np.zeros_like(a)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    m = _motion()
    sets = [good((0, 0), sample) for sample in (amd.SAMPLE_U16, amd.SAMPLE_F32)] + [good((-1, -1)), good((-1, 0)), good((0, 0))]      # sets may differ in everything

    def arr(ss):
        return amd._set_array(ss)

    calls = {
        "apply": lambda ss=sets[:4], mo=m, mw=MW, **kw: L.rife_hip_apply_motion_sets(None, arr(ss)[0], arr(ss)[1], br(mo), mw, MH),
        "apply_device": lambda ss=sets[:4], mo=m, mw=MW, **kw: L.rife_hip_apply_device_motion_sets(None, arr(ss)[0], arr(ss)[1], br(mo), mw, MH, None),
        "process": lambda ss=sets[:4], mo=None, mw=MW, px=amd.PIX_RGB8, i0=p(a): L.rife_hip_process_apply_sets(None, i0, p(a), mw, MH, 0.5, p(o), px, arr(ss)[0], arr(ss)[1]),
        "process_device": lambda ss=sets[:4], mo=None, mw=MW, px=amd.PIX_RGB8, i0=p(a): L.rife_hip_process_device_apply_sets(None, i0, p(a), mw, MH, 0.5, p(o), px, arr(ss)[0], arr(ss)[1], None),
    }
    up = good((1, 1), mw=MW + 1); bad_shift = good((0, 0)); bad_shift.shift_y = 1
    bad_planes = good((-1, -1)); bad_planes.p1.contents.pitch[1] = 2
    bad_extent = good((-1, -1), extent=(3, 3))
    for name, call in calls.items():
        assert call(ss=[]) == -amd.EINVAL and "the set count (0) is not in 1..4" in err(), (name, err())
        assert call(ss=sets) == -amd.EINVAL and "the set count (5) is not in 1..4" in err()
        assert call(ss=[sets[0], bad_shift]) == -amd.EINVAL and "set 1: the shift pair (0, 1)" in err(), (name, err())
        assert call(ss=[sets[0], sets[2], bad_planes]) == -amd.EINVAL and "set 2: planes 1: plane 1: the pitch (2) is smaller" in err()
        assert call(ss=[bad_extent]) == -amd.EINVAL and "set 0: the extent (3 x 3)" in err()
        assert call(ss=[sets[0], sets[1], sets[2], up]) == -amd.EINVAL and "set 3: the plane size" in err() and "does not fit a motion of" in err()
        assert call(mw=MW + 1) == -amd.EINVAL and "set 0: the plane size" in err()
        assert "apply motion" in err()
        if name.startswith("apply"):
            assert call(mo=None) == -amd.EINVAL and "motion: null motion descriptor" in err()
            half = _motion(); half.mask = None
            assert call(mo=half) == -amd.EINVAL and "needs both flow and mask" in err()
            assert call(mo=_motion(MW - 1, MH)) == -amd.EINVAL and "motion: flow: the pitch" in err()
            assert call(mo=_motion(fmt=1)) in (-2, -amd.EINVAL)      # F16 motion is accepted: the next answer is the device's or the engine's
        else:
            assert call(px=3) == -amd.EINVAL and "unknown pixel format" in err()
            assert call(i0=None) == -amd.EINVAL and "null pointer" in err()
            assert call(mw=0) == -amd.EINVAL
        rc = call()
        assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL), (name, rc, err())      # -RIFE_HIP_ENODEV / "null engine"
    # the host call takes a null frame ("not wanted"); the device call does not
    n, ar_ = arr(sets[:2])
    rc = L.rife_hip_process_apply_sets(None, p(a), p(a), MW, MH, 0.5, None, 0, n, ar_)
    assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL) and "null pointer" not in err()
    assert L.rife_hip_process_device_apply_sets(None, p(a), p(a), MW, MH, 0.5, None, 0, n, ar_, None) == -amd.EINVAL and "null pointer" in err()


def test_python_surface():
    a = np.zeros((2, MH, MW + 5), np.uint16)
    w2, h2 = (MW + 1) // 2, (MH + 1) // 2
    c0, c1 = np.zeros((2, h2, w2), np.uint16), np.ones((2, h2, w2), np.uint16)
    s = amd.apply_set(c0, c1, shift=(-1, -1), maxval=4095, extent=(32, 32))
    assert (s.shift_x, s.shift_y, s.wp, s.hp) == (-1, -1, 32, 32)
    assert s.p0.contents.maxval == s.out.contents.maxval == 4095 and s.out.contents.n == 2 and s.p1.contents.plane[0] == c1.ctypes.data
    assert len(s.planes) == 2 and s.planes[0].shape == (h2, w2) and s.planes[0].dtype == np.uint16 and s.out.contents.plane[1] == s.planes[1].ctypes.data
    amd.apply_set_check(s, MW, MH)
    with pytest.raises(amd.RifeError, match="does not fit a motion of"):
        amd.apply_set_check(s, MW, MH + 2)
    o = np.zeros((2, MH, MW + 5), np.uint16)
    s0 = amd.apply_set(a[:, :, :MW], a[:, :, :MW], out=o[:, :, :MW])      # defaults: shift (0, 0), extent 0, 0, written in place
    assert (s0.shift_x, s0.shift_y, s0.wp, s0.hp) == (0, 0, 0, 0) and s0.out.contents.pitch[0] == (MW + 5) * 2 and s0.planes[1].ctypes.data == o[1].ctypes.data
    amd.apply_set_check(s0, MW, MH)
    d = amd.planes_desc(w2, h2, amd.SAMPLE_F32, [(4096, w2 * 4)])
    sd = amd.apply_set_desc(d, d, d, (-1, 0), (64, 64))
    assert (sd.shift_x, sd.shift_y, sd.wp, sd.hp) == (-1, 0, 64, 64) and sd.p0.contents.plane[0] == 4096
    n, arr = amd._set_array([s, s0, sd])
    assert n == 3 and arr[1].out.contents.pitch[0] == (MW + 5) * 2 and arr[2].shift_y == 0
    for name in ("apply_motion_sets", "apply_device_motion_sets", "process_apply_sets", "process_device_apply_sets"):
        assert callable(getattr(amd.RIFE, name))
    assert callable(amd.op_apply_scaled)
    with pytest.raises(ValueError, match="uint8, uint16, float16 or float32"):
        amd.apply_set(np.zeros((1, 4, 4), np.float64), np.zeros((1, 4, 4), np.float64))


# ---- the conditions the GPU tests rest on, against the reference alone ------------------------------------------------------------------------------------------------
def test_resample_by_hand():
    """the definition on a motion small enough to write out"""
    f = np.arange(3 * 3 * 4, dtype=np.float32).reshape(3, 3, 4); m = (np.arange(9, dtype=np.float32).reshape(3, 3) + 1) / 16
    f2, m2 = asr.resample(f, m, asr.SHIFT_420, 2, 2)
    assert m2[0, 0] == ((m[0, 0] + m[0, 1]) + (m[1, 0] + m[1, 1])) * np.float32(0.25) and m2[1, 1] == m[2, 2] and m2[0, 1] == (m[0, 2] + m[1, 2]) * np.float32(0.5)
    assert f2[1, 0, 1] == (f[2, 0, 1] + f[2, 1, 1]) * np.float32(0.5) * np.float32(0.5)      # an odd edge: the mean of the samples that exist, then the halved scale
    f2, m2 = asr.resample(f, m, asr.SHIFT_422, 2, 3)
    assert f2[1, 0, 0] == (f[1, 0, 0] + f[1, 1, 0]) * np.float32(0.5) * np.float32(0.5) and f2[1, 0, 1] == (f[1, 0, 1] + f[1, 1, 1]) * np.float32(0.5) and m2[2, 1] == m[2, 2]
    f2, m2 = asr.resample(f, m, asr.SHIFT_UP, 6, 5)
    assert m2[0, 0] == m[0, 0] and m2[0, 5] == m[0, 2]      # clamped corners: 0.75 a + 0.25 a twice, exact on this grid
    H = lambda r, j, jn: m[r, j] * np.float32(0.75) + m[r, jn] * np.float32(0.25)
    assert m2[3, 2] == H(1, 1, 0) * np.float32(0.75) + H(2, 1, 0) * np.float32(0.25) and m2[2, 3] == H(1, 1, 2) * np.float32(0.75) + H(0, 1, 2) * np.float32(0.25)
    Hf = lambda r: f[r, 0, 2] * np.float32(0.75) + f[r, 1, 2] * np.float32(0.25)
    assert f2[4, 1, 2] == (Hf(2) * np.float32(0.75) + Hf(1) * np.float32(0.25)) * np.float32(2) == 48      # an even row leans on the row above; displacements double
    f0, m0 = asr.resample(f, m, (0, 0), 3, 3)
    assert np.array_equal(f0, f) and np.array_equal(m0, m)


def _all_sizes(shift):
    return [(mw, mh, ws, hs) for mw, mh in asr.SIZES for ws, hs in asr.plane_sizes(shift, mw, mh)]


@pytest.mark.parametrize("shift", asr.SHIFTS, ids=_sid)
def test_dense_boundary_share_is_under_the_cap(shift):
    for sample, maxval in ar.DENSE_KINDS[:3]:
        for mw, mh, ws, hs in _all_sizes(shift):
            for ext in asr.extents(shift, mw, mh, ws, hs)[:2]:
                c = asr.cached("dense", shift, mw, mh, ws, hs, 2, sample, maxval, ext)
                print("dense %s %s/%d motion %dx%d planes %dx%d extent %s: boundary set %.4f of the samples (seed %d), max |flow'| %.2f" % (
                    _sid(shift), sample, maxval, mw, mh, ws, hs, ext, c["boundary_frac"], c["seed"], np.abs(c["flow"]).max()))
                assert c["boundary_frac"] < ar.CAP
                assert np.abs(c["flow"]).max() > 2.0 and 0.0 < c["mask"].min() and c["mask"].max() < 1.0, "a case without motion checks nothing"


@pytest.mark.parametrize("shift", asr.SHIFTS, ids=_sid)
def test_planted_cases_are_exact_in_float32(shift):
    for sample, maxval in ((0, 255), (1, 1023), (1, 65535), (2, 0), (3, 0)):
        for mw, mh in asr.TINY + asr.SIZES:
            for ws, hs in asr.plane_sizes(shift, mw, mh):
                for ext in (asr.extents(shift, mw, mh, ws, hs)[0], asr.extents(shift, mw, mh, ws, hs)[2]):
                    for half in (False, True):
                        c = asr.cached("planted", shift, mw, mh, ws, hs, 2, sample, maxval, ext, half)
                        f64, m64 = asr.resample64(c["mflow"], c["mmask"], shift, ws, hs)
                        assert np.array_equal(c["flow"].astype(np.float64), f64) and np.array_equal(c["mask"].astype(np.float64), m64), "the resampled motion is not exact"
                        assert ar.exact_in_float32(c), (shift, sample, maxval, mw, mh, ws, hs, ext, half)
                        want = ar.expected_exact(c["ref"], sample, maxval)
                        assert want.dtype == _DT[sample] and want.shape == c["p0"].shape


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "sanitize", "apply_set_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "apply_set_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"apply_set_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 3000 and int(m.group(2)) == 0, p.stdout[-500:]
    print(p.stdout.splitlines()[-1])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_makefile_builds_the_same_program():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../apply-set-check-asan:"):].split("\n", 2)
    assert "apply_set_check_main.cpp" in rule[0] and "apply_set_check.h" in rule[0] and "apply_check.h" in rule[0] and "motion_check.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1]
    line = mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
    assert line.index("../apply-check-asan") < line.index("../apply-set-check-asan")
