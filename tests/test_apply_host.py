"""Apply motion (include/rife_hip.h rife_hip_planes_t), the part that needs no device: rife_hip_planes_check through ctypes on the PRODUCT library, every rule by its
words; the 4 GB bound; the argument checks of the four apply calls, which come before "no device"; the struct and the symbols; the Python surface;
tests/sanitize/apply_check_main.cpp, a program of its own under ASan + UBSan over csrc/apply_check.h; and the conditions the GPU tests (tests/test_gpu_apply.py) rest
on, checked against the reference alone - every dense case's boundary share is under the cap, every planted and far case is exact in float32 numpy, and the CPU
oracle's flow and mask put through apply_ref on the u8 planes of its input frames reproduce the oracle's own quantised frame."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import apply_ref as ar
import motion_ref as mr
import tail_ref as tr

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 33, 47
_DT = {amd.SAMPLE_U8: np.uint8, amd.SAMPLE_U16: np.uint16, amd.SAMPLE_F16: np.float16, amd.SAMPLE_F32: np.float32}
_IDS = {0: "u8", 1: "u16", 2: "f16", 3: "f32"}


def good(sample, n=3, w=W, h=H, pad=6):
    """A descriptor over n host planes with `pad` samples of row padding each."""
    a = np.zeros((n, h, w + pad), _DT[sample])
    d = amd.planes_of(tuple(a[k, :, :w] for k in range(n)))
    d._keep = a
    return d


def clone(d):
    c = amd.rife_hip_planes()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(d))
    c._keep = d
    return c


def check(d):
    L = amd.lib()
    rc = L.rife_hip_planes_check(ctypes.byref(d) if d is not None else None)
    return rc, L.rife_hip_last_error().decode()


def refused(d, word):
    rc, msg = check(d)
    assert rc == -amd.EINVAL and word in msg, (rc, msg)


def test_header_numbers_struct_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "rife_hip.h")).read()
    for name, v in (("U8", 0), ("U16", 1), ("F16", 2), ("F32", 3)):
        assert re.search(r"#define RIFE_HIP_SAMPLE_%s\s+%d\b" % (name, v), hdr)
    assert (amd.SAMPLE_U8, amd.SAMPLE_U16, amd.SAMPLE_F16, amd.SAMPLE_F32) == (ar.SAMPLE_U8, ar.SAMPLE_U16, ar.SAMPLE_F16, ar.SAMPLE_F32) == (0, 1, 2, 3)
    for s in ("rife_hip_planes_check", "rife_hip_padded_size", "rife_hip_apply_device_motion", "rife_hip_apply_motion", "rife_hip_process_apply", "rife_hip_process_device_apply"):
        assert s in amd.C_ABI_SYMBOLS and hasattr(amd.lib(), s), s
    assert "rife_hip_op_apply" in amd.TEST_ABI_SYMBOLS and "rife_hip_op_apply" in open(os.path.join(ROOT, "include", "rife_hip_test.h")).read()
    # five ints, padding to the pointer, four pointers, four ptrdiff_t: the struct of the header on this ABI
    assert re.search(r"int w, h, n, sample, maxval;[^}]*void\* plane\[4\];[^}]*ptrdiff_t pitch\[4\];[^}]*\} rife_hip_planes_t;", hdr, re.S)
    assert ctypes.sizeof(amd.rife_hip_planes) == 24 + 32 + 32 and amd.rife_hip_planes.plane.offset == 24 and amd.rife_hip_planes.pitch.offset == 56


@pytest.mark.parametrize("sample", [0, 1, 2, 3], ids=lambda s: _IDS[s])
def test_planes_check_rules(sample):
    es = np.dtype(_DT[sample]).itemsize
    g = good(sample)
    assert check(g)[0] == 0, check(g)
    assert g.maxval == {0: 255, 1: 65535}.get(sample, 0) and g.n == 3 and g.pitch[0] == (W + 6) * es
    for n in (1, 4):
        assert check(good(sample, n))[0] == 0
    b = clone(g); b.w = 0; refused(b, "bad plane size")
    b = clone(g); b.h = -1; refused(b, "bad plane size")
    b = clone(g); b.n = 0; refused(b, "the plane count (0) is not in 1..4")
    b = clone(g); b.n = 5; refused(b, "the plane count (5) is not in 1..4")
    b = clone(g); b.sample = 4; refused(b, "unknown sample type")
    b = clone(g); b.sample = -1; refused(b, "unknown sample type")
    if sample in (0, 1):
        top = 255 if sample == 0 else 65535
        b = clone(g); b.maxval = 0; refused(b, "maxval (0) is not in 1..%d" % top)
        b = clone(g); b.maxval = top + 1; refused(b, "maxval (%d) is not in 1..%d" % (top + 1, top))
        b = clone(g); b.maxval = 1; assert check(b)[0] == 0
    else:
        b = clone(g); b.maxval = 1; refused(b, "maxval must be 0 for float samples")
    b = clone(g); b.plane[1] = None; refused(b, "plane 1: null pointer")
    b = clone(g); b.pitch[2] = 0; refused(b, "plane 2: the pitch is not positive")
    b = clone(g); b.pitch[0] = -g.pitch[0]; refused(b, "plane 0: the pitch is not positive")
    b = clone(g); b.pitch[0] = W * es - es; refused(b, "plane 0: the pitch (%d) is smaller than the row bytes (%d)" % (W * es - es, W * es))
    if es > 1:
        b = clone(g); b.pitch[1] += 1; refused(b, "plane 1: the pitch is not a multiple of the element size (%d)" % es)
        b = clone(g); b.plane[2] += 1; refused(b, "plane 2: the pointer is not aligned to the element size (%d)" % es)
    refused(None, "null planes descriptor")
    t = clone(g)      # tight rows are fine too
    for k in range(3):
        t.pitch[k] = W * es
    assert check(t)[0] == 0


@pytest.mark.parametrize("sample", [0, 1, 2, 3], ids=lambda s: _IDS[s])
def test_the_4_gb_bound(sample):
    """h * pitch < 2^32 per plane: the kernel addresses every plane with 32-bit byte offsets, as motion_check.h's buffers."""
    es = np.dtype(_DT[sample]).itemsize
    g = good(sample)
    under = (2 ** 32 - 1) // H // es * es
    assert under * H < 2 ** 32 <= (under + es) * H
    b = clone(g); b.pitch[1] = under; assert check(b)[0] == 0
    b = clone(g); b.pitch[1] = under + es; refused(b, "plane 1: h * pitch reaches 2^32")
    b = clone(g); b.h = 1; b.pitch[0] = 2 ** 32; refused(b, "plane 0: h * pitch reaches 2^32")


def _motion(w=W, h=H, fmt=0):
    dt = np.float32 if fmt == 0 else np.float16
    f = np.zeros((h, w, 4), dt); m = np.zeros((h, w), dt)
    d = amd.motion_desc(f.ctypes.data, m.ctypes.data, fmt, f.strides[0], m.strides[0])
    d._keep = (f, m)
    return d


def test_argument_checks_come_before_the_device():
    """-EINVAL for every argument fault of the four calls, with or without a device (no engine is needed to get there); a sound call on a box without a device then
    gets -ENODEV, on a box with one the null engine is the next -EINVAL."""
    L = amd.lib()
    err = lambda: L.rife_hip_last_error().decode()
    br = lambda d: ctypes.byref(d) if d is not None else None
    p0, p1, po, m = good(1), good(1), good(1), _motion()
    a = np.zeros((H, W, 3), np.uint8); o = np.zeros_like(a)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    calls = {
        "apply": lambda q0=p0, q1=p1, qo=po, mo=m, wp=0, hp=0, **kw: L.rife_hip_apply_motion(None, br(q0), br(q1), br(mo), wp, hp, br(qo)),
        "apply_device": lambda q0=p0, q1=p1, qo=po, mo=m, wp=0, hp=0, **kw: L.rife_hip_apply_device_motion(None, br(q0), br(q1), br(mo), wp, hp, br(qo), None),
        "process": lambda q0=p0, q1=p1, qo=po, mo=None, wp=0, hp=0, px=amd.PIX_RGB8, i0=p(a), w=W: L.rife_hip_process_apply(None, i0, p(a), w, H, 0.5, p(o), px, br(q0), br(q1), wp, hp, br(qo)),
        "process_device": lambda q0=p0, q1=p1, qo=po, mo=None, wp=0, hp=0, px=amd.PIX_RGB8, i0=p(a), w=W: L.rife_hip_process_device_apply(None, i0, p(a), w, H, 0.5, p(o), px, br(q0), br(q1), wp, hp, br(qo), None),
    }
    bad = clone(p0); bad.pitch[0] = 2
    other_n = good(1, 2); other_sample = good(0); other_max = clone(po); other_max.maxval = 1023; other_size = good(1, 3, W + 1, H)
    for name, call in calls.items():
        assert call(q0=None) == -amd.EINVAL and "planes 0: null planes descriptor" in err(), (name, err())
        assert call(q1=None) == -amd.EINVAL and "planes 1: null planes descriptor" in err()
        assert call(qo=None) == -amd.EINVAL and "planes out: null planes descriptor" in err()
        assert call(q0=bad) == -amd.EINVAL and "planes 0: plane 0: the pitch (2) is smaller" in err()
        for q in (other_n, other_sample, other_size):
            assert call(q1=q) == -amd.EINVAL and "the three plane sets differ in w, h, n, sample or maxval" in err(), (name, err())
        assert call(qo=other_max) == -amd.EINVAL and "the three plane sets differ" in err()
        assert call(wp=W - 1, hp=H) == -amd.EINVAL and "the extent (%d x %d) is neither 0, 0 nor at least the plane size" % (W - 1, H) in err()
        assert call(wp=W, hp=0) == -amd.EINVAL and "the extent" in err()
        assert call(wp=2 ** 14, hp=2 ** 13 + 1) == -amd.EINVAL and "the extent is too large" in err()
        assert "apply motion" in err()
        if name.startswith("apply"):
            assert call(mo=None) == -amd.EINVAL and "motion: null motion descriptor" in err()
            half = _motion(); half.mask = None
            assert call(mo=half) == -amd.EINVAL and "needs both flow and mask" in err()
            small = _motion(W - 1, H)
            assert call(mo=small) == -amd.EINVAL and "motion: flow: the pitch" in err()
            assert call(mo=_motion(fmt=1)) in (-2, -amd.EINVAL)      # F16 motion is accepted: the next answer is the device's or the engine's
        else:
            assert call(px=3) == -amd.EINVAL and "unknown pixel format" in err()
            assert call(i0=None) == -amd.EINVAL and "null pointer" in err()
            assert call(w=0) == -amd.EINVAL
            assert call(w=W + 1) == -amd.EINVAL and "the planes and the frames differ in size" in err()
        rc = call()
        assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL), (name, rc, err())      # -RIFE_HIP_ENODEV / "null engine"
    # the host call takes a null frame ("not wanted"); the device call does not
    rc = L.rife_hip_process_apply(None, p(a), p(a), W, H, 0.5, None, 0, br(p0), br(p1), 0, 0, br(po))
    assert rc == (-2 if amd.device_count() < 1 else -amd.EINVAL) and "null pointer" not in err()
    assert L.rife_hip_process_device_apply(None, p(a), p(a), W, H, 0.5, None, 0, br(p0), br(p1), 0, 0, br(po), None) == -amd.EINVAL and "null pointer" in err()
    wp, hp = ctypes.c_int(), ctypes.c_int()
    assert L.rife_hip_padded_size(None, W, H, ctypes.byref(wp), ctypes.byref(hp)) == -amd.EINVAL


def test_python_surface():
    a = np.zeros((3, H, W + 5), np.uint16)
    d = amd.planes_of(a[:, :, :W])      # one (n, h, w) array, a view with padded rows: described in place
    assert (d.w, d.h, d.n, d.sample, d.maxval) == (W, H, 3, amd.SAMPLE_U16, 65535)
    assert [d.plane[k] for k in range(3)] == [a[k].ctypes.data for k in range(3)] and d.pitch[0] == (W + 5) * 2
    amd.planes_check(d)
    d = amd.planes_of((a[0, :, :W], a[2, :, :W]), maxval=4095)
    assert d.n == 2 and d.maxval == 4095
    assert amd.planes_of(np.zeros((H, W), np.float16)).maxval == 0
    with pytest.raises(ValueError, match="uint8, uint16, float16 or float32"):
        amd.planes_of(np.zeros((1, H, W), np.float64))
    with pytest.raises(ValueError, match="1..4"):
        amd.planes_of(np.zeros((5, H, W), np.uint8))
    with pytest.raises(ValueError, match="whose rows are contiguous"):
        amd.planes_of((np.zeros((H, W), np.uint8), np.zeros((H, W + 1), np.uint8)))
    with pytest.raises(ValueError, match="whose rows are contiguous"):
        amd.planes_of((np.zeros((H, 2 * W), np.uint8)[:, ::2],))
    with pytest.raises(amd.RifeError, match="maxval"):
        amd.planes_check(amd.planes_desc(W, H, amd.SAMPLE_U8, [(a.ctypes.data, W)], maxval=256))
    with pytest.raises(ValueError, match="one dtype"):
        amd._motion_in(W, H, np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float16))
    with pytest.raises(ValueError, match=r"flow is \(h, w, 4\)"):
        amd._motion_in(W, H, np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.float32))


# ---- the conditions the GPU tests rest on, against the reference alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample,maxval", ar.DENSE_KINDS[:3], ids=lambda v: str(v))
def test_dense_boundary_share_is_under_the_cap(sample, maxval):
    for w, h in ar.SIZES[1:]:
        for ext in ((w, h), ar.padded(w, h)):
            c = ar.cached("dense", w, h, 3, sample, maxval, ext)
            print("dense %s/%d %dx%d extent %s: boundary set %.4f of the samples (seed %d), max tau %.3g, max amax %.2f" % (
                _IDS[sample], maxval, w, h, ext, c["boundary_frac"], c["seed"], c["ref"]["tau"].max(), c["ref"]["amax"].max()))
            assert c["boundary_frac"] < ar.CAP
            assert np.abs(c["flow"]).max() > 2.0 and 0.0 < c["mask"].min() and c["mask"].max() < 1.0, "a case without motion checks nothing"


def test_tau_is_the_docstrings_formula():
    c = ar.cached("dense", 33, 47, 3, ar.SAMPLE_U16, 4095)
    r = c["ref"]
    assert np.array_equal(r["tau"], 100.0 * 2.0 ** -24 * r["amax"] ** 2 * r["S"]) and r["S"].max() <= 4095 and r["amax"].min() >= 1.0
    inside = r["amax"] == 1.0
    assert inside.mean() > 0.8 and r["tau"][inside].max() <= 100 * 2.0 ** -24 * 4095 < 0.0245


@pytest.mark.parametrize("kind", ["planted", "far"])
def test_planted_and_far_cases_are_exact_in_float32(kind):
    for sample, maxval in ((0, 255), (1, 1023), (1, 65535), (2, 0), (3, 0)):
        if kind == "far" and maxval > 1023:
            continue
        for w, h in ((1, 1), (33, 47), (100, 60)):
            for ext in ((w, h), ar.padded(w, h, 64)):
                c = ar.cached(kind, w, h, 3, sample, maxval, ext)
                assert ar.exact_in_float32(c), (kind, sample, maxval, w, h, ext)
                if kind == "far" and w > 1:
                    assert c["ref"]["amax"].max() > 100, "no sample leaves the extent by hundreds of pixels"
                    assert (c["ref"]["amax"] > 1).mean() > 0.2
                want = ar.expected_exact(c["ref"], sample, maxval)
                assert want.dtype == _DT[sample] and want.shape == c["p0"].shape


@pytest.mark.parametrize("name", ["smooth", "ragged", "scale2"])
def test_oracle_frame_from_the_oracle_motion_through_apply_ref(name, modeldirs, tmp_path_factory):
    """Frame semantics against the reference alone: the oracle's flow and mask applied by apply_ref to the u8 R, G, B planes of the input frames, extent = the padded
    frame, reproduce the oracle's quantised out0 outside the boundary set tau = 2^-6 amax (the engine scales by 1 / 255 first: tests/motion_ref.py), and that set
    stays under the cap - the condition item 3 of tests/test_gpu_apply.py applies to the engine."""
    o = mr.oracle_motion(name, modeldirs["rife-v4.6"], tmp_path_factory.getbasetemp())
    _, w, h, scale, _ = mr.E2E[name]
    ext = ar.padded(w, h, o["pad"])
    r = ar.apply64(np.moveaxis(o["a"], -1, 0), np.moveaxis(o["b"], -1, 0), o["flow"], o["mask"], ext)
    val = np.moveaxis(r["v"], 0, -1) + 0.5
    ok, frac = mr.frame_matches(o["frame"], val, r["amax"], 8)
    print("%s %dx%d extent %s: boundary set %.4f of the codes" % (name, w, h, ext, frac))
    assert frac < tr.CAP and ok
    # and apply_ref agrees with motion_ref's own rebuild to float64 rounding
    val2, amax2 = mr.rebuilt((o["a"], o["b"]), o["flow"], o["mask"], o["pad"])
    assert np.abs(val - val2).max() < 1e-3 and np.array_equal(amax2 >= 1, r["amax"] >= 1)


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "sanitize", "apply_check_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_check_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "apply_check")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"apply_check: (\d+) cases, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 2000 and int(m.group(2)) == 0, p.stdout[-500:]
    print(p.stdout.splitlines()[-1])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_makefile_builds_the_same_program():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../apply-check-asan:"):].split("\n", 2)
    assert "apply_check_main.cpp" in rule[0] and "apply_check.h" in rule[0] and "motion_check.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1]
    assert "../apply-check-asan" in mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
    assert mk.index("../motion-check-asan:") < mk.index("../apply-check-asan:")
