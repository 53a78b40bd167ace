"""`rife-hip -i in.y4m -o out.y4m`: the YUV4MPEG2 video mode of the command line.

Without a GPU (the tests with cpp_cli in their names): header parsing and writing, the frame-rate fraction, the -n schedule, in-order output from several save
threads and every refusal, against the host-only stub engine of tests/sanitize/ (its 8-bit "interpolation" is a byte blend a test can predict).  The binary is
RIFE_HIP_BIN when that is set (the sanitizer builds of tools/sanitize_run.sh) and a plain build of the same sources otherwise.
On a GPU: the real binary's output frames equal the Python mirror's process_yuv at the scheduled timesteps, byte for byte."""
import importlib
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import cli_harness as cli
import yuv_ref as yr
from conftest import ROOT

CSRC = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc")
REAL = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")


@pytest.fixture(scope="module")
def stub_bin(tmp_path_factory):
    if os.environ.get("RIFE_HIP_BIN"):
        return os.environ["RIFE_HIP_BIN"]
    out = str(tmp_path_factory.mktemp("stubcli") / "rife-hip-stub")
    san = os.path.join(ROOT, "tests", "sanitize")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "main.cpp"), os.path.join(CSRC, "rife.cpp"), os.path.join(san, "stub_engine.cpp"),
                    os.path.join(san, "stub_engine_yuv.cpp"), "-o", out, "-lz", "-lpthread"], check=True, capture_output=True)
    return out


def run(binary, args):
    p = subprocess.run([binary] + args, capture_output=True)
    return p.returncode, p.stderr.decode(errors="replace"), p.stdout


def write_y4m(path, header, frames, marker=b"FRAME\n"):
    with open(path, "wb") as f:
        f.write(header.encode() + b"\n")
        for fr in frames:
            f.write(marker + fr.tobytes())


def read_y4m(data, frame_bytes):
    """-> (header tokens, list of frame byte strings); asserts the framing."""
    nl = data.index(b"\n")
    toks = data[:nl].decode().split(" ")
    body = data[nl + 1:]
    rec = 6 + frame_bytes
    assert len(body) % rec == 0, "output is not a whole number of frames"
    frames = []
    for k in range(len(body) // rec):
        assert body[k * rec:k * rec + 6] == b"FRAME\n"
        frames.append(body[k * rec + 6:(k + 1) * rec])
    return toks, frames


def random_frames(n, w, h, px, seed):
    rng = np.random.default_rng(seed)
    top = 1024 if yr.depth(px) == 10 else 256
    return [rng.integers(0, top, yr.frame_elems(w, h)).astype(yr.dtype(px)) for _ in range(n)]


def stub_blend(a, b, t):
    """tests/sanitize/stub_engine.cpp: (uint8_t)((1.f - t) * a + t * b + 0.5f) per byte."""
    t = np.float32(t)
    return ((np.float32(1) - t) * a.astype(np.float32) + t * b.astype(np.float32) + np.float32(0.5)).astype(np.uint8)


HDR = "YUV4MPEG2 W33 H47 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED"


# ---- valid files -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 15, 5])
def test_cpp_cli_y4m_header_rate_schedule_and_order(stub_bin, tmp_path, n):
    w, h, count = 33, 47, 7
    frames = random_frames(count, w, h, yr.PIX_I420, 3)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    write_y4m(src, HDR, frames)
    rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6", "-j", "1:4:4"] + (["-n", str(n)] if n else []))
    assert rc == 0, err
    nout = n or 2 * count
    toks, out = read_y4m(open(dst, "rb").read(), yr.frame_bytes(w, h, yr.PIX_I420))
    g = gcd(30000 * nout, 1001 * count)
    assert toks == ["YUV4MPEG2", "W33", "H47", "F%d:%d" % (30000 * nout // g, 1001 * count // g), "Ip", "A1:1", "C420jpeg", "XYSCSS=420JPEG", "XCOLORRANGE=LIMITED"]
    sched = cli.build_schedule(count, nout)                   # the directory mode's schedule
    assert len(out) == nout == len(sched)
    for i, (sx, fx) in enumerate(sched):
        want = frames[sx] if fx == 0.0 else frames[sx + 1] if fx == 1.0 else stub_blend(frames[sx], frames[sx + 1], fx)
        assert out[i] == want.tobytes(), "output frame %d (frames %d, %d at %g)" % (i, sx, sx + 1, fx)
    # -o - : the same bytes on stdout, nothing else there
    rc, err, so = run(stub_bin, ["-i", src, "-o", "-", "-m", "rife-v4.6", "-j", "2:3:3", "-v"] + (["-n", str(n)] if n else []))
    assert rc == 0, err
    assert so == open(dst, "rb").read()


def test_cpp_cli_y4m_ten_bit_and_sparse_headers(stub_bin, tmp_path):
    w, h, count = 5, 3, 4
    frames = random_frames(count, w, h, yr.PIX_I420P10, 4)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    write_y4m(src, "YUV4MPEG2 W5 H3 F25:1 C420p10", frames)
    rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6", "-c", "2020"])
    assert rc == 0, err
    toks, out = read_y4m(open(dst, "rb").read(), yr.frame_bytes(w, h, yr.PIX_I420P10))
    assert toks == ["YUV4MPEG2", "W5", "H3", "F50:1", "C420p10"] and len(out) == 8
    assert out[0] == frames[0].tobytes() and out[2] == frames[1].tobytes()      # timestep 0: the engine's copy of the frame
    # no I, no C field: progressive 4:2:0 at 8 bits
    f8 = random_frames(2, 4, 4, yr.PIX_I420, 5)
    write_y4m(src, "YUV4MPEG2 W4 H4 F24:1", f8)
    rc, err, so = run(stub_bin, ["-i", src, "-o", "-", "-m", "rife-v4.6", "-n", "3", "-c", "601:full"])
    assert rc == 0, err
    toks, out = read_y4m(so, 24)
    assert toks == ["YUV4MPEG2", "W4", "H4", "F36:1"] and len(out) == 3 and out[0] == f8[0].tobytes()


# ---- bad files and flags: a message, exit status 1, never a crash -----------------------------------------------------------------------------

def _good(tmp_path):
    src = str(tmp_path / "good.y4m")
    write_y4m(src, "YUV4MPEG2 W8 H6 F25:1 Ip C420jpeg", random_frames(3, 8, 6, yr.PIX_I420, 6))
    return src


BAD_HEADERS = [("YUV4MPEG2 W8 H6 F25:1 Ip C422", "C422"), ("YUV4MPEG2 W8 H6 F25:1 It C420", "It"), ("YUV4MPEG2 W8 H6 F25:1 Im C420", "Im"),
               ("YUV4MPEG2 W0 H6 F25:1 C420", "W0"), ("YUV4MPEG2 W8 H0 F25:1 C420", "H0"), ("YUV4MPEG2 W99999999 H6 F25:1 C420", "W99999999"),
               ("YUV4MPEG2 W8 H6666666666666 F25:1 C420", "H6666666666666"), ("YUV4MPEG2 W-8 H6 F25:1 C420", "W-8"), ("YUV4MPEG2 H6 F25:1 C420", "W"),
               ("YUV4MPEG2 W8 H6 F25:0 C420", "F25:0"), ("YUV4MPEG2 W8 H6 C420", "F"), ("YUV4MPEG2 W8 H6 F25:1 C444", "C444"), ("YUV4MPEG2 W8 H6 F25:1 C420p12", "C420p12"),
               ("YUV4MPEG3 W8 H6 F25:1 C420", "YUV4MPEG2"), ("YUV4MPEG2 W8 H6 F25:1 C420 " + "X" * 300, "256")]


@pytest.mark.parametrize("header,word", BAD_HEADERS, ids=[w for _, w in BAD_HEADERS])
def test_cpp_cli_y4m_bad_headers_are_refused(stub_bin, tmp_path, header, word):
    src, dst = str(tmp_path / "bad.y4m"), str(tmp_path / "out.y4m")
    write_y4m(src, header, random_frames(3, 8, 6, yr.PIX_I420, 7))
    rc, err, so = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"])
    assert rc == 1 and word in err and so == b"", (rc, err)
    assert not os.path.exists(dst)


def test_cpp_cli_y4m_bad_bodies_are_refused(stub_bin, tmp_path):
    frames = random_frames(3, 8, 6, yr.PIX_I420, 8)
    src, dst = str(tmp_path / "bad.y4m"), str(tmp_path / "out.y4m")
    write_y4m(src, "YUV4MPEG2 W8 H6 F25:1 C420", frames)
    whole = open(src, "rb").read()
    for cut in (1, 30, 72 + 5, 72 + 6 - 1):                     # inside the last frame's samples, inside its marker, one byte short of it
        open(src, "wb").write(whole[:-cut])
        rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"])
        assert rc == 1 and "truncated" in err, (cut, rc, err)
    open(src, "wb").write(whole + b"FRA")
    rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"])
    assert rc == 1 and "truncated" in err, (rc, err)
    write_y4m(src, "YUV4MPEG2 W8 H6 F25:1 C420", frames, marker=b"FRAMF\n")
    rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"])
    assert rc == 1 and "FRAME" in err, (rc, err)
    write_y4m(src, "YUV4MPEG2 W8 H6 F25:1 C420", frames[:1])
    rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"])
    assert rc == 1 and "two frames" in err, (rc, err)
    open(src, "wb").write(b"")
    rc, err, _ = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"])
    assert rc == 1 and "header" in err, (rc, err)
    assert not os.path.exists(dst)


@pytest.mark.parametrize("flags,word", [(["-a"], "-a"), (["-b", "10"], "-b 10"), (["-x"], "(-x)"), (["-z"], "(-z)"), (["-u"], "(-u)"), (["-c", "470"], "470"),
                                        (["-c", "709:tv"], "tv"), (["-m", "rife-v2.3"], "rife-v2.3"), (["-m", "rife-anime"], "rife-anime")],
                         ids=["a", "b10", "x", "z", "u", "matrix", "range", "v2", "v1"])
def test_cpp_cli_y4m_flags_out_of_scope_are_refused(stub_bin, tmp_path, flags, word):
    src, dst = _good(tmp_path), str(tmp_path / "out.y4m")
    rc, err, so = run(stub_bin, ["-i", src, "-o", dst, "-m", "rife-v4.6"] + flags)
    assert rc == 1 and word in err and so == b"", (rc, err)
    assert not os.path.exists(dst)


def test_cpp_cli_y4m_output_and_stdin_rules(stub_bin, tmp_path):
    src = _good(tmp_path)
    rc, err, _ = run(stub_bin, ["-i", src, "-o", str(tmp_path / "out.png"), "-m", "rife-v4.6"])
    assert rc == 1 and ".y4m" in err
    rc, err, _ = run(stub_bin, ["-i", src, "-o", str(tmp_path), "-m", "rife-v4.6"])
    assert rc == 1 and ".y4m" in err
    rc, err, _ = run(stub_bin, ["-i", "-", "-o", str(tmp_path / "out.y4m"), "-m", "rife-v4.6"])
    assert rc == 1 and "stdin" in err
    rc, err, _ = run(stub_bin, ["-h"])
    assert ".y4m" in err and "stdin" in err


# ---- on the GPU: the real binary against the Python mirror ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REAL), reason="rife-hip is not built")
@pytest.mark.parametrize("w,h,count,tag,px,flags", [(100, 60, 7, "C420jpeg", yr.PIX_I420, []), (33, 47, 5, "C420p10", yr.PIX_I420P10 | yr.CSP_BT2020NCL, ["-c", "2020"])],
                         ids=["100x60-C420jpeg", "33x47-C420p10"])
def test_y4m_file_equals_process_yuv_at_the_scheduled_timesteps(modeldirs, tmp_path, w, h, count, tag, px, flags):
    import deep_ref
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    model = modeldirs["rife-v4.6"]
    frames = [yr.rgb10_to_yuv(deep_ref.deep_pair_uncached(w, h, 90 + i)[i & 1], px) for i in range(count)]
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    write_y4m(src, "YUV4MPEG2 W%d H%d F24:1 Ip A1:1 %s" % (w, h, tag), frames)
    n = 2 * count + 1
    rc, err, _ = run(REAL, ["-i", src, "-o", dst, "-m", model, "-n", str(n), "-j", "1:2:2"] + flags)
    assert rc == 0, err
    toks, out = read_y4m(open(dst, "rb").read(), yr.frame_bytes(w, h, px))
    g = gcd(24 * n, count)
    assert toks == ["YUV4MPEG2", "W%d" % w, "H%d" % h, "F%d:%d" % (24 * n // g, count // g), "Ip", "A1:1", tag]
    eng = amd.RIFE(0, rife_v4=True); eng.load(model)
    sched = cli.build_schedule(count, n)
    assert len(out) == n
    for i, (sx, fx) in enumerate(sched):
        want = eng.process_yuv(frames[sx], frames[sx + 1], w, h, fx, px)
        assert out[i] == want.tobytes(), "output frame %d (frames %d, %d at %g)" % (i, sx, sx + 1, fx)
    rc, err, so = run(REAL, ["-i", src, "-o", "-", "-m", model, "-n", str(n), "-j", "2:2:3"] + flags)
    assert rc == 0, err
    assert so == open(dst, "rb").read()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REAL), reason="rife-hip is not built")
def test_y4m_refusals_come_from_the_engine(modeldirs, tmp_path):
    """rife-v4 (4.0) shares the directory prefix, and a 10-bit file tagged full range has no exact round trip: the engine says so before a frame is written."""
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    write_y4m(src, "YUV4MPEG2 W8 H6 F25:1 C420", random_frames(3, 8, 6, yr.PIX_I420, 1))
    rc, err, _ = run(REAL, ["-i", src, "-o", dst, "-m", modeldirs["rife-v4"]])
    assert rc == 1 and "rife-v4 (4.0)" in err, (rc, err)
    write_y4m(src, "YUV4MPEG2 W8 H6 F25:1 C420p10 XCOLORRANGE=FULL", random_frames(3, 8, 6, yr.PIX_I420P10, 1))
    rc, err, _ = run(REAL, ["-i", src, "-o", dst, "-m", modeldirs["rife-v4.6"]])
    assert rc == 1 and "full-range" in err, (rc, err)
