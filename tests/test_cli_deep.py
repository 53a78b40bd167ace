"""`rife-hip -b 10`: the 10-bit codecs without a GPU (`--transcode10`), and the command line against the Python mirror on one.

Files: a 16-bit PNG or a PPM with maxval 65535 is read as code = v >> 6, a PPM with maxval 1023 as its codes, an 8-bit file as (v << 2) | (v >> 6); output .png is
16-bit RGB with v = (code << 6) | (code >> 4), .ppm is P6 with maxval 1023 (two bytes per sample, most significant first)."""
import importlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deep_ref
from conftest import ROOT

RIFE_HIP = os.environ.get("RIFE_HIP_BIN") or os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")      # RIFE_HIP_BIN: the sanitizer builds (tools/sanitize_run.sh)
needs_cli = pytest.mark.skipif(not os.path.exists(RIFE_HIP), reason="rife-hip is not built")


def run_cpp(args):
    p = subprocess.run([RIFE_HIP] + args, capture_output=True, text=True)
    return p.returncode, p.stderr


def _chunk(t, b):
    return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b) & 0xffffffff)


def write_png(path, arr, depth):
    """(h, w, 3) samples -> a plain RGB PNG of `depth` 8 or 16 (filter 0, one IDAT): written here, independent of the code under test."""
    h, w, _ = arr.shape
    rows = arr.astype(">u2" if depth == 16 else np.uint8)
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(h))
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))


def read_png16(path):
    """Parse IHDR, inflate with zlib and undo the row filters: the 16-bit RGB samples of a non-interlaced PNG, (h, w, 3) uint16."""
    d = open(path, "rb").read()
    assert d[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(d):
        n, t = struct.unpack(">I", d[pos:pos + 4])[0], d[pos + 4:pos + 8]
        body = d[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", d[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(t + body) & 0xffffffff, "chunk CRC"
        if t == b"IHDR": ihdr = struct.unpack(">IIBBBBB", body)
        if t == b"IDAT": idat += body
        pos += 12 + n
    w, h, depth, ctype, comp, flt, inter = ihdr
    assert (depth, ctype, comp, flt, inter) == (16, 2, 0, 0, 0), ihdr
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    stride = w * 6
    assert raw.size == (stride + 1) * h
    out = np.zeros((h, stride), np.uint8)
    for y in range(h):
        ft, line = int(raw[(stride + 1) * y]), raw[(stride + 1) * y + 1:(stride + 1) * (y + 1)].astype(np.int32)
        up = out[y - 1].astype(np.int32) if y else np.zeros(stride, np.int32)
        if ft == 0: cur = line
        elif ft == 2: cur = line + up
        else:
            cur = np.zeros(stride, np.int32)
            for x in range(stride):
                a = cur[x - 6] if x >= 6 else 0
                c = up[x - 6] if x >= 6 else 0
                if ft == 1: pr = a
                elif ft == 3: pr = (a + up[x]) >> 1
                else:
                    p = a + up[x] - c
                    pa, pb, pc = abs(p - a), abs(p - up[x]), abs(p - c)
                    pr = a if pa <= pb and pa <= pc else (up[x] if pb <= pc else c)
                cur[x] = (line[x] + pr) & 255
        out[y] = cur & 255
    return out.reshape(h, w, 3, 2).astype(np.uint16)[..., 0] << 8 | out.reshape(h, w, 3, 2)[..., 1]


def read_ppm1023(path):
    d = open(path, "rb").read()
    f = d.split(b"\n", 3)
    assert f[0] == b"P6" and f[2] == b"1023", f[:3]
    w, h = (int(x) for x in f[1].split())
    assert len(f[3]) == w * h * 6
    return np.frombuffer(f[3], ">u2").reshape(h, w, 3).astype(np.uint16)


def png_value(codes):
    return ((codes.astype(np.uint32) << 6) | (codes >> 4)).astype(np.uint16)


@needs_cli
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23), (1, 1), (333, 7)])
def test_cpp_cli_transcode10_round_trip_returns_the_codes(tmp_path, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    codes = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
    a, b, c = str(tmp_path / "a.png"), str(tmp_path / "b.ppm"), str(tmp_path / "c.png")
    write_png(a, png_value(codes), 16)
    assert run_cpp(["--transcode10", a, b]) == (0, "")
    assert np.array_equal(read_ppm1023(b), codes)
    assert run_cpp(["--transcode10", b, c]) == (0, "")
    assert np.array_equal(read_png16(c), png_value(codes)), "16-bit PNG -> PPM-1023 -> 16-bit PNG must return the same samples"
    # any 16-bit sample reads as its top ten bits
    v = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
    write_png(a, v, 16)
    assert run_cpp(["--transcode10", a, b])[0] == 0
    assert np.array_equal(read_ppm1023(b), v >> 6)
    # an independent decoder reads what was written
    Image = pytest.importorskip("PIL.Image")
    im = np.asarray(Image.open(c))
    want = png_value(codes)
    assert im.shape == (h, w, 3)
    assert np.array_equal(im, want if im.dtype == np.uint16 else (want >> 8).astype(np.uint8))


@needs_cli
def test_cpp_cli_transcode10_reads_every_source_depth(tmp_path):
    rng = np.random.default_rng(5)
    h, w = 19, 31
    out = str(tmp_path / "o.ppm")
    v8 = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    write_png(str(tmp_path / "e.png"), v8, 8)
    assert run_cpp(["--transcode10", str(tmp_path / "e.png"), out])[0] == 0
    assert np.array_equal(read_ppm1023(out), (v8.astype(np.uint16) << 2) | (v8 >> 6)), "an 8-bit file is (v << 2) | (v >> 6)"
    open(tmp_path / "e.ppm", "wb").write(b"P6\n%d %d\n255\n" % (w, h) + v8.tobytes())
    assert run_cpp(["--transcode10", str(tmp_path / "e.ppm"), out])[0] == 0
    assert np.array_equal(read_ppm1023(out), (v8.astype(np.uint16) << 2) | (v8 >> 6))
    v16 = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
    open(tmp_path / "f.ppm", "wb").write(b"P6\n%d %d\n65535\n" % (w, h) + v16.astype(">u2").tobytes())
    assert run_cpp(["--transcode10", str(tmp_path / "f.ppm"), out])[0] == 0
    assert np.array_equal(read_ppm1023(out), v16 >> 6)
    codes = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
    open(tmp_path / "g.ppm", "wb").write(b"P6\n%d %d\n1023\n" % (w, h) + codes.astype(">u2").tobytes())
    assert run_cpp(["--transcode10", str(tmp_path / "g.ppm"), out])[0] == 0
    assert np.array_equal(read_ppm1023(out), codes)
    # 8-bit containers are refused for 10-bit output
    for ext in ("jpg", "webp"):
        rc, err = run_cpp(["--transcode10", str(tmp_path / "g.ppm"), str(tmp_path / ("o." + ext))])
        assert rc == 1 and "png (16-bit) or ppm" in err


@needs_cli
def test_cpp_cli_default_depth_reads_a_16_bit_png_as_before(tmp_path):
    """-b 8 (the default): a 16-bit PNG keeps its high byte, a PPM with another maxval than 255 is refused - unchanged."""
    rng = np.random.default_rng(6)
    v16 = rng.integers(0, 65536, (21, 17, 3)).astype(np.uint16)
    write_png(str(tmp_path / "a.png"), v16, 16)
    assert run_cpp(["--transcode", str(tmp_path / "a.png"), str(tmp_path / "a.ppm")])[0] == 0
    d = open(tmp_path / "a.ppm", "rb").read()
    assert d.startswith(b"P6\n17 21\n255\n") and np.array_equal(np.frombuffer(d[len(b"P6\n17 21\n255\n"):], np.uint8).reshape(21, 17, 3), v16 >> 8)
    open(tmp_path / "g.ppm", "wb").write(b"P6\n17 21\n1023\n" + (v16 >> 6).astype(">u2").tobytes())
    rc, err = run_cpp(["--transcode", str(tmp_path / "g.ppm"), str(tmp_path / "b.ppm")])
    assert rc == 1 and "decode image" in err


@needs_cli
def test_cpp_cli_truncated_and_crafted_16_bit_files_are_refused_not_fatal(tmp_path):
    rng = np.random.default_rng(7)
    h, w = 40, 50
    v = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
    good = str(tmp_path / "good.png")
    write_png(good, v, 16)
    blob = open(good, "rb").read()
    out = str(tmp_path / "o.png")
    cases = {"cut_half.png": blob[:len(blob) // 2], "cut_tail.png": blob[:-20], "cut_ihdr.png": blob[:20]}
    # a header that promises more rows than the data holds, with a valid CRC
    ih = struct.pack(">IIBBBBB", w, h * 4, 16, 2, 0, 0, 0)
    cases["tall.png"] = blob[:8] + _chunk(b"IHDR", ih) + blob[33:]
    # bit flips inside the compressed stream
    for k in range(6):
        b = bytearray(blob); p = 60 + int(rng.integers(0, len(blob) - 80)); b[p] ^= 1 << int(rng.integers(0, 8))
        cases["flip%d.png" % k] = bytes(b)
    ppm = b"P6\n%d %d\n1023\n" % (w, h) + (v >> 6).astype(">u2").tobytes()
    cases["cut.ppm"] = ppm[:len(ppm) - 7]
    cases["over.ppm"] = b"P6\n2 1\n1023\n" + np.array([1, 2, 1024, 4, 5, 6], ">u2").tobytes()      # a sample above maxval
    cases["huge.ppm"] = b"P6\n70000 70000\n65535\n" + b"\x00" * 64
    for name, data in cases.items():
        open(tmp_path / name, "wb").write(data)
        p = subprocess.run([RIFE_HIP, "--transcode10", str(tmp_path / name), out], capture_output=True, text=True)
        assert p.returncode in (0, 1), (name, p.returncode, p.stderr[-300:])      # refused (or, for a flip the CRC-less reader cannot see, decoded) - never a signal or a sanitizer exit
        if name.startswith(("cut", "tall", "over", "huge")):
            assert p.returncode == 1 and "decode image" in p.stderr, name


@needs_cli
def test_cpp_cli_rejects_a_bad_depth_and_8_bit_containers():
    rc, err = run_cpp(["-0", "a.png", "-1", "b.png", "-o", "o.png", "-b", "12"])
    assert rc == 255 and "invalid bit depth argument" in err
    rc, err = run_cpp(["-0", "a.png", "-1", "b.png", "-o", "o.jpg", "-b", "10", "-m", "rife-v4.6"])
    assert rc == 255 and "png (16-bit) or ppm" in err


# ---- on the GPU: the command line against the Python mirror ---------------------------------------------------------------------

@pytest.mark.gpu
@needs_cli
@pytest.mark.parametrize("fmt", ["png", "ppm"])
def test_cpp_cli_b10_directory_equals_the_python_mirror(modeldirs, tmp_path, fmt):
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    d = modeldirs["rife-v4.6"]
    w, h = 200, 120
    frames = [deep_ref.deep_pair(w, h, 300 + i)[i & 1] for i in range(3)]
    os.makedirs(tmp_path / "in"); os.makedirs(tmp_path / "out")
    for i, f in enumerate(frames):
        write_png(str(tmp_path / "in" / ("%03d.png" % i)), png_value(f), 16)
    p = subprocess.run([RIFE_HIP, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "-m", d, "-n", "7", "-b", "10", "-f", "%08d." + fmt], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-800:]
    names = sorted(os.listdir(tmp_path / "out"))
    assert len(names) == 7
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    scale = 3 / 7.0
    for i, name in enumerate(names):
        fx = np.float32(i * scale); sx = int(np.floor(fx)); fx = np.float32(fx - sx)
        if sx >= 2: sx, fx = 1, np.float32(1.0)
        want = g.process(frames[sx], frames[sx + 1], float(fx))
        path = str(tmp_path / "out" / name)
        got = read_png16(path) >> 6 if fmt == "png" else read_ppm1023(path)
        if fmt == "png":
            assert np.array_equal(read_png16(path), png_value(want)), name
        assert np.array_equal(got, want), (name, sx, float(fx))


@pytest.mark.gpu
@needs_cli
def test_cpp_cli_b10_refuses_other_families_and_modes_at_start_up(modeldirs, tmp_path):
    f = deep_ref.deep_pair(64, 64, 1)
    write_png(str(tmp_path / "a.png"), png_value(f[0]), 16); write_png(str(tmp_path / "b.png"), png_value(f[1]), 16)
    base = ["-0", str(tmp_path / "a.png"), "-1", str(tmp_path / "b.png"), "-o", str(tmp_path / "o.png"), "-b", "10"]
    for extra, word in ((["-m", modeldirs["rife-v2.3"]], "rife-v2"), (["-m", modeldirs["rife-v4.6"], "-x"], "TTA"), (["-m", modeldirs["rife-v4.6"], "-u"], "UHD"),
                        (["-m", modeldirs["rife-v4.6"], "-z"], "temporal")):
        p = subprocess.run([RIFE_HIP] + base + extra, capture_output=True, text=True)
        assert p.returncode != 0 and "10-bit frames are served for model family rife-v4.6" in p.stderr and word in p.stderr, p.stderr[-500:]
        assert not os.path.exists(tmp_path / "o.png")
    p = subprocess.run([RIFE_HIP] + base + ["-m", modeldirs["rife-v4.6"]], capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(tmp_path / "o.png"), p.stderr[-500:]
