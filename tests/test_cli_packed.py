"""`rife-hip -b 16 [-a]`: the 16-bit codecs without a GPU (`--transcode16`, `--transcode16a`), the start-up refusals, and the command line against the Python mirror
(RIFE.process_hbd_packed) on one.

Files: a 16-bit PNG (colour types 0, 2, 4, 6) or a PPM with maxval 65535 is read with its full samples, a PPM with maxval 1023 as (c << 6) | (c >> 4), every 8-bit
source as v * 257; with -a a 16-bit alpha channel is read in full, 8-bit alpha as a * 257, a file without alpha is opaque.  Output .png is 16-bit RGB (colour type 6
with -a) with the samples as they are, .ppm is P6 with maxval 65535 (without -a).  The PNG files here are written and parsed by this file's own code."""
import importlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT

RIFE_HIP = os.environ.get("RIFE_HIP_BIN") or os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")      # RIFE_HIP_BIN: the sanitizer builds
CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}                                                                            # channels -> PNG colour type


def run_cpp(args):
    p = subprocess.run([RIFE_HIP] + args, capture_output=True, text=True)
    return p.returncode, p.stderr


def _chunk(t, b):
    return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b) & 0xffffffff)


def write_png(path, arr, depth, extra=b""):
    """(h, w, 1 | 2 | 3 | 4) samples -> a grey / grey + alpha / RGB / RGBA PNG of `depth` 8 or 16 (filter 0, one IDAT); extra: chunks between IHDR and IDAT"""
    h, w, ch = arr.shape
    rows = arr.astype(">u2" if depth == 16 else np.uint8)
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(h))
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, CTYPE[ch], 0, 0, 0)) + extra + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))


def read_png16(path, ch):
    """Parse IHDR, check every CRC, inflate with zlib and undo the row filters 0 (none), 1 (sub) and 2 (up): the samples of a non-interlaced 16-bit PNG of `ch` channels"""
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
    assert (depth, ctype, comp, flt, inter) == (16, CTYPE[ch], 0, 0, 0), ihdr
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    stride, bpp = w * ch * 2, ch * 2
    assert raw.size == (stride + 1) * h
    out = np.zeros((h, stride), np.uint8)
    for y in range(h):
        ft, line = int(raw[(stride + 1) * y]), raw[(stride + 1) * y + 1:(stride + 1) * (y + 1)]
        assert ft in (0, 1, 2), "row filter %d" % ft
        if ft == 0: out[y] = line
        elif ft == 2: out[y] = line + (out[y - 1] if y else 0)                                # uint8 arithmetic wraps modulo 256
        else: out[y] = np.cumsum(line.reshape(w, bpp).astype(np.uint32), axis=0).astype(np.uint8).reshape(-1)
    b = out.reshape(h, w, ch, 2).astype(np.uint16)
    return (b[..., 0] << 8) | b[..., 1]


def read_ppm65535(path):
    d = open(path, "rb").read()
    f = d.split(b"\n", 3)
    assert f[0] == b"P6" and f[2] == b"65535", f[:3]
    w, h = (int(x) for x in f[1].split())
    assert len(f[3]) == w * h * 6
    return np.frombuffer(f[3], ">u2").reshape(h, w, 3).astype(np.uint16)


# ---- the codecs, no GPU -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23), (1, 1), (333, 7)])
def test_transcode16_is_the_identity_on_16_bit_rgb(tmp_path, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    v = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
    a, b, c = str(tmp_path / "a.png"), str(tmp_path / "b.ppm"), str(tmp_path / "c.png")
    write_png(a, v, 16)
    assert run_cpp(["--transcode16", a, b]) == (0, "")
    assert np.array_equal(read_ppm65535(b), v)
    assert run_cpp(["--transcode16", b, c]) == (0, "")
    assert np.array_equal(read_png16(c, 3), v), "16-bit PNG -> PPM-65535 -> 16-bit PNG must return the same samples"
    # an RGBA file read without alpha keeps its colour; grey files spread their sample
    rgba = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    write_png(a, rgba, 16)
    assert run_cpp(["--transcode16", a, c])[0] == 0 and np.array_equal(read_png16(c, 3), rgba[..., :3])
    grey = rng.integers(0, 65536, (h, w, 2)).astype(np.uint16)
    write_png(a, grey[..., :1], 16)
    assert run_cpp(["--transcode16", a, c])[0] == 0 and np.array_equal(read_png16(c, 3), np.repeat(grey[..., :1], 3, axis=2))
    write_png(a, grey, 16)
    assert run_cpp(["--transcode16a", a, c])[0] == 0
    assert np.array_equal(read_png16(c, 4), np.concatenate([np.repeat(grey[..., :1], 3, axis=2), grey[..., 1:]], axis=2)), "grey + alpha at 16 bits"


@pytest.mark.parametrize("w,h", [(64, 48), (37, 23), (1, 1)])
def test_transcode16a_is_the_identity_on_16_bit_rgba(tmp_path, w, h):
    rng = np.random.default_rng(w * 999 + h)
    v = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    a, c = str(tmp_path / "a.png"), str(tmp_path / "c.png")
    write_png(a, v, 16)
    assert run_cpp(["--transcode16a", a, c]) == (0, "")
    assert np.array_equal(read_png16(c, 4), v)
    # a file without alpha is opaque
    write_png(a, v[..., :3], 16)
    assert run_cpp(["--transcode16a", a, c])[0] == 0
    got = read_png16(c, 4)
    assert np.array_equal(got[..., :3], v[..., :3]) and (got[..., 3] == 65535).all()
    open(tmp_path / "f.ppm", "wb").write(b"P6\n%d %d\n65535\n" % (w, h) + v[..., :3].astype(">u2").tobytes())
    assert run_cpp(["--transcode16a", str(tmp_path / "f.ppm"), c])[0] == 0
    got = read_png16(c, 4)
    assert np.array_equal(got[..., :3], v[..., :3]) and (got[..., 3] == 65535).all()
    # a 16-bit colour key: the pixel that equals it in every bit is clear, all others opaque
    key = v[0, 0, :3]
    write_png(a, v[..., :3], 16, extra=_chunk(b"tRNS", key.astype(">u2").tobytes()))
    assert run_cpp(["--transcode16a", a, c])[0] == 0
    got = read_png16(c, 4)
    assert np.array_equal(got[..., 3], np.where((v[..., :3] == key).all(axis=2), 0, 65535))
    # an independent decoder reads what was written
    try:
        from PIL import Image
    except ImportError:
        return
    write_png(a, v, 16)
    assert run_cpp(["--transcode16a", a, c])[0] == 0
    im = np.asarray(Image.open(c))
    assert im.shape == (h, w, 4)
    assert np.array_equal(im, v if im.dtype == np.uint16 else (v >> 8).astype(np.uint8))


def test_transcode16_reads_every_source_depth(tmp_path):
    rng = np.random.default_rng(5)
    h, w = 19, 31
    out, outa = str(tmp_path / "o.ppm"), str(tmp_path / "o.png")
    v8 = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    wide = v8.astype(np.uint16) * 257
    write_png(str(tmp_path / "e.png"), v8[..., :3], 8)
    assert run_cpp(["--transcode16", str(tmp_path / "e.png"), out])[0] == 0
    assert np.array_equal(read_ppm65535(out), wide[..., :3]), "an 8-bit file is v * 257"
    write_png(str(tmp_path / "e4.png"), v8, 8)
    assert run_cpp(["--transcode16a", str(tmp_path / "e4.png"), outa])[0] == 0
    assert np.array_equal(read_png16(outa, 4), wide), "8-bit alpha is a * 257"
    open(tmp_path / "e.ppm", "wb").write(b"P6\n%d %d\n255\n" % (w, h) + v8[..., :3].tobytes())
    assert run_cpp(["--transcode16", str(tmp_path / "e.ppm"), out])[0] == 0
    assert np.array_equal(read_ppm65535(out), wide[..., :3])
    codes = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
    open(tmp_path / "g.ppm", "wb").write(b"P6\n%d %d\n1023\n" % (w, h) + codes.astype(">u2").tobytes())
    assert run_cpp(["--transcode16", str(tmp_path / "g.ppm"), out])[0] == 0
    assert np.array_equal(read_ppm65535(out), (codes << 6) | (codes >> 4)), "a maxval-1023 file is (c << 6) | (c >> 4)"
    # other containers are refused for 16-bit output, ppm with alpha too
    for flag, ext in (("--transcode16", "jpg"), ("--transcode16", "webp"), ("--transcode16a", "ppm"), ("--transcode16a", "webp")):
        rc, err = run_cpp([flag, str(tmp_path / "g.ppm"), str(tmp_path / ("x." + ext))])
        assert rc == 1 and "16-bit frames are written as png" in err, (flag, ext, err)


def test_truncated_and_crafted_files_are_refused_not_fatal(tmp_path):
    rng = np.random.default_rng(7)
    h, w = 40, 50
    v = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    good = str(tmp_path / "good.png")
    write_png(good, v, 16)
    blob = open(good, "rb").read()
    out = str(tmp_path / "o.png")
    cases = {"cut_half.png": blob[:len(blob) // 2], "cut_tail.png": blob[:-20], "cut_ihdr.png": blob[:20]}
    cases["tall.png"] = blob[:8] + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h * 4, 16, 6, 0, 0, 0)) + blob[33:]
    ppm = b"P6\n%d %d\n65535\n" % (w, h) + v[..., :3].astype(">u2").tobytes()
    cases["cut.ppm"] = ppm[:len(ppm) - 7]
    cases["huge.ppm"] = b"P6\n70000 70000\n65535\n" + b"\x00" * 64
    for name, data in cases.items():
        open(tmp_path / name, "wb").write(data)
        for flag in ("--transcode16", "--transcode16a"):
            p = subprocess.run([RIFE_HIP, flag, str(tmp_path / name), out], capture_output=True, text=True)
            assert p.returncode == 1 and "decode image" in p.stderr, (name, flag, p.returncode, p.stderr[-300:])


# ---- start-up refusals, no GPU: each ends before a device is opened ---------------------------------------------------------------------------------------------------
def test_start_up_refusals():
    base = ["-0", "a.png", "-1", "b.png"]
    rc, err = run_cpp(base + ["-o", "x.jpg", "-b", "16", "-m", "rife-v4.6"])
    assert rc == 255 and "16-bit frames (-b 16) are written as png or ppm (maxval 65535) only, not jpg" in err, err
    rc, err = run_cpp(base + ["-o", "x.webp", "-b", "16", "-m", "rife-v4.6"])
    assert rc == 255 and "-b 16" in err and "not webp" in err, err
    rc, err = run_cpp(base + ["-o", "x.ppm", "-b", "16", "-a", "-m", "rife-v4.6"])
    assert rc == 255 and "16-bit frames (-b 16) are written as png only, not ppm" in err, err
    rc, err = run_cpp(base + ["-o", "x.webp", "-b", "16", "-a", "-m", "rife-v4.6"])
    assert rc == 255 and "16-bit frames (-b 16) are written as png only, not webp" in err, err
    for flag, word in (("-x", "-x (TTA mode)"), ("-z", "-z (temporal TTA mode)"), ("-u", "-u (UHD mode)")):
        rc, err = run_cpp(base + ["-o", "x.png", "-b", "16", "-m", "rife-v4.6", flag])
        assert rc == 255 and "16-bit frames (-b 16) are served in plain mode only" in err and word in err, err
    rc, err = run_cpp(base + ["-o", "x.png", "-b", "16", "-m", "rife-v2.3"])
    assert rc == 255 and "16-bit frames (-b 16) are served for model family rife-v4.6 only, not for rife-v2.3" in err, err
    rc, err = run_cpp(base + ["-o", "x.png", "-b", "16"])      # the default model is rife-v2.3
    assert rc == 255 and "-b 16" in err and "rife-v2.3" in err, err
    rc, err = run_cpp(["-i", "in.y4m", "-o", "out.y4m", "-b", "16", "-m", "rife-v4.6"])
    assert rc == 1 and "-b 16 goes with image files, not with a .y4m video" in err, err
    # what was refused before stays refused, by the same words
    rc, err = run_cpp(base + ["-o", "x.png", "-b", "12"])
    assert rc == 255 and "invalid bit depth argument" in err
    rc, err = run_cpp(base + ["-o", "x.png", "-b", "10", "-a", "-m", "rife-v4.6"])
    assert rc == 255 and "not with -b 10" in err and "two alpha bits" in err
    p = subprocess.run([RIFE_HIP, "-h"], capture_output=True, text=True)
    assert "8, 10 or 16" in p.stderr and "with -b 16: 16-bit RGBA png out" in p.stderr


# ---- on the GPU: the command line against the Python mirror -----------------------------------------------------------------------------------------------------------
def _stills(w, h, ch, n):
    """n frames of a moving pattern over the whole 16-bit range, with a soft matte for ch = 4"""
    frames = []
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    for i in range(n):
        rng = np.random.default_rng(300 + i)
        planes = [0.5 + 0.3 * np.sin((x + 4.0 * i + 7 * k) / 11.0) + 0.19 * np.cos((y - 3.0 * i + 5 * k) / 8.0) for k in range(3)]
        if ch == 4:
            planes.append(np.clip(0.5 + 0.7 * np.sin((x + 3.0 * i) / 9.0) * np.cos((y + 2.0 * i) / 7.0), 0, 1))
        f = np.stack(planes, axis=2) * 65535 + rng.integers(-200, 200, (h, w, ch))
        frames.append(np.clip(f, 0, 65535).astype(np.uint16))
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,fmt", [(False, "png"), (False, "ppm"), (True, "png")], ids=["rgb-png", "rgb-ppm", "rgba-png"])
def test_cpp_cli_b16_directory_equals_the_python_mirror(modeldirs, tmp_path, alpha, fmt):
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    d = modeldirs["rife-v4.6"]
    w, h, ch = 200, 120, 4 if alpha else 3
    frames = _stills(w, h, ch, 3)
    os.makedirs(tmp_path / "in"); os.makedirs(tmp_path / "out")
    for i, f in enumerate(frames):
        write_png(str(tmp_path / "in" / ("%03d.png" % i)), f, 16)
    p = subprocess.run([RIFE_HIP, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "-m", d, "-n", "7", "-b", "16", "-f", "%08d." + fmt] + (["-a"] if alpha else []),
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-800:]
    names = sorted(os.listdir(tmp_path / "out"))
    assert len(names) == 7
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    scale = 3 / 7.0
    moved = False
    for i, name in enumerate(names):
        fx = np.float32(i * scale); sx = int(np.floor(fx)); fx = np.float32(fx - sx)
        if sx >= 2: sx, fx = 1, np.float32(1.0)
        want = g.process_hbd_packed(frames[sx], frames[sx + 1], float(fx), 16)
        path = str(tmp_path / "out" / name)
        got = read_png16(path, ch) if fmt == "png" else read_ppm65535(path)
        assert got.shape == want.shape and np.array_equal(got, want), (name, sx, float(fx), int((got != want).sum()))
        moved |= bool(0 < fx < 1 and (want != frames[sx]).any())
    assert moved, "no interpolated frame differs from its first input: the run checks nothing"


@pytest.mark.gpu
def test_cpp_cli_b16_refuses_other_families_and_modes_at_start_up(modeldirs, tmp_path):
    f = _stills(64, 64, 4, 2)
    write_png(str(tmp_path / "a.png"), f[0], 16); write_png(str(tmp_path / "b.png"), f[1], 16)
    base = ["-0", str(tmp_path / "a.png"), "-1", str(tmp_path / "b.png"), "-o", str(tmp_path / "o.png"), "-b", "16", "-a"]
    # rife-v4 (4.0) shares the directory prefix: only the engine tells it apart, with the one-pixel call at start-up
    p = subprocess.run([RIFE_HIP] + base + ["-m", modeldirs["rife-v4"]], capture_output=True, text=True)
    assert p.returncode != 0 and "-b 16 is not available" in p.stderr and "high bit depth" in p.stderr and "rife-v4 (4.0)" in p.stderr, p.stderr[-500:]
    assert not os.path.exists(tmp_path / "o.png")
    p = subprocess.run([RIFE_HIP] + base + ["-m", modeldirs["rife-v4.6"]], capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(tmp_path / "o.png"), p.stderr[-500:]
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    assert np.array_equal(read_png16(str(tmp_path / "o.png"), 4), g.process_hbd_packed(f[0], f[1], 0.5, 16))
