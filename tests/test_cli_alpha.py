"""`rife-hip -a`: the RGBA codecs without a GPU (`--transcode -a in out`), the start-up refusals, and the command line against the Python mirror on a GPU.

Files with -a: PNG colour types 4 and 6 bring their alpha channel (16-bit: the high byte, like the colour), a palette PNG its tRNS entries, a grey or RGB PNG
with a tRNS colour key alpha 0 where the pixel equals the key; WebP its alpha; a 32-bit BMP its fourth byte or alpha mask (all zero: opaque, like stb_image).
Every other file is opaque.  Output is colour type 6 PNG or lossless WebP."""
import importlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import alpha_ref
from conftest import ROOT

RIFE_HIP = os.environ.get("RIFE_HIP_BIN") or os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")      # RIFE_HIP_BIN: the sanitizer builds (tools/sanitize_run.sh)
needs_cli = pytest.mark.skipif(not os.path.exists(RIFE_HIP), reason="rife-hip is not built")


def run_cpp(args):
    p = subprocess.run([RIFE_HIP] + args, capture_output=True, text=True)
    return p.returncode, p.stderr


def _chunk(t, b):
    return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b) & 0xffffffff)


def write_png(path, rows, w, h, depth, ctype, extra=b""):
    """rows: h byte strings of packed samples -> a PNG (filter 0, one IDAT), `extra` = chunks between IHDR and IDAT: written here, independent of the code under test."""
    raw = b"".join(b"\x00" + bytes(r) for r in rows)
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) + extra + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))


def read_rgba(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "RGBA", (path, im.mode)
    return np.asarray(im)


def transcode(tmp_path, src, ext="png"):
    out = str(tmp_path / ("out_%s.%s" % (os.path.basename(str(src)).replace(".", "_"), ext)))
    rc, err = run_cpp(["--transcode", "-a", str(src), out])
    assert (rc, err) == (0, ""), (str(src), rc, err)
    return read_rgba(out)


def random_rgba(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    a[: h // 2, : w // 2, 3] = 255; a[h // 2:, : w // 3, 3] = 0          # opaque and clear regions next to random alpha
    return a


@needs_cli
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23), (1, 1), (333, 7), (1300, 900)])
def test_cpp_cli_rgba_png_round_trip_against_pil(tmp_path, w, h):
    """PNG colour type 6 written by PIL (adaptive filters) -> rife-hip's reader -> its writer (band-parallel at the largest size) -> PIL: the same four planes."""
    from PIL import Image
    a = random_rgba(w, h, w * 1000 + h)
    if w * h > 100000:
        a[..., :3] = alpha_ref.rgb_pair(w, h, 3)[0]                      # compressible colour: several deflate bands with history
    src = tmp_path / "a.png"
    Image.fromarray(a, "RGBA").save(src)
    assert np.array_equal(transcode(tmp_path, src), a)


@needs_cli
def test_cpp_cli_every_png_form_of_alpha_against_pil(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(11)
    h, w = 29, 41
    # grey + alpha (colour type 4)
    la = rng.integers(0, 256, (h, w, 2)).astype(np.uint8)
    Image.fromarray(la, "LA").save(tmp_path / "la.png")
    assert np.array_equal(transcode(tmp_path, tmp_path / "la.png"), np.asarray(Image.open(tmp_path / "la.png").convert("RGBA")))
    assert np.array_equal(transcode(tmp_path, tmp_path / "la.png")[..., 3], la[..., 1])
    # palette + tRNS (shorter than the palette: the rest is opaque)
    idx = rng.integers(0, 200, (h, w)).astype(np.uint8)
    pal = rng.integers(0, 256, 256 * 3).astype(np.uint8)
    trns = rng.integers(0, 256, 120).astype(np.uint8)
    im = Image.fromarray(idx, "P"); im.putpalette(pal.tobytes())
    im.save(tmp_path / "p.png", transparency=trns.tobytes())
    got = transcode(tmp_path, tmp_path / "p.png")
    assert np.array_equal(got, np.asarray(Image.open(tmp_path / "p.png").convert("RGBA")))
    assert np.array_equal(got[..., 3], np.where(idx < 120, trns[np.minimum(idx, 119)], 255))
    # RGB + tRNS colour key, grey + tRNS colour key
    rgb = rng.integers(0, 4, (h, w, 3)).astype(np.uint8) * 60           # few colours: the key occurs
    key = tuple(int(v) for v in rgb[3, 5])
    Image.fromarray(rgb, "RGB").save(tmp_path / "k.png", transparency=key)
    got = transcode(tmp_path, tmp_path / "k.png")
    want_a = np.where(np.all(rgb == np.array(key, np.uint8), axis=2), 0, 255)
    assert 0 < (want_a == 0).sum() < want_a.size
    assert np.array_equal(got[..., :3], rgb) and np.array_equal(got[..., 3], want_a)
    assert np.array_equal(got, np.asarray(Image.open(tmp_path / "k.png").convert("RGBA")))
    g8 = rng.integers(0, 8, (h, w)).astype(np.uint8) * 30
    Image.fromarray(g8, "L").save(tmp_path / "g.png", transparency=int(g8[2, 2]))
    got = transcode(tmp_path, tmp_path / "g.png")
    assert np.array_equal(got[..., 3], np.where(g8 == g8[2, 2], 0, 255)) and np.array_equal(got[..., 0], g8) and np.array_equal(got[..., 2], g8)


@needs_cli
def test_cpp_cli_16_bit_and_low_depth_alpha(tmp_path):
    """Written by hand: 16-bit RGBA and grey + alpha keep the high byte of all four samples; a 16-bit colour key compares all sixteen bits; a 4-bit grey file
    with a key compares the raw sample and scales the colour to 0..255 as without -a."""
    rng = np.random.default_rng(12)
    h, w = 17, 23
    v = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    write_png(str(tmp_path / "rgba16.png"), [v[y].astype(">u2").tobytes() for y in range(h)], w, h, 16, 6)
    assert np.array_equal(transcode(tmp_path, tmp_path / "rgba16.png"), (v >> 8).astype(np.uint8))
    ga = rng.integers(0, 65536, (h, w, 2)).astype(np.uint16)
    write_png(str(tmp_path / "ga16.png"), [ga[y].astype(">u2").tobytes() for y in range(h)], w, h, 16, 4)
    got = transcode(tmp_path, tmp_path / "ga16.png")
    assert np.array_equal(got[..., 0], ga[..., 0] >> 8) and np.array_equal(got[..., 1], ga[..., 0] >> 8) and np.array_equal(got[..., 3], ga[..., 1] >> 8)
    c = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
    c[4, 4] = c[0, 0]; c[5, 5] = c[0, 0] ^ np.uint16(1)                 # equal in the high byte only: stays opaque
    write_png(str(tmp_path / "key16.png"), [c[y].astype(">u2").tobytes() for y in range(h)], w, h, 16, 2, _chunk(b"tRNS", c[0, 0].astype(">u2").tobytes()))
    got = transcode(tmp_path, tmp_path / "key16.png")
    want_a = np.where(np.all(c == c[0, 0], axis=2), 0, 255)
    assert want_a[0, 0] == 0 and want_a[4, 4] == 0 and want_a[5, 5] == 255
    assert np.array_equal(got[..., 3], want_a) and np.array_equal(got[..., :3], (c >> 8).astype(np.uint8))
    g4 = rng.integers(0, 16, (h, 24)).astype(np.uint8)
    rows = [bytes((g4[y, 0::2] << 4) | g4[y, 1::2]) for y in range(h)]
    write_png(str(tmp_path / "g4.png"), rows, 24, h, 4, 0, _chunk(b"tRNS", struct.pack(">H", 9)))
    got = transcode(tmp_path, tmp_path / "g4.png")
    assert np.array_equal(got[..., 0], g4 * 17) and np.array_equal(got[..., 3], np.where(g4 == 9, 0, 255))
    # a tRNS chunk too short to be a key is no key
    write_png(str(tmp_path / "short.png"), [c[y].astype(">u2").tobytes() for y in range(h)], w, h, 16, 2, _chunk(b"tRNS", b"\x00\x01\x02"))
    assert np.all(transcode(tmp_path, tmp_path / "short.png")[..., 3] == 255)


@needs_cli
def test_cpp_cli_files_without_alpha_are_opaque_and_default_mode_is_unchanged(tmp_path):
    from PIL import Image
    a = random_rgba(52, 31, 13)
    Image.fromarray(a[..., :3].copy(), "RGB").save(tmp_path / "rgb.png")
    open(tmp_path / "rgb.ppm", "wb").write(b"P6\n52 31\n255\n" + a[..., :3].tobytes())
    Image.fromarray(a[..., :3].copy(), "RGB").save(tmp_path / "rgb.jpg", quality=95)
    for name in ("rgb.png", "rgb.ppm"):
        got = transcode(tmp_path, tmp_path / name)
        assert np.array_equal(got[..., :3], a[..., :3]) and np.all(got[..., 3] == 255), name
    got = transcode(tmp_path, tmp_path / "rgb.jpg")
    assert got.shape == (31, 52, 4) and np.all(got[..., 3] == 255)
    # without -a an RGBA file is read as its colour, as always, and RGB output is what it was
    Image.fromarray(a, "RGBA").save(tmp_path / "rgba.png")
    assert run_cpp(["--transcode", str(tmp_path / "rgba.png"), str(tmp_path / "plain.png")]) == (0, "")
    im = Image.open(tmp_path / "plain.png")
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), a[..., :3])
    assert run_cpp(["--transcode", str(tmp_path / "rgba.png"), str(tmp_path / "plain.ppm")]) == (0, "")
    assert open(tmp_path / "plain.ppm", "rb").read() == b"P6\n52 31\n255\n" + a[..., :3].tobytes()
    # RGBA output goes to png or webp only
    for ext in ("jpg", "ppm"):
        rc, err = run_cpp(["--transcode", "-a", str(tmp_path / "rgba.png"), str(tmp_path / ("o." + ext))])
        assert rc == 1 and "png or webp" in err


def _has_webp():
    try:
        from PIL import features
        return bool(features.check("webp"))
    except Exception:
        return False


@needs_cli
def test_cpp_cli_webp_with_alpha(tmp_path):
    from PIL import Image
    rc, err = run_cpp(["-0", "a.png", "-1", "b.png", "-o", "o.webp", "-m", "rife-v4.6", "-a"])
    if "built without libwebp" in err:
        pytest.skip("this rife-hip was built without libwebp")
    a = random_rgba(75, 44, 14)
    a[..., 3] = np.maximum(a[..., 3], 1)                                 # libwebp's simple encoder does not keep the colour under alpha 0
    Image.fromarray(a, "RGBA").save(tmp_path / "a.png")
    out = str(tmp_path / "a.webp")
    assert run_cpp(["--transcode", "-a", str(tmp_path / "a.png"), out]) == (0, "")
    assert np.array_equal(transcode(tmp_path, out), a), "png -> webp -> png"
    if _has_webp():
        im = Image.open(out)
        assert im.mode == "RGBA" and np.array_equal(np.asarray(im), a)
        Image.fromarray(a, "RGBA").save(tmp_path / "pil.webp", lossless=True, exact=True)
        assert np.array_equal(transcode(tmp_path, tmp_path / "pil.webp"), a)
        Image.fromarray(a[..., :3].copy(), "RGB").save(tmp_path / "rgb.webp", lossless=True)
        got = transcode(tmp_path, tmp_path / "rgb.webp")
        assert np.array_equal(got[..., :3], a[..., :3]) and np.all(got[..., 3] == 255)
    # alpha 0 survives as alpha 0
    a[:5, :5, 3] = 0
    Image.fromarray(a, "RGBA").save(tmp_path / "z.png")
    assert run_cpp(["--transcode", "-a", str(tmp_path / "z.png"), str(tmp_path / "z.webp")]) == (0, "")
    got = transcode(tmp_path, tmp_path / "z.webp")
    assert np.array_equal(got[..., 3], a[..., 3]) and np.array_equal(got[a[..., 3] > 0], a[a[..., 3] > 0])


def bmp32(px, comp=0, masks=None, hsz=40, bottom_up=True):
    """px: (h, w, 4) bytes in FILE order per pixel -> a 32-bit BMP."""
    h, w, _ = px.shape
    rows = px[::-1] if bottom_up else px
    extra = b"" if masks is None else b"".join(struct.pack("<I", m) for m in masks)
    hdr = struct.pack("<IiiHHIIiiII", hsz, w, h if bottom_up else -h, 1, 32, comp, w * h * 4, 2835, 2835, 0, 0)
    hdr = (hdr + extra).ljust(hsz, b"\x00") if hsz > 40 else hdr + extra
    off = 14 + len(hdr)
    return b"BM" + struct.pack("<IHHI", off + w * h * 4, 0, 0, off) + hdr + rows.tobytes()


@needs_cli
def test_cpp_cli_32_bit_bmp_alpha(tmp_path):
    a = random_rgba(33, 21, 15)
    bgra = a[..., [2, 1, 0, 3]]
    for name, data in (("rgb.bmp", bmp32(bgra)), ("topdown.bmp", bmp32(bgra, bottom_up=False)),
                       ("v4.bmp", bmp32(bgra, comp=3, masks=(0x00ff0000, 0x0000ff00, 0x000000ff, 0xff000000), hsz=108)),
                       ("v4argb.bmp", bmp32(a[..., [3, 0, 1, 2]], comp=3, masks=(0x0000ff00, 0x00ff0000, 0xff000000, 0x000000ff), hsz=108))):
        open(tmp_path / name, "wb").write(data)
        assert np.array_equal(transcode(tmp_path, tmp_path / name), a), name
    # bitfields without an alpha mask, an all-zero fourth byte, a 24-bit file: opaque
    open(tmp_path / "noa.bmp", "wb").write(bmp32(bgra, comp=3, masks=(0x00ff0000, 0x0000ff00, 0x000000ff)))
    z = bgra.copy(); z[..., 3] = 0
    open(tmp_path / "zero.bmp", "wb").write(bmp32(z))
    for name in ("noa.bmp", "zero.bmp"):
        got = transcode(tmp_path, tmp_path / name)
        assert np.array_equal(got[..., :3], a[..., :3]) and np.all(got[..., 3] == 255), name
    # an alpha mask that is not eight contiguous bits is refused
    open(tmp_path / "badmask.bmp", "wb").write(bmp32(bgra, comp=3, masks=(0x00ff0000, 0x0000ff00, 0x000000ff, 0x0f000000), hsz=108))
    rc, err = run_cpp(["--transcode", "-a", str(tmp_path / "badmask.bmp"), str(tmp_path / "o.png")])
    assert rc == 1 and "decode image" in err


@needs_cli
def test_cpp_cli_truncated_and_crafted_rgba_files_are_refused_not_fatal(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(16)
    a = random_rgba(50, 40, 16)
    Image.fromarray(a, "RGBA").save(tmp_path / "good.png")
    blob = open(tmp_path / "good.png", "rb").read()
    cases = {"cut_half.png": blob[:len(blob) // 2], "cut_tail.png": blob[:-20], "cut_ihdr.png": blob[:20]}
    cases["tall.png"] = blob[:8] + _chunk(b"IHDR", struct.pack(">IIBBBBB", 50, 160, 8, 6, 0, 0, 0)) + blob[33:]
    cases["huge.png"] = blob[:8] + _chunk(b"IHDR", struct.pack(">IIBBBBB", 60000, 60000, 8, 6, 0, 0, 0)) + blob[33:]
    for k in range(6):
        b = bytearray(blob); p = 60 + int(rng.integers(0, len(blob) - 80)); b[p] ^= 1 << int(rng.integers(0, 8))
        cases["flip%d.png" % k] = bytes(b)
    # palette file whose tRNS is LONGER than any palette, and whose pixels index past the palette
    idx = rng.integers(0, 256, (8, 8)).astype(np.uint8)
    rows = [idx[y].tobytes() for y in range(8)]
    raw = b"".join(b"\x00" + r for r in rows)
    cases["pal_short.png"] = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 8, 8, 8, 3, 0, 0, 0)) + _chunk(b"PLTE", bytes(range(30))) +
                              _chunk(b"tRNS", bytes(300)) + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))
    # colour key chunks of odd sizes on every colour type that has none
    for ct, ch in ((4, 2), (6, 4)):
        r = rng.integers(0, 256, (8, 8 * ch)).astype(np.uint8)
        cases["trns_ct%d.png" % ct] = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 8, 8, 8, ct, 0, 0, 0)) + _chunk(b"tRNS", b"\x01") +
                                      _chunk(b"IDAT", zlib.compress(b"".join(b"\x00" + r[y].tobytes() for y in range(8)))) + _chunk(b"IEND", b""))
    good_bmp = bmp32(a[..., [2, 1, 0, 3]], comp=3, masks=(0x00ff0000, 0x0000ff00, 0x000000ff, 0xff000000), hsz=108)
    cases["cut.bmp"] = good_bmp[:len(good_bmp) - 9]
    cases["cut_hdr.bmp"] = good_bmp[:60]
    cases["hdr56.bmp"] = good_bmp[:14] + struct.pack("<I", 56) + good_bmp[18:]      # claims a 56-byte header: the alpha mask is its last dword
    cases["neg.bmp"] = good_bmp[:18] + struct.pack("<i", -50) + good_bmp[22:]
    out = str(tmp_path / "o.png")
    for name, data in cases.items():
        open(tmp_path / name, "wb").write(data)
        p = subprocess.run([RIFE_HIP, "--transcode", "-a", str(tmp_path / name), out], capture_output=True, text=True)
        assert p.returncode in (0, 1), (name, p.returncode, p.stderr[-300:])      # refused or decoded - never a signal or a sanitizer exit
        if name.startswith(("cut", "tall", "huge", "pal_short", "neg")):
            assert p.returncode == 1 and "decode image" in p.stderr, name
        if name.startswith("trns_ct"):
            assert p.returncode == 0, name
    if _has_webp():
        Image.fromarray(a, "RGBA").save(tmp_path / "good.webp", lossless=True)
        wb = open(tmp_path / "good.webp", "rb").read()
        for name, data in (("cut.webp", wb[:len(wb) // 2]), ("riff_only.webp", wb[:12]), ("flip.webp", wb[:40] + bytes([wb[40] ^ 0x55]) + wb[41:])):
            open(tmp_path / name, "wb").write(data)
            p = subprocess.run([RIFE_HIP, "--transcode", "-a", str(tmp_path / name), out], capture_output=True, text=True)
            assert p.returncode in (0, 1), (name, p.returncode, p.stderr[-300:])


@needs_cli
def test_cpp_cli_start_up_refusals(tmp_path):
    """Before any device is opened (no GPU needed): -a with containers without alpha, with -b 10, with -x / -z / -u and with a family that is not rife-v4."""
    base = ["-0", "a.png", "-1", "b.png", "-a"]
    for extra, word in ((["-o", "o.jpg", "-m", "rife-v4.6"], "png or webp"), (["-o", "o.ppm", "-m", "rife-v4.6"], "png or webp"),
                        (["-o", "o.png", "-m", "rife-v4.6", "-b", "10"], "-b 10"), (["-o", "o.png", "-m", "rife-v4.6", "-x"], "-x"),
                        (["-o", "o.png", "-m", "rife-v4.6", "-z"], "-z"), (["-o", "o.png", "-m", "rife-v4.6", "-u"], "-u"),
                        (["-o", "o.png", "-m", "rife-v2.3"], "rife-v4.6 only"), (["-o", "o.png", "-m", "rife-HD"], "rife-v4.6 only"), (["-o", "o.png"], "rife-v4.6 only")):
        rc, err = run_cpp(base + extra)
        assert rc == 255 and word in err and ("alpha (-a)" in err or "RGBA frames (-a)" in err), (extra, rc, err)
    os.makedirs(tmp_path / "in"); os.makedirs(tmp_path / "out")
    rc, err = run_cpp(["-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "-m", "rife-v4.6", "-a", "-f", "%08d.jpg"])
    assert rc == 255 and "png or webp" in err
    rc, err = run_cpp(["-h"])
    assert "-a " in err and "alpha" in err


# ---- on the GPU: the command line against the Python mirror ---------------------------------------------------------------------

@pytest.mark.gpu
@needs_cli
@pytest.mark.parametrize("fmt", ["png", "webp"])
def test_cpp_cli_a_directory_equals_the_python_mirror(modeldirs, tmp_path, fmt):
    from PIL import Image
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    d = modeldirs["rife-v4.6"]
    w, h = 200, 120
    frames = [alpha_ref.rgba_pair(w, h, 300 + i, "smooth")[i & 1].copy() for i in range(3)]
    for f in frames:
        f[..., 3] = np.maximum(f[..., 3], 1) if fmt == "webp" else f[..., 3]
    os.makedirs(tmp_path / "in"); os.makedirs(tmp_path / "out")
    for i, f in enumerate(frames):
        Image.fromarray(f, "RGBA").save(str(tmp_path / "in" / ("%03d.png" % i)))
    p = subprocess.run([RIFE_HIP, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "-m", d, "-n", "7", "-a", "-f", "%08d." + fmt], capture_output=True, text=True)
    if fmt == "webp" and "built without libwebp" in p.stderr:
        pytest.skip("this rife-hip was built without libwebp")
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
        if fmt == "webp":
            assert run_cpp(["--transcode", "-a", path, path + ".png"]) == (0, "")
            path += ".png"
        got = read_rgba(path)
        assert np.array_equal(got[..., 3], want[..., 3]), (name, sx, float(fx))
        keep = want[..., 3] > 0 if fmt == "webp" else np.ones((h, w), bool)
        assert np.array_equal(got[keep], want[keep]), (name, sx, float(fx))
    # without -a the same directory gives the RGB frames it always gave
    os.makedirs(tmp_path / "out3")
    p = subprocess.run([RIFE_HIP, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out3"), "-m", d, "-n", "7"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-800:]
    im = Image.open(str(tmp_path / "out3" / sorted(os.listdir(tmp_path / "out3"))[1]))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), g.process(frames[0][..., :3].copy(), frames[1][..., :3].copy(), float(np.float32(scale))))


@pytest.mark.gpu
@needs_cli
def test_cpp_cli_a_refuses_rife_v4_at_start_up_and_serves_v46(modeldirs, tmp_path):
    from PIL import Image
    f = alpha_ref.rgba_pair(64, 64, 1, "hard")
    Image.fromarray(f[0], "RGBA").save(tmp_path / "a.png"); Image.fromarray(f[1], "RGBA").save(tmp_path / "b.png")
    base = ["-0", str(tmp_path / "a.png"), "-1", str(tmp_path / "b.png"), "-o", str(tmp_path / "o.png"), "-a"]
    p = subprocess.run([RIFE_HIP] + base + ["-m", modeldirs["rife-v4"]], capture_output=True, text=True)
    assert p.returncode != 0 and "RGBA frames are served for model family rife-v4.6" in p.stderr and "rife-v4 (4.0)" in p.stderr, p.stderr[-500:]
    assert not os.path.exists(tmp_path / "o.png")
    p = subprocess.run([RIFE_HIP] + base + ["-m", modeldirs["rife-v4.6"]], capture_output=True, text=True)
    assert p.returncode == 0 and read_rgba(str(tmp_path / "o.png")).shape == (64, 64, 4), p.stderr[-500:]
