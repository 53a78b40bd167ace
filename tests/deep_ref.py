"""Expected values and test frames for the deep-colour (10-bit) path.

The reference has no 10-bit path, but its network takes arbitrary fp32 planes: the expected frame is the oracle's flownet on planes
code * (1 / 1023.f), zero-padded to (3, hp, wp), with the timestep plane as `in2`; blob `out0` cropped to (h, w) and quantised
min(max((int)(v * 1023.f + 0.5f), 0), 1023) - the semantics include/rife_hip.h states.  At depth 8 the same recipe reproduces OracleRIFE.process()
with set_gpu_crop(1) bit for bit (tests/test_deep_host.py pins that)."""
import numpy as np

MAXCODE = {8: 255, 10: 1023}


def padded(w, h):
    return (w + 31) // 32 * 32, (h + 31) // 32 * 32


def planes(codes, depth):
    """(h, w, 3) integer codes -> (3, hp, wp) float32 planes, zero-padded: code * (1 / max) as the engine computes it (fp32 reciprocal, one multiply)."""
    h, w, _ = codes.shape
    wp, hp = padded(w, h)
    k = np.float32(1) / np.float32(MAXCODE[depth])
    p = np.zeros((3, hp, wp), np.float32)
    p[:, :h, :w] = (np.minimum(codes, MAXCODE[depth]).astype(np.float32) * k).transpose(2, 0, 1)
    return p


def quantise(out0, w, h, depth):
    """(3, hp, wp) float32 -> (h, w, 3) codes: min(max((int)(v * max + 0.5f), 0), max), cropped with the padded pitch."""
    m = np.float32(MAXCODE[depth])
    v = out0[:, :h, :w].astype(np.float32) * m + np.float32(0.5)
    return np.clip(v.astype(np.int32), 0, MAXCODE[depth]).transpose(1, 2, 0).astype(np.uint16 if depth > 8 else np.uint8)


def net_inputs(a, b, t, depth, flows=()):
    h, w, _ = a.shape
    wp, hp = padded(w, h)
    inputs = {"in0": planes(a, depth), "in1": planes(b, depth), "in2": np.full((1, hp, wp), t, np.float32)}
    for k, f in enumerate(flows):
        inputs["flow%d" % k] = np.ascontiguousarray(f, np.float32)
    return inputs


def extract(oracle, a, b, t, depth, blob, flows=()):
    """Blob `blob` of the oracle's flownet for frames of integer codes at `depth` (optionally with blobs flow0.. injected)."""
    h, w, _ = a.shape
    wp, hp = padded(w, h)
    return oracle.net_extract(0, net_inputs(a, b, t, depth, flows), blob, 16 * wp * hp)


def expected_frame(oracle, a, b, t, depth=10):
    h, w, _ = a.shape
    return quantise(extract(oracle, a, b, t, depth, "out0"), w, h, depth)


_CACHE = {}


def deep_pair(w, h, seed=1000, amp=6):
    """deep_pair_uncached with the large frames kept (several tests share them; callers copy before they modify)."""
    key = (w, h, seed, amp)
    if key not in _CACHE:
        if len(_CACHE) >= 4:
            _CACHE.clear()
        _CACHE[key] = deep_pair_uncached(w, h, seed, amp)
    return _CACHE[key]


def deep_pair_uncached(w, h, seed=1000, amp=6):
    """Two truly 10-bit frames (h, w, 3) uint16, codes 0..1023: 8 low-frequency sinusoids per channel + filled discs, frame 1 = frame 0's content
    translated by (dx, dy) in [-8, 8] px, + uniform noise of +-amp codes, rounded to 10-bit codes.  At least 70 % of the samples have nonzero low two
    bits (asserted for frames of 1,000 samples and more): an 8-bit pass shifted left by two cannot reproduce them."""
    rng = np.random.default_rng(seed)
    dx, dy = rng.uniform(-8, 8, 2)
    x = np.arange(w, dtype=np.float32); y = np.arange(h, dtype=np.float32)

    def render(ox, oy, r):
        img = np.empty((h, w, 3), np.float32)
        for c in range(3):
            acc = np.zeros((h, w), np.float32)
            for _ in range(8):
                fx, fy = r.uniform(0.002, 0.03, 2)
                ph = r.uniform(0, 2 * np.pi)
                ax = ((x - ox) * (fx * 2 * np.pi) + ph).astype(np.float32); by = ((y - oy) * (fy * 2 * np.pi)).astype(np.float32)
                acc += np.outer(np.cos(by), np.sin(ax)) + np.outer(np.sin(by), np.cos(ax))
            img[..., c] = 0.5 + (0.35 / 8.0) * acc
        for _ in range(16):
            cx, cy = r.uniform(0, w), r.uniform(0, h)
            rad = r.uniform(0.02, 0.08) * min(w, h)
            col = r.uniform(0, 1, 3).astype(np.float32)
            y0, y1 = max(0, int(cy + oy - rad) - 1), min(h, int(cy + oy + rad) + 2)
            x0, x1 = max(0, int(cx + ox - rad) - 1), min(w, int(cx + ox + rad) + 2)
            if y0 >= y1 or x0 >= x1:
                continue
            m = (x[None, x0:x1] - ox - cx) ** 2 + (y[y0:y1, None] - oy - cy) ** 2 < rad * rad
            img[y0:y1, x0:x1][m] = col
        return img

    f0 = render(0.0, 0.0, np.random.default_rng(seed + 1))
    f1 = render(dx, dy, np.random.default_rng(seed + 1))
    out = []
    for f in (f0, f1):
        n = rng.integers(-amp, amp + 1, f.shape, dtype=np.int16)
        out.append(np.clip(np.rint(f * 1023).astype(np.int32) + n, 0, 1023).astype(np.uint16))
    for f in out:
        if f.size >= 1000:
            share = float((f & 3).astype(bool).mean())
            assert share >= 0.70, "only %.1f %% of the samples use the low two bits" % (100 * share)
    return out[0], out[1]


def to_depth8(codes10):
    """The same scene rounded to 8 bits (what a user had to feed before): round(code * 255 / 1023)."""
    return np.rint(codes10.astype(np.float64) * (255.0 / 1023.0)).astype(np.uint8)


def report(got, want, depth=10):
    """(max |diff|, share exact, share off by one, PSNR) in codes of `depth`."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    mse = float((d.astype(np.float64) ** 2).mean())
    psnr = 99.0 if mse == 0 else 10 * np.log10(float(MAXCODE[depth]) ** 2 / mse)
    return int(d.max()), float((d == 0).mean()), float((d == 1).mean()), psnr
