"""Expected values and test frames for the RGBA path (include/rife_hip.h RIFE_HIP_PIX_RGBA8).

The reference has no alpha, but its graph can be made to compute it.  With blobs flow0 .. flow3 injected, the flownet's `out0` depends on `in0` / `in1`
through the two warps and the blend only (tests/test_alpha_host.py pins that: injecting the oracle's own four flows reproduces `out0` bit for bit).  So:
  1. extract flow0 .. flow3 from the oracle's flownet on the COLOUR planes (deep_ref.extract at depth 8);
  2. run the flownet again with in0, in1 = the alpha plane, code * (1 / 255.f), EDGE-padded to (hp, wp), in all three channels and the four blobs
     injected; channel 0 of `out0`, cropped and quantised min(max((int)(v * 255.f + 0.5f), 0), 255), is the expected alpha.
That is the header's statement: alpha is warped by the flows and blended by the mask that were estimated from the colour."""
import numpy as np

import deep_ref


def alpha_planes(alpha):
    """(h, w) uint8 -> (3, hp, wp) float32: code * (1 / 255.f) in all three channels, padded by edge replication."""
    h, w = alpha.shape
    wp, hp = deep_ref.padded(w, h)
    k = np.float32(1) / np.float32(255)
    p = np.pad(alpha.astype(np.float32) * k, ((0, hp - h), (0, wp - w)), mode="edge")
    return np.ascontiguousarray(np.broadcast_to(p, (3, hp, wp)), np.float32)


def colour_flows(oracle, rgb0, rgb1, t):
    """Step 1: the four flow blobs of the colour run."""
    return [deep_ref.extract(oracle, rgb0, rgb1, t, 8, "flow%d" % k) for k in range(4)]


def alpha_out0(oracle, alpha0, alpha1, t, flows):
    """Step 2: blob `out0` (3, hp, wp) of the flownet on the alpha planes with `flows` injected."""
    h, w = alpha0.shape
    wp, hp = deep_ref.padded(w, h)
    inputs = {"in0": alpha_planes(alpha0), "in1": alpha_planes(alpha1), "in2": np.full((1, hp, wp), t, np.float32)}
    for k, f in enumerate(flows):
        inputs["flow%d" % k] = np.ascontiguousarray(f, np.float32)
    return oracle.net_extract(0, inputs, "out0", 16 * wp * hp)


def quantise_plane(plane, w, h):
    v = plane[:h, :w].astype(np.float32) * np.float32(255) + np.float32(0.5)
    return np.clip(v.astype(np.int32), 0, 255).astype(np.uint8)


def expected_rgba(oracle, a, b, t):
    """a, b: (h, w, 4) uint8 RGBA.  Returns the expected (h, w, 4) frame: colour = the depth-8 recipe on R, G, B (== OracleRIFE.process with the GPU crop
    rule), alpha = the recipe above."""
    h, w, _ = a.shape
    rgb0, rgb1 = np.ascontiguousarray(a[..., :3]), np.ascontiguousarray(b[..., :3])
    flows = colour_flows(oracle, rgb0, rgb1, t)
    colour = deep_ref.quantise(deep_ref.extract(oracle, rgb0, rgb1, t, 8, "out0", flows=flows), w, h, 8)
    al = quantise_plane(alpha_out0(oracle, a[..., 3], b[..., 3], t, flows)[0], w, h)
    return np.concatenate([colour, al[..., None]], axis=2)


def rgb_pair(w, h, seed):
    """Two (h, w, 3) uint8 frames of the deep-colour test scene (sinusoids + discs, the second frame translated, + noise) rounded to 8 bits."""
    a, b = deep_ref.deep_pair(w, h, seed)
    return deep_ref.to_depth8(a), deep_ref.to_depth8(b)


def matte_pair(w, h, seed, hard):
    """Two (h, w) uint8 alpha planes that MOVE WITH THE SCENE of rgb_pair(w, h, seed): discs and a gradient translated by the scene's (dx, dy).
    hard: codes 0 / 255 only; otherwise smooth (anti-aliased edges, a low-frequency gradient)."""
    rng = np.random.default_rng(seed)
    dx, dy = rng.uniform(-8, 8, 2)                      # deep_pair_uncached draws the same two numbers first
    x = np.arange(w, dtype=np.float32); y = np.arange(h, dtype=np.float32)

    def render(ox, oy):
        r = np.random.default_rng(seed + 7)
        m = np.zeros((h, w), np.float32)
        for _ in range(10):
            cx, cy = r.uniform(0, w), r.uniform(0, h)
            rad = r.uniform(0.05, 0.25) * max(min(w, h), 4)
            d = np.sqrt((x[None, :] - ox - cx) ** 2 + (y[:, None] - oy - cy) ** 2)
            m = np.maximum(m, np.clip((rad - d) / (1.0 if hard else 6.0) + 0.5, 0, 1))
        if not hard:
            m = 0.75 * m + 0.25 * (0.5 + 0.5 * np.outer(np.sin((y - oy) * 0.021), np.cos((x - ox) * 0.017))).astype(np.float32)
        return m

    out = []
    for (ox, oy) in ((0.0, 0.0), (dx, dy)):
        m = render(ox, oy)
        out.append((np.where(m >= 0.5, 255, 0) if hard else np.rint(m * 255)).astype(np.uint8))
    return out[0], out[1]


def rgba_pair(w, h, seed, alpha="random"):
    """(h, w, 4) uint8 pair: the colour of rgb_pair + an alpha plane: "random" (uniform noise, independent per frame), "smooth", "hard", or an int code."""
    a, b = rgb_pair(w, h, seed)
    if alpha == "random":
        rng = np.random.default_rng(seed + 99)
        a0, a1 = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif alpha in ("smooth", "hard"):
        a0, a1 = matte_pair(w, h, seed, alpha == "hard")
    else:
        a0 = a1 = np.full((h, w), int(alpha), np.uint8)
    return np.ascontiguousarray(np.dstack([a, a0])), np.ascontiguousarray(np.dstack([b, a1]))


def report(got, want):
    """(max |diff|, share off by one) of two uint8 arrays."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d == 1).mean())
