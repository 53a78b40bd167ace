"""Expected values for flow scale 2 (include/rife_hip.h rife_hip_set_flow_scale): the rife-v4.6 flownet with every IFBlock scale doubled.

The reference has no such mode for rife-v4.x, but its executor runs whatever graph flownet.param describes: the expected frame is the oracle's flownet on
the REWRITTEN graph, fed planes zero-padded to 64n, blob out0 cropped and quantised as tests/deep_ref.py does.  The rewrite is structural - the n-th Interp, the
one-input mul / div BinaryOps, the weighted Eltwise sums, the last two-input Concat, the PixelShuffle whose top is flow3 and the first two-input BinaryOp after it -
and uses no layer names (the synthetic model directories name layers differently from the reference's).  It inserts four weightless layers, so flownet.bin is
untouched."""
import os
import shutil

import numpy as np

import deep_ref

STOCK_INTERPS = [1 / 8, 8, 1 / 4, 1 / 4, 4, 1 / 2, 1 / 2, 2]
SCALED_INTERPS = [1 / 16, 16, 1 / 8, 1 / 8, 8, 1 / 4, 1 / 4, 4, 1 / 2, 1 / 2, 2]


def _f(v):
    return "%e" % v


def _parse(line):
    tok = line.split()
    nb, nt = int(tok[2]), int(tok[3])
    return {"type": tok[0], "name": tok[1], "bottoms": tok[4:4 + nb], "tops": tok[4 + nb:4 + nb + nt], "params": tok[4 + nb + nt:]}


def _emit(l):
    return "%-24s %-24s %d %d %s" % (l["type"], l["name"], len(l["bottoms"]), len(l["tops"]), " ".join(l["bottoms"] + l["tops"] + l["params"]))


def _get(l, key):
    for p in l["params"]:
        k, v = p.split("=", 1)
        if k == str(key):
            return v
    return None


def _set(l, key, value):
    l["params"] = [("%s=%s" % (key, value)) if p.split("=", 1)[0] == str(key) else p for p in l["params"]]


def rewrite_param(text):
    """flownet.param of rife-v4.6 -> the same graph at flow scale 2.  ValueError if the graph does not have the rife-v4.6 shape."""
    lines = text.strip("\n").split("\n")
    if len(lines) < 3 or lines[0].strip() != "7767517":
        raise ValueError("not an ncnn .param text")
    nl, nb = (int(v) for v in lines[1].split())
    layers = [_parse(s) for s in lines[2:] if s.strip()]
    if len(layers) != nl:
        raise ValueError("layer count does not match the header")
    interps = [l for l in layers if l["type"] == "Interp"]
    if len(interps) != 8 or any(abs(float(_get(l, 1)) - s) > 1e-6 or _get(l, 1) != _get(l, 2) for l, s in zip(interps, STOCK_INTERPS)):
        raise ValueError("not the rife-v4.6 graph: its eight Interp layers are 1/8, 8, 1/4, 1/4, 4, 1/2, 1/2, 2")
    # blocks 0..2: factors below 1 halved, above 1 doubled
    for l in interps:
        s = float(_get(l, 1))
        s = s / 2 if s < 1 else s * 2
        _set(l, 1, _f(s)); _set(l, 2, _f(s))
    # the scalar of the mul / div next to an Interp (one input, with_scalar, op 2 = mul / 3 = div)
    scal = [l for l in layers if l["type"] == "BinaryOp" and len(l["bottoms"]) == 1 and _get(l, 1) == "1" and _get(l, 0) in ("2", "3")]
    if [float(_get(l, 2)) for l in scal] != [8.0, 4.0, 2.0]:
        raise ValueError("not the rife-v4.6 graph: scalar mul 8, div 4, div 2 expected")
    for l in scal:
        _set(l, 2, _f(2 * float(_get(l, 2))))
    # the second coefficient of the two weighted sums
    elt = [l for l in layers if l["type"] == "Eltwise"]
    if [_get(l, -23301) and [float(v) for v in _get(l, -23301).split(",")] for l in elt] != [[2.0, 1.0, 4.0], [2.0, 1.0, 2.0]]:
        raise ValueError("not the rife-v4.6 graph: Eltwise sums with coefficients (1, 4) and (1, 2) expected")
    for l in elt:
        c = [float(v) for v in _get(l, -23301).split(",")]
        _set(l, -23301, "2,%s,%s" % (_f(c[1]), _f(2 * c[2])))
    # block 3: Interp(0.5) on the 8-channel concat, Interp(0.5) then / 2 on the flow concatenated to it
    cats = [i for i, l in enumerate(layers) if l["type"] == "Concat" and len(l["bottoms"]) == 2]
    ps = [i for i, l in enumerate(layers) if l["type"] == "PixelShuffle" and l["tops"] == ["flow3"]]
    if len(cats) != 3 or len(ps) != 1 or ps[0] < cats[-1]:
        raise ValueError("not the rife-v4.6 graph: three two-input Concats and a PixelShuffle that writes flow3 expected")
    ci = cats[-1]
    cat = layers[ci]
    x8, fl = cat["bottoms"]
    half = ["0=2", "1=" + _f(0.5), "2=" + _f(0.5)]
    new = [{"type": "Interp", "name": "fs2_interp_x", "bottoms": [x8], "tops": ["fs2_x"], "params": list(half)},
           {"type": "Interp", "name": "fs2_interp_f", "bottoms": [fl], "tops": ["fs2_f"], "params": list(half)},
           {"type": "BinaryOp", "name": "fs2_div_f", "bottoms": ["fs2_f"], "tops": ["fs2_fd"], "params": ["0=3", "1=1", "2=" + _f(2.0)]}]
    cat["bottoms"] = ["fs2_x", "fs2_fd"]
    layers[ci:ci] = new
    # Interp(2) on flow3, in front of everything that reads it
    pi = ps[0] + 3
    readers = [l for l in layers[pi + 1:] if "flow3" in l["bottoms"]]
    if len(readers) != 1:
        raise ValueError("not the rife-v4.6 graph: one reader of flow3 expected")
    readers[0]["bottoms"] = ["fs2_u" if b == "flow3" else b for b in readers[0]["bottoms"]]
    layers.insert(pi + 1, {"type": "Interp", "name": "fs2_interp_u", "bottoms": ["flow3"], "tops": ["fs2_u"], "params": ["0=2", "1=" + _f(2.0), "2=" + _f(2.0)]})
    # F = F * 1 + u[0:4] * 2 in place of the plain add: the first two-input BinaryOp after flow3
    adds = [l for l in layers[pi + 2:] if l["type"] == "BinaryOp" and len(l["bottoms"]) == 2]
    if not adds or _get(adds[0], 0) not in (None, "0"):
        raise ValueError("not the rife-v4.6 graph: a plain add of the block-3 flow expected")
    adds[0]["type"] = "Eltwise"
    adds[0]["params"] = ["0=1", "-23301=2,%s,%s" % (_f(1.0), _f(2.0))]
    return "\n".join(["7767517", "%d %d" % (nl + 4, nb + 4)] + [_emit(l) for l in layers]) + "\n"


def scaled_modeldir(modeldir, tmp):
    """A directory holding the rewritten flownet.param next to a copy of the original flownet.bin."""
    tmp = os.fspath(tmp)
    os.makedirs(tmp, exist_ok=True)
    with open(os.path.join(modeldir, "flownet.param")) as f:
        text = rewrite_param(f.read())
    with open(os.path.join(tmp, "flownet.param"), "w") as f:
        f.write(text)
    shutil.copyfile(os.path.join(modeldir, "flownet.bin"), os.path.join(tmp, "flownet.bin"))
    return tmp


def padded(w, h):
    return (w + 63) // 64 * 64, (h + 63) // 64 * 64


def planes(codes, depth):
    """(h, w, 3) integer codes -> (3, hp, wp) float32 planes zero-padded to 64n: code * (1 / max), as deep_ref.planes computes it."""
    h, w, _ = codes.shape
    wp, hp = padded(w, h)
    k = np.float32(1) / np.float32(deep_ref.MAXCODE[depth])
    p = np.zeros((3, hp, wp), np.float32)
    p[:, :h, :w] = (np.minimum(codes, deep_ref.MAXCODE[depth]).astype(np.float32) * k).transpose(2, 0, 1)
    return p


def net_inputs(a, b, t, depth, flows=()):
    h, w, _ = a.shape
    wp, hp = padded(w, h)
    inputs = {"in0": planes(a, depth), "in1": planes(b, depth), "in2": np.full((1, hp, wp), t, np.float32)}
    for k, f in enumerate(flows):
        inputs["flow%d" % k] = np.ascontiguousarray(f, np.float32)
    return inputs


def extract(oracle2, a, b, t, depth, blob, flows=()):
    """Blob `blob` of the oracle on the rewritten graph (optionally with blobs flow0.. injected, at hp/16 .. hp/2)."""
    h, w, _ = a.shape
    wp, hp = padded(w, h)
    return oracle2.net_extract(0, net_inputs(a, b, t, depth, flows), blob, 16 * wp * hp)


def expected_frame(oracle2, a, b, t, depth=8):
    h, w, _ = a.shape
    return deep_ref.quantise(extract(oracle2, a, b, t, depth, "out0"), w, h, depth)


def stage_blobs(text):
    """Blob names of the stages of the REWRITTEN graph (text of its flownet.param), found by structure as rewrite_param finds its layers:
      block0_in   the bottom of the first stride-2 Convolution (7 channels at 1/16)
      block_in    the tops of the three two-input Concats (12 channels at 1/8, 1/4, 1/2)
      stems       per block 0..3 the tops of its two stride-2 Convolutions
      F, M        the running flow and mask logit after the update of block 0..3: F = the top of the scalar mul, then of the three weighted Eltwise sums; M = the
                  Crop from channel 4 of the same upsampled flow, then the two-input adds that read that Crop (4 and 1 channels at full resolution; entries 0..2
                  are the tensors blocks 1..3 read, entry 3 is what the tail warps with)
    Split tops alias their bottom.  ValueError if the graph does not have that shape."""
    layers = [_parse(s) for s in text.strip("\n").split("\n")[2:] if s.strip()]
    prod = {t: l for l in layers for t in l["tops"]}

    def src(b):
        while b in prod and prod[b]["type"] == "Split":
            b = prod[b]["bottoms"][0]
        return b

    s2 = [l for l in layers if l["type"] == "Convolution" and _get(l, 3) == "2"]
    cats = [l for l in layers if l["type"] == "Concat" and len(l["bottoms"]) == 2]
    scal = [l for l in layers if l["type"] == "BinaryOp" and len(l["bottoms"]) == 1 and _get(l, 1) == "1" and _get(l, 0) == "2"]
    elt = [l for l in layers if l["type"] == "Eltwise" and _get(l, -23301)]
    if len(s2) != 8 or len(cats) != 3 or len(scal) != 1 or len(elt) != 3:
        raise ValueError("not the rewritten rife-v4.6 graph: 8 stride-2 Convolutions, 3 two-input Concats, 1 scalar mul and 3 weighted Eltwise sums expected")
    F, M = [], []
    for k, l in enumerate(scal + elt):
        crop = prod.get(l["bottoms"][-1])                     # Crop of channels 0..3 of u = Interp(flow_k)
        if crop is None or crop["type"] != "Crop" or prod[src(crop["bottoms"][0])]["type"] != "Interp":
            raise ValueError("not the rewritten rife-v4.6 graph: update %d does not read a Crop of an upsampled flow" % k)
        u = src(crop["bottoms"][0])
        mc = [c for c in layers if c["type"] == "Crop" and src(c["bottoms"][0]) == u and _get(c, -23309) == "1,4"]
        if len(mc) != 1:
            raise ValueError("not the rewritten rife-v4.6 graph: one Crop of the mask channel per update expected")
        m = mc[0]["tops"][0]
        if k:
            adds = [a for a in layers if a["type"] == "BinaryOp" and len(a["bottoms"]) == 2 and m in [src(b) for b in a["bottoms"]] and _get(a, 0) in (None, "0")]
            if len(adds) != 1:
                raise ValueError("not the rewritten rife-v4.6 graph: one add of the mask increment per update expected")
            m = adds[0]["tops"][0]
        F.append(l["tops"][0]); M.append(m)
    return {"block0_in": src(s2[0]["bottoms"][0]), "block_in": [l["tops"][0] for l in cats],
            "stems": [(s2[2 * b]["tops"][0], s2[2 * b + 1]["tops"][0]) for b in range(4)], "F": F, "M": M}


SCALES = (16, 8, 4, 2)
PEAK = (0.5, 0.12, 0.06, 0.03)      # peak displacement that blob k adds, as a share of the shorter padded side


def injected_flows_scaled(w, h, seed, n):
    """injected_flows with the amplitude tied to the frame: the same field recipe (sin x cos + noise, channels 4 and 5 as they are), but blob k moves samples by at
    most about PEAK[k] * min(wp, hp) pixels after the x s of its update, whatever the frame's size - so that a good part of the sampling positions stays inside
    the padded frame and a good part leaves it (inside_share; tests/test_flowscale_host.py holds that for every case of the GPU tests)."""
    wp, hp = padded(w, h)
    rng = np.random.default_rng(seed)
    out = []
    for k, s in enumerate(SCALES[:n]):
        H, W = hp // s, wp // s
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        f = np.empty((6, H, W), np.float32)
        amp = PEAK[k] * min(wp, hp) / s
        for c in range(4):
            ph = rng.uniform(0, 6.28, 2)
            f[c] = amp * np.sin(xx * (rng.uniform(0.5, 3.0) * 6.28 / W) + ph[0]) * np.cos(yy * (rng.uniform(0.5, 3.0) * 6.28 / H) + ph[1]) + rng.normal(0, 0.3 * amp / 8, (H, W))
        f[4] = rng.normal(0, 1.5, (H, W)); f[5] = rng.normal(0, 1.0, (H, W))
        out.append(f.astype(np.float32))
    return out


def inside_share(F):
    """F (4, hp, wp), the running flow at full resolution -> (share of the pixels whose sampling position (x + F.x, y + F.y) lies inside the padded frame, the
    same for (x + F.z, y + F.w), largest |displacement| in pixels)."""
    _, hp, wp = F.shape
    yy, xx = np.mgrid[0:hp, 0:wp].astype(np.float64)
    sh = []
    for c in (0, 2):
        px, py = xx + F[c], yy + F[c + 1]
        sh.append(float(((px >= 0) & (px <= wp - 1) & (py >= 0) & (py <= hp - 1)).mean()))
    return sh[0], sh[1], float(np.abs(F).max())


# The cases of tests/test_gpu_flowscale_gather.py: (w, h, seed) - each size the smallest that still reaches its edge.  Frames are noise for odd seeds and smooth
# for even ones; the flows are injected_flows_scaled(w, h, FLOW_SEED + seed, ..).
GATHER_CASES = [(1, 1, 1),          # 64x64: flow0 is 4x4, block 0's trunk 1x1; up_coeff's in - 2 edge
                (65, 64, 2),        # 128x64: one column past 64
                (100, 60, 3),       # 128x64
                (130, 9, 4),        # 192x64
                (8, 300, 5),        # 64x320
                (333, 241, 6),      # 384x256
                (640, 360, 7)]      # 640x384: the first size with two 32-wide tiles across in the scale-8 stem (Wo = 40); the scale-4 stem has three, the scale-2 stem five
FLOW_SEED = 100
FINAL_CASES = [(100, 60, 1), (333, 241, 4)]      # test_gpu_flowscale.py: k_final_scaled on four injected blobs


def injected_flows(w, h, seed, n):
    """tests/test_gpu_gather.py's injected_flows at the mode's sizes (its arguments fix 32n and the scales 8, 4, 2, 1): blobs flow0..flow{n-1},
    6 x hp/s x wp/s with s = 16, 8, 4, 2 of the frame padded to 64n - smooth fields + noise; after the x s of the flow update the coarse one moves samples by
    hundreds of pixels, the finer ones add tens; channel 4 = mask logit increments of a few units."""
    wp, hp = padded(w, h)
    rng = np.random.default_rng(seed)
    out = []
    for k, s in enumerate((16, 8, 4, 2)[:n]):
        H, W = hp // s, wp // s
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        f = np.empty((6, H, W), np.float32)
        amp = (40.0, 6.0, 3.0, 1.5)[k]
        for c in range(4):
            ph = rng.uniform(0, 6.28, 2)
            f[c] = amp * np.sin(xx * (rng.uniform(0.5, 3.0) * 6.28 / W) + ph[0]) * np.cos(yy * (rng.uniform(0.5, 3.0) * 6.28 / H) + ph[1]) + rng.normal(0, 0.3 * amp / 8, (H, W))
        f[4] = rng.normal(0, 1.5, (H, W)); f[5] = rng.normal(0, 1.0, (H, W))
        out.append(f.astype(np.float32))
    return out
