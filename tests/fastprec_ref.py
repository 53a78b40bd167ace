"""Fast precision (include/rife_hip.h rife_hip_set_precision) restated without a GPU: the reference of tests/test_fastprec_host.py and tests/test_gpu_fastprec.py.

One residual trunk layer x <- leaky(conv3x3(x) + b + x) on a tensor stored as {hi = f16(x), lo = f16(x - hi)} computes, in fast precision,

    acc = sum over the taps of W . hi  +  I . (hi + lo)          (fp32 accumulation)

then the unchanged epilogue (bias, LeakyReLU, split of the fp32 result into {hi, lo}).  The convolution sees its input rounded to f16, the skip connection does
not.  fast_trunk_layer() is that layer in float64, fast_exact_case() the exact inputs of tests/s16_ref.py with the expectation recomputed for it, FastNet the
whole network (tests/torch_graph.TorchNet) with the same rounding in front of every trunk convolution."""
import numpy as np
import torch

import s16_ref
from torch_graph import TorchNet


def fast_trunk_layer(hi, lo, w, b, slope):
    """y = conv3x3(hi, pad 1) + b + (hi + lo) in float64, then the fp32 slope multiply of s16_ref.trunk_layer.  Returns float64."""
    hi = np.asarray(hi, np.float64); lo = np.asarray(lo, np.float64)
    y = s16_ref.conv3x3_f64(hi, w) + np.asarray(b, np.float64)[:, None, None] + (hi + lo) + 0.0
    neg = (y.astype(np.float32) * np.float32(slope)).astype(np.float64)
    return np.where(y < 0, neg, y)


_CACHE = {}


def fast_exact_case(C, H, W, n_layers=1):
    """The inputs of s16_ref.cached_exact_case(C, H, W, n_layers) - x, w, b, slope 0.25 - with the expected tensors of fast precision, layer by layer.
    Asserts, on what it computed, the precondition that makes the expected bytes independent of the summation order: operands on the grid 2^-g, integer
    weights, every partial sum of |products| below 2^24 grid steps, an output that is exactly an fp32 value, and no f16-subnormal lo in it.
    Returns dict(x, w, b, slope, want [per layer, float64], full [s16_ref's full-precision expectation per layer]); computed once per process."""
    key = (C, H, W, n_layers)
    if key in _CACHE:
        return _CACHE[key]
    e = s16_ref.cached_exact_case(C, H, W, n_layers)
    g = 12 if n_layers == 1 else 10                                          # s16_ref.exact_case: the input grid
    assert e["slope"] == 0.25
    hi, lo = s16_ref.split(e["x"])
    wants = []
    for i in range(n_layers):
        w, b = e["w"][i], e["b"][i]
        h64, l64 = hi.astype(np.float64), lo.astype(np.float64)
        assert s16_ref._on_grid(h64, g) and s16_ref._on_grid(l64, g) and s16_ref._on_grid(b, g) and s16_ref._on_grid(w, 0), "layer %d: an operand off the grid" % i
        bound = float((s16_ref.conv3x3_f64(np.abs(h64), np.abs(w)) + np.abs(np.asarray(b, np.float64))[:, None, None] + np.abs(h64) + np.abs(l64)).max()) * 2.0 ** g
        assert bound < 2.0 ** 24, "layer %d: |partial sums| reach %.3g grid steps (limit 2^24)" % (i, bound)
        y = fast_trunk_layer(hi, lo, w, b, e["slope"])
        g += 2                                                               # y * 0.25
        assert s16_ref._on_grid(y, g) and np.array_equal(y.astype(np.float32).astype(np.float64), y), "layer %d: the output is not exactly an fp32 value" % i
        hi, lo = s16_ref.split(y.astype(np.float32))                         # what the kernel stores and the next layer reads
        assert np.all((lo == 0) | (np.abs(lo.astype(np.float64)) >= s16_ref.MIN_NORMAL_F16)), "layer %d: an f16-subnormal lo in the output" % i
        wants.append(y)
    _CACHE[key] = dict(x=e["x"], w=e["w"], b=e["b"], slope=e["slope"], want=wants, full=e["want"])
    return _CACHE[key]


def _resolve(blob, producer):
    """The blob a Split top stands for."""
    while blob in producer and producer[blob]["type"] == "Split":
        blob = producer[blob]["bottoms"][0]
    return blob


def trunk_convolutions(layers):
    """Names of the residual trunk convolutions, found structurally: a 3 x 3 stride-1 Convolution with as many input as output channels whose top is one input
    of a two-input add (BinaryOp, op 0) and whose own input (through Split layers) is the other."""
    producer = {t: l for l in layers for t in l["tops"]}
    out = []
    for l in layers:
        p = l["params"]
        if l["type"] != "Convolution" or int(p.get(1, 0)) != 3 or int(p.get(3, 1)) != 1 or int(p.get(6, 0)) != 9 * int(p[0]) * int(p[0]):
            continue
        src = _resolve(l["bottoms"][0], producer)
        for a in layers:
            if a["type"] == "BinaryOp" and len(a["bottoms"]) == 2 and int(a["params"].get(0, 0)) == 0 and l["tops"][0] in a["bottoms"]:
                other = [b for b in a["bottoms"] if b != l["tops"][0]]
                if len(other) == 1 and _resolve(other[0], producer) == src:
                    out.append(l["name"])
    return out


class FastNet(TorchNet):
    """TorchNet with the input of every residual trunk convolution rounded to f16 (round to nearest even) in front of the convolution only: the add still reads
    the unrounded blob.  rounding=False: TorchNet, bit for bit (the same per-layer evaluation, no rounding).  ValueError for a graph without such layers."""

    def __init__(self, param_path, bin_path, rounding=True):
        super().__init__(param_path, bin_path)
        self.trunk = set(trunk_convolutions(self.layers))
        if not self.trunk:
            raise ValueError("the graph has no residual trunk convolution (a 3 x 3 convolution added to its own input): fast precision is defined for rife-v4.6")
        self.rounding = rounding

    @torch.no_grad()
    def run(self, inputs, want):
        blobs = dict(inputs)
        one = object.__new__(TorchNet)                                       # TorchNet.run on one layer at a time: its arithmetic, layer by layer
        for l in self.layers:
            if l["type"] == "Input" or all(t in blobs for t in l["tops"]) or not all(b in blobs for b in l["bottoms"]):
                continue
            ins = {b: blobs[b] for b in l["bottoms"]}
            if self.rounding and l["name"] in self.trunk:
                ins = {b: v.to(torch.float16).to(torch.float32) for b, v in ins.items()}
            one.layers = [l]
            for t, v in zip(l["tops"], TorchNet.run(one, ins, l["tops"])):
                blobs[t] = v
        return [blobs[w] for w in want]


# ---- the end-to-end inputs of tests/test_gpu_fastprec.py (B1) and of the CPU model of the effect (tests/test_fastprec_host.py): (name, w, h, kind, seed, timestep,
# depth, flow scale).  kind: smooth / noise = tools/gen_frames; soft10 = 10-bit codes 384 + the smooth pair: every value of the low two bits, and edges of at
# most 255 codes per pixel.  (The model moves block-3 flows by up to 3e-3 px: across an edge of deep_ref.deep_pair's discs - up to 1023 codes per pixel - that is
# more than one 10-bit code before rounding, and the model's maximum was 1 or 2 codes depending on the CPU's convolution; under 255 codes per pixel it stays below one.)
B1_INPUTS = [
    ("rgb8-96x64", 96, 64, "smooth", 11, 0.5, 8, 1),
    ("rgb8-100x60", 100, 60, "smooth", 12, 0.7, 8, 1),
    ("rgb8-33x47", 33, 47, "smooth", 13, 0.3, 8, 1),
    ("rgb8-256x192", 256, 192, "smooth", 14, 0.5, 8, 1),
    ("rgb8-256x192-noise", 256, 192, "noise", 15, 0.25, 8, 1),
    ("rgb10-256x192", 256, 192, "soft10", 16, 0.5, 10, 1),
    ("rgb8-160x96-fs2", 160, 96, "smooth", 17, 0.6, 8, 2),
]


def b1_frames(inp):
    from tools import gen_frames
    _, w, h, kind, seed = inp[:5]
    if kind == "soft10":
        return tuple((f.astype(np.uint16) + np.uint16(384)) for f in gen_frames.smooth_pair(w, h, seed))
    return gen_frames.noise_pair(w, h, seed) if kind == "noise" else gen_frames.smooth_pair(w, h, seed)


_MODEL = {}


def model_effect(modeldir, inp, tmp=None):
    """The CPU model of fast precision on one B1 input: FastNet against TorchNet on the planes the engine feeds the network (deep_ref.planes; flow scale 2: the
    rewritten graph of tests/flowscale_ref.py on planes padded to 64n, `tmp` = a directory for it).
    Returns dict(max_codes, share, float_codes [max |out0(fast) - out0(full)| in codes, before quantisation], flow [max |flow_k(fast) - flow_k(full)| for
    k = 0..3], frame_fast, frame_full); computed once per process."""
    import os
    import deep_ref
    import flowscale_ref
    name, w, h, kind, seed, t, depth, fscale = inp
    if name in _MODEL:
        return _MODEL[name]
    a, b = b1_frames(inp)
    ref = deep_ref
    if fscale == 2:
        modeldir = flowscale_ref.scaled_modeldir(modeldir, tmp)
        ref = flowscale_ref
    paths = (os.path.join(modeldir, "flownet.param"), os.path.join(modeldir, "flownet.bin"))
    ins = {k: torch.from_numpy(v) for k, v in ref.net_inputs(a, b, t, depth).items()}
    blobs = ["flow0", "flow1", "flow2", "flow3", "out0"]
    full = TorchNet(*paths).run(ins, blobs)
    fast = FastNet(*paths).run(ins, blobs)
    f_full = deep_ref.quantise(full[4].numpy(), w, h, depth)
    f_fast = deep_ref.quantise(fast[4].numpy(), w, h, depth)
    d = np.abs(f_fast.astype(np.int32) - f_full.astype(np.int32))
    fc = float((fast[4][:, :h, :w] - full[4][:, :h, :w]).abs().max()) * deep_ref.MAXCODE[depth]
    _MODEL[name] = dict(max_codes=int(d.max()), share=float((d > 0).mean()), float_codes=fc, flow=[float((fast[k] - full[k]).abs().max()) for k in range(4)],
                        frame_fast=f_fast, frame_full=f_full)
    return _MODEL[name]
