"""Micro-graphs for the generic layer-wise graph executor (csrc/graph_exec.h, graph_run.h, graph_kernels.h) and their references.

Two references, both independent of the engine:

* `run_f32`: a float32 STEP-BY-STEP numpy evaluation, one rounding per arithmetic operation in the order the ncnn layer performs them.  The data-movement
  layers and the layers whose arithmetic is one rounded operation per step (neg, Clip, ReLU, PReLU, BinaryOp, Eltwise, the SE tail as three operations,
  InnerProduct as a sequential sum in index order) must match it BIT FOR BIT: the library is built with -ffp-contract=off, so the kernels round after every
  operation as well.  rife.Warp and Interp come from the oracle's single-op entry points (pyoracle.warp / pyoracle.interp).
  tests/test_graph_plan_host.py pins this evaluation to OracleRIFE.net_extract bit for bit.
* `run_f64`: tests/torch_graph.TorchNet in float64, for everything else (convolutions, sigmoid, pooling).

Graphs are built with tools/gen_models.Graph and written with seeded weights by `write()`.
"""
import os
import shutil

import numpy as np
import torch

from oracle import pyoracle
from tools import gen_models, ncnn_param
from torch_graph import TorchNet, load_bin


# ----------------------------------------------------------------------------------------------
# writing a micro-graph
# ----------------------------------------------------------------------------------------------
def synth(g, rng, fp16=True, weights=None):
    """Seeded weights for every weighted layer of `g` in .bin order: (type, weight, bias | None, slopes | None) like gen_models.synth_weights.
    fp16: weights are fp16 numbers (the split-f16 kernel paths); else they keep 24 significant bits (the fp32 paths).  weights: {layer index among the
    weighted layers: array} overrides."""
    out = []
    for i, l in enumerate(g.weighted()):
        m = l["meta"]
        if "slope" in m:
            out.append(("prelu", None, None, rng.uniform(0.05, 0.5, m["slope"]).astype(np.float32)))
            continue
        oc, ic, kh, kw = m["w"]
        w = rng.standard_normal((oc, ic, kh, kw)) / np.sqrt(ic * kh * kw / (4.0 if l["type"] == "Deconvolution" else 1.0))
        w = w.astype(np.float16).astype(np.float32) if fp16 else w.astype(np.float32)
        if weights and i in weights:
            w = np.asarray(weights[i], np.float32).reshape(oc, ic, kh, kw)
        b = (rng.standard_normal(oc) * 0.1).astype(np.float32) if m.get("bias", True) else None
        out.append((l["type"], w, b, None))
    return out


def write(dirpath, name, g, rng, fp16=True, weights=None):
    """<dirpath>/<name>.param + .bin; returns (base path, the weight list)."""
    os.makedirs(dirpath, exist_ok=True)
    base = os.path.join(dirpath, name)
    with open(base + ".param", "w") as f:
        f.write(g.emit())
    ws = synth(g, rng, fp16, weights)
    (gen_models.write_bin if fp16 else gen_models.write_bin_f32)(base + ".bin", ws)
    return base, ws


def oracle_for(base, modeldirs, tmpdir):
    """An OracleRIFE whose flownet is the micro-graph at `base`: the oracle's loader wants three nets, so the generated contextnet / fusionnet of the
    rife family stand next to it."""
    d = os.path.join(str(tmpdir), "oracle_" + os.path.basename(base))
    os.makedirs(d, exist_ok=True)
    for ext in (".param", ".bin"):
        shutil.copyfile(base + ext, os.path.join(d, "flownet" + ext))
        for net in ("contextnet", "fusionnet"):
            shutil.copyfile(os.path.join(modeldirs["rife"], net + ext), os.path.join(d, net + ext))
    o = pyoracle.OracleRIFE()
    o.load(d)
    return o


# ----------------------------------------------------------------------------------------------
# float32 step-by-step evaluation
# ----------------------------------------------------------------------------------------------
_F = np.float32


def _binop(op, a, b):
    return {0: lambda: a + b, 1: lambda: a - b, 2: lambda: a * b, 3: lambda: a / b, 7: lambda: b - a}[op]()


def run_f32(base, inputs, want):
    """inputs: {blob: (C, H, W) float32}, vectors as (C, 1, 1).  Every intermediate is a float32 array: numpy rounds each operation once."""
    layers = ncnn_param.parse(base + ".param")
    load_bin(layers, base + ".bin")
    blobs = {k: np.ascontiguousarray(v, _F) for k, v in inputs.items()}
    producer = {t: i for i, l in enumerate(layers) for t in l["tops"]}
    need, stack = set(), [w for w in want if w not in blobs]
    while stack:                                          # Extractor semantics: only what the wanted blobs need, cut at the bound blobs
        i = producer[stack.pop()]
        if i not in need:
            need.add(i)
            stack.extend(b for b in layers[i]["bottoms"] if b not in blobs)
    for i, l in enumerate(layers):
        t, p, a = l["type"], l["params"], l["arrays"]
        if i not in need:
            continue
        x = [blobs[b] for b in l["bottoms"]]
        x0 = x[0]
        with np.errstate(all="ignore"):
            if t == "Split":
                for o in l["tops"]:
                    blobs[o] = x0
                continue
            if t == "Concat":
                y = np.concatenate(x, 0)
            elif t == "Crop":
                c1 = a[10][0]
                y = x0[int(a[9][0]): x0.shape[0] if c1 >= 2147483647 else int(c1)]
            elif t == "PixelShuffle":
                r = int(p[0]); c, h, w = x0.shape
                y = x0.reshape(c // (r * r), r, r, h, w).transpose(0, 3, 1, 4, 2).reshape(c // (r * r), h * r, w * r)
            elif t == "UnaryOp":
                assert int(p[0]) == 1
                y = -x0
            elif t == "Clip":
                y = x0.copy(); y[y < _F(p[0])] = _F(p[0]); y[y > _F(p[1])] = _F(p[1])
            elif t == "ReLU":
                s = _F(p.get(0, 0.0))
                y = np.where(x0 < 0, _F(0) if s == 0 else x0 * s, x0)             # ncnn: max(x, 0) for slope 0, x * slope below zero otherwise
            elif t == "PReLU":
                y = np.where(x0 < 0, x0 * l["slope"].numpy().astype(_F)[:, None, None], x0)
            elif t == "BinaryOp":
                y = _binop(int(p.get(0, 0)), x0, x[1] if len(x) > 1 else _F(p[2]))
            elif t == "Eltwise":
                c = a.get(1)
                y = x0 * _F(c[0]) + x[1] * _F(c[1]) if c else x0 + x[1]
            elif t == "InnerProduct":
                w = l["weight"].numpy().astype(_F)
                v = x0.reshape(-1)
                s = l["bias"].numpy().astype(_F).copy() if l["bias"] is not None else np.zeros(w.shape[0], _F)
                for j in range(v.size):
                    s = s + v[j] * w[:, j]
                act = int(p.get(9, 0))
                if act == 1:
                    s = np.where(s > 0, s, _F(0))
                elif act == 2:
                    s = np.where(s > 0, s, s * _F(a[10][0]))
                else:
                    assert act == 0, "sigmoid is not a one-rounding operation"
                y = s.reshape(-1, 1, 1)
            elif t == "rife.Warp":
                y = pyoracle.warp(x0, x[1][:2])
            elif t == "Interp":
                hs, ws = _F(p.get(1, 1.0)), _F(p.get(2, 1.0))
                y = x0 if (int(x0.shape[1] * hs), int(x0.shape[2] * ws)) == x0.shape[1:] else pyoracle.interp(x0, float(hs), float(ws))
            else:
                raise NotImplementedError("%s has no float32 step-by-step form: compare it with run_f64" % t)
        assert y.dtype == _F, (t, y.dtype)
        blobs[l["tops"][0]] = np.ascontiguousarray(y)
    return [blobs[w] for w in want]


def run_f64(base, inputs, want):
    """TorchNet in float64; inputs as for run_f32; 1-D results come back as (C, 1, 1)."""
    net = TorchNet(base + ".param", base + ".bin", dtype=torch.float64)
    outs = net.run({k: torch.from_numpy(np.ascontiguousarray(v, np.float64)) for k, v in inputs.items()}, want)
    return [o.numpy().reshape(-1, 1, 1) if o.dim() == 1 else o.numpy() for o in outs]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, _F), np.ascontiguousarray(b, _F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------------------------
# the micro-graphs
# ----------------------------------------------------------------------------------------------
BINOPS = (0, 1, 2, 3, 7)
SCALAR = 0.37


def away_from_zero(rng, shape):
    """divisors: magnitude in [0.5, 2), either sign"""
    return (rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(_F)


def elementwise_graph(c, h, w):
    """Every data-movement and one-rounding layer kind in ONE graph at c channels, h x w pixels - each kind twice, the second reading the first's result
    (a blob the executor allocated: pixel stride 16n > c unless c = 16n), and a Concat behind each pair, so a kernel that mistook the pixel stride for the
    channel count, or wrote into a neighbour's channels, shows.  Returns (graph, wanted blobs); inputs: elementwise_inputs()."""
    g = gen_models.Graph()
    a, b0, bv, b1, fl, ps = (g.input(n) for n in ("a", "b0", "bv", "b1", "fl", "ps"))
    want = []

    def pair(f):
        o1 = f(a); o2 = f(o1)
        want.extend([o1, o2, g.concat([o1, o2, a])])

    pair(lambda x: g.neg(x))
    pair(lambda x: g.clip(x, -0.5, 0.7))
    pair(lambda x: g.leaky(x, 0.0))
    pair(lambda x: g.leaky(x, 0.2))
    pair(lambda x: g.prelu(x, c))
    for op in BINOPS:
        pair(lambda x: g.scalar(x, op, SCALAR))
        for other in (b0, bv, b1):                      # same shape, per-channel vector, one channel broadcast over channels
            pair(lambda x: g.add("BinaryOp", [x, other], ["0=%d" % op]))
    pair(lambda x: g.wsum(x, b0, 0.75, -1.3))
    pair(lambda x: g.add("Eltwise", [x, b0], ["0=1"]))
    pair(lambda x: g.warp(x, fl))
    cat = g.concat([a, b0]); want.append(cat)
    cr = g.crop(cat, 1, c + 1); want.extend([cr, g.crop(cr, 0, 2147483647), g.crop(cat, c, 2147483647)])
    p1 = g.pixelshuffle(ps, 2); p2 = g.pixelshuffle(g.concat([ps, ps]), 2)
    want.extend([p1, p2, g.concat([p1, g.crop(p2, 0, c)])])
    if h >= 2 and w >= 2:
        for s in (0.5, 0.25, 2.0, 4.0):
            if int(h * s) >= 1 and int(w * s) >= 1:
                i1 = g.interp(a, s); i2 = g.interp(b0, s)
                want.extend([i1, i2, g.concat([i1, i2])])
    # InnerProduct on the vector: bias + relu, plain, leaky; 16-wide middle like the SE bottleneck
    f1 = g.add("InnerProduct", [bv], ["0=16", "1=1", "2=%d" % (16 * c), "9=1"], meta=dict(w=(16, c, 1, 1), kind="fc", bias=True))
    f2 = g.add("InnerProduct", [f1], ["0=%d" % c, "1=1", "2=%d" % (16 * c)], meta=dict(w=(c, 16, 1, 1), kind="fc", bias=True))
    f3 = g.inner(f2, c, 17, "leaky", 0.3)
    want.extend([f1, f2, f3, g.concat([f2, bv])])
    return g, want


def elementwise_inputs(c, h, w, rng):
    flow = rng.standard_normal((2, h, w)) * 12.0 + rng.choice([-30.0, 0.0, 25.0], (2, h, w))      # many taps leave the frame by tens of pixels
    return {"a": rng.standard_normal((c, h, w)).astype(_F), "b0": away_from_zero(rng, (c, h, w)), "bv": away_from_zero(rng, (c, 1, 1)),
            "b1": away_from_zero(rng, (1, h, w)), "fl": flow.astype(_F), "ps": rng.standard_normal((4 * c, h, w)).astype(_F)}


def se_graph(c, form):
    """The tail of a squeeze-and-excitation block (tools/gen_models._se_tail) at c channels: Pooling -> InnerProduct(16, leaky) -> InnerProduct(c, sigmoid)
    -> BinaryOp mul(y, .) -> BinaryOp add(., skip) -> PReLU.  form "fold": as generated (the loader folds the last three into kg_se_tail); "swapped": the
    add's operands exchanged; "reader": a second reader of the mul's result - neither folds.  Returns (graph, out blob, the fc blob to bind)."""
    g = gen_models.Graph()
    y, skip = g.input("y"), g.input("skip")
    m = g.pool_global_avg(y)
    m = g.inner(m, c, 16, "leaky", 0.25)
    m = g.inner(m, 16, c, "sigmoid")
    mul = g.binary(y, m, 2)
    add = g.binary(skip, mul, 0) if form == "swapped" else g.binary(mul, skip, 0)
    out = g.prelu(add, c)
    extra = g.neg(mul) if form == "reader" else None
    g.blobs = dict(out=out, m=m, mul=mul, add=add, extra=extra)
    return g, out, m, extra


def se_tail_f32(y, scale, skip, slopes):
    """the tail as three separately rounded float32 operations"""
    v = (y * scale.reshape(-1, 1, 1)).astype(_F)
    v = (v + skip).astype(_F)
    return np.where(v < 0, (v * slopes[:, None, None]).astype(_F), v)


# ----------------------------------------------------------------------------------------------
# convolutions through the executor
# ----------------------------------------------------------------------------------------------
def _cc(name, cin, cout, k, stride, h, w, fp16=True, bias=True, act=None, tail=None, deconv=False):
    return dict(name=name, cin=cin, cout=cout, k=k, stride=stride, h=h, w=w, fp16=fp16, bias=bias, act=act, tail=tail, deconv=deconv)


def conv_cases():
    """act: None | "leaky" (9=2) | "sigmoid" (9=4); tail: None | "prelu" (folds into the convolution) | "prelu2" (the convolution's top has a second reader:
    no fold).  Sizes h x w are the smallest that still have ragged tiles (5 x 7, 9 x 33), more than one 32-wide tile (24 x 64), and the three at which the
    launcher changes kernel: 384 workgroups of 8-row tiles (two rows per wave) and 448 (conv_mfma8_kernel), see engine_dispatch.h."""
    cs = []
    for s in (1, 2):
        for fp16 in (True, False):
            for bias in (True, False):
                cs.append(_cc("c3_s%d_%s_%s" % (s, "h" if fp16 else "f", "b" if bias else "nb"), 16, 32, 3, s, 9, 33, fp16, bias))
        cs.append(_cc("c3_s%d_cin6" % s, 6, 32, 3, s, 24, 64))                               # fp16 weights, but no split-f16 kernel for 6 channels
    cs.append(_cc("c3_leaky", 16, 32, 3, 1, 9, 33, act="leaky"))
    cs.append(_cc("c3_leaky_f", 8, 16, 3, 2, 9, 33, fp16=False, act="leaky"))
    cs.append(_cc("c3_prelu", 16, 48, 3, 1, 24, 64, tail="prelu"))
    cs.append(_cc("c3_prelu_f", 5, 48, 3, 2, 9, 33, fp16=False, tail="prelu"))
    cs.append(_cc("c3_prelu2", 16, 48, 3, 1, 9, 33, tail="prelu2"))
    cs.append(_cc("c3_prelu2_f", 8, 32, 3, 1, 5, 7, fp16=False, tail="prelu2"))
    for cout in (2, 6, 18):                                                                  # output channels padded to 4n with zero filters
        cs.append(_cc("c3_cout%d" % cout, 16, cout, 3, 1, 24, 64))
        cs.append(_cc("c3_cout%d_f_s2" % cout, 5, cout, 3, 2, 5, 7, fp16=False, tail="prelu"))
        cs.append(_cc("c5_cout%d" % cout, 8, cout, 5, 1, 9, 33, bias=False))
    for s in (1, 2):
        for (h, w), (cin, cout) in zip(((5, 7), (9, 33), (24, 64)), ((6, 32), (8, 48), (20, 64))):
            cs.append(_cc("c5_s%d_%dx%d" % (s, h, w), cin, cout, 5, s, h, w))
            cs.append(_cc("c5_s%d_%dx%d_f_prelu" % (s, h, w), cin, cout, 5, s, h, w, fp16=False, tail="prelu"))
        cs.append(_cc("c5_s%d_20_32_5x7" % s, 20, 32, 5, s, 5, 7, bias=False))
        cs.append(_cc("c5_s%d_6_64_24x64" % s, 6, 64, 5, s, 24, 64, tail="prelu2"))
    cs.append(_cc("c5_ms2_256x192", 8, 64, 5, 1, 192, 256))                                  # 8 x 24 x 2 = 384 workgroups of 8-row tiles: MS = 2
    cs.append(_cc("c3_ms2_256x384_f", 8, 32, 3, 1, 384, 256, fp16=False))                    # 8 x 48 x 1 = 384: MS = 2, fp32
    cs.append(_cc("c3_mfma8_128x224_f", 16, 256, 3, 1, 224, 128, fp16=False))                # 4 x 28 x 4 = 448 workgroups: conv_mfma8_kernel
    cs.append(_cc("c3_generic_128x216_f", 16, 256, 3, 1, 216, 128, fp16=False))              # 4 x 27 x 4 = 432: one tile row less, the generic kernel
    for k in (1, 7):
        for s in (1, 2):
            for cout in (4, 20):
                cs.append(_cc("direct_k%d_s%d_cout%d" % (k, s, cout), 5, cout, k, s, 9, 33, fp16=(cout == 4), bias=(k == 1), tail="prelu" if s == 2 else None))
    cs.append(_cc("dc_prelu", 16, 32, 4, 2, 9, 33, tail="prelu", deconv=True))
    cs.append(_cc("dc_prelu_f", 8, 20, 4, 2, 5, 7, fp16=False, tail="prelu", deconv=True))
    cs.append(_cc("dc_sigmoid", 16, 4, 4, 2, 24, 64, act="sigmoid", deconv=True))
    cs.append(_cc("dc_sigmoid_f", 32, 4, 4, 2, 5, 7, fp16=False, act="sigmoid", deconv=True))
    return cs


def conv_graph(cs):
    """x -> convolution [-> PReLU]; a convolution whose output channel count is no multiple of 4 is followed by Concat([result, n]) with a 3-channel
    neighbour n, which must come through exactly.  Returns (graph, wanted blobs: the result first)."""
    g = gen_models.Graph()
    x = g.input("x")
    cin, cout, k = cs["cin"], cs["cout"], cs["k"]
    if cs["deconv"]:
        y = g.deconv(x, cin, cout, sigmoid=cs["act"] == "sigmoid", kind="plain")
    elif cs["act"] == "leaky":
        assert k == 3 and cs["bias"]
        y = g.conv(x, cin, cout, cs["stride"], leaky=0.2, kind="plain")
    else:
        y = g.convk(x, cin, cout, k, cs["stride"], bias=cs["bias"], act=cs["act"])
    out, want = y, []
    if cs["tail"]:
        out = g.prelu(y, cout)
    want.append(out)
    if cs["tail"] == "prelu2":
        want.append(g.neg(y))
    if cout % 4:
        want.append(g.concat([out, g.input("n")]))
    return g, want


def conv_out_size(cs):
    return (2 * cs["h"], 2 * cs["w"]) if cs["deconv"] else ((cs["h"] - 1) // cs["stride"] + 1, (cs["w"] - 1) // cs["stride"] + 1)


def conv_inputs(cs, rng):
    ins = {"x": rng.standard_normal((cs["cin"], cs["h"], cs["w"])).astype(_F)}
    if cs["cout"] % 4:
        ins["n"] = rng.standard_normal((3,) + conv_out_size(cs)).astype(_F)
    return ins


def conv_is_split_f16(cs):
    """The split-f16 kernels (conv_h2*_kernel, head_h2_kernel) take a 3 x 3 / 4 x 4-transposed layer whose weights are fp16 numbers and whose input
    channel count is a multiple of 16 (csrc/engine_layers.h upload_layer, csrc/engine_dispatch.h conv_is_h2 / conv_is_h2s2 / conv_is_head_h2); every other
    layer runs in fp32 (conv_mfma_kernel, conv_mfma8_kernel, kg_conv_direct)."""
    return cs["fp16"] and cs["k"] in (3, 4) and cs["cin"] % 16 == 0


def conv_bar(cs, x, w, want):
    """tests/test_gpu_kernels.py: conv_tol for the fp32 kernels and the direct kernel, 4e-6 max|want| + 1e-6 for the split-f16 kernels.  A sigmoid behind the
    convolution divides the convolution's error by at least 4 (its slope is at most 1/4) and adds its own 2^-22 (relative, of a value below 1)."""
    if conv_is_split_f16(cs):
        if cs["act"] != "sigmoid":
            return 4e-6 * np.abs(want).max() + 1e-6
        pre = np.abs(np.log(want) - np.log1p(-want)).max()                     # max |convolution result| from the float64 sigmoid values
        return (4e-6 * pre + 1e-6) / 4 + 2.0 ** -22
    tol = 2e-5 * (1.0 + np.abs(w).sum(axis=(1, 2, 3)).max() * np.abs(x).max())
    return tol / 4 + 2.0 ** -22 if cs["act"] == "sigmoid" else tol


# ----------------------------------------------------------------------------------------------
# the real v1-family nets, stage by stage
# ----------------------------------------------------------------------------------------------
def real_net_stages(param_path, plan):
    """[(wanted blob, blobs to bind)] of a generated flownet / contextnet / fusionnet of the v1 family (tools/gen_models.py), found from the graph itself:
    flownet - each IFNet block's delta (the PixelShuffle result, resized where the block is coarse) from the frames and the earlier deltas, then `flow`;
    contextnet - f1 .. f4 from the frame, the flow and the previous level's feature blob; fusionnet - each encoder level (the PReLU closing an SE tail,
    `plan` names them) from the inputs and the level before, then `output` from the inputs and every level.  Bound blobs are never a Split's output."""
    layers = ncnn_param.parse(param_path)
    alias = {t: l["bottoms"][0] for l in layers if l["type"] == "Split" for t in l["tops"]}
    inputs = [l["tops"][0] for l in layers if l["type"] == "Input"]
    if "input0" in inputs:
        deltas = []
        for l in layers:
            if l["type"] == "PixelShuffle":
                up = [m["tops"][0] for m in layers if m["type"] == "Interp" and alias.get(m["bottoms"][0], m["bottoms"][0]) == l["tops"][0]]
                deltas.append(up[0] if up else l["tops"][0])
        return [(d, inputs + deltas[:b]) for b, d in enumerate(deltas)] + [("flow", list(deltas))]
    if "input.1" in inputs:
        warps = [l for l in layers if l["type"] == "rife.Warp"]
        xs = [alias.get(l["bottoms"][0], l["bottoms"][0]) for l in warps]
        return [(l["tops"][0], inputs + ([xs[i - 1]] if i else [])) for i, l in enumerate(warps)]
    tails = {l["fold"] for l in plan if l["kind"] == "BinaryOp" and l["fold"]}
    s = [l["tops"][0] for l in layers if l["name"] in tails]
    return [(b, inputs + ([s[i - 1]] if i else [])) for i, b in enumerate(s)] + [("output", inputs + s)]


def real_net_inputs(modeldir, W, H, seed):
    """float64 inputs of the three nets of one model directory for a smooth frame pair, chained as the engine chains them (tests/test_oracle_vs_torch.py):
    {net: {blob: (C, H, W) float64}}."""
    from tools import gen_frames
    a, b = gen_frames.smooth_pair(W, H, seed)
    x0, x1 = ((f.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1).astype(np.float64) for f in (a, b))
    nets = {n: TorchNet(os.path.join(modeldir, n + ".param"), os.path.join(modeldir, n + ".bin"), dtype=torch.float64) for n in ("flownet", "contextnet", "fusionnet")}
    t = torch.from_numpy
    (flow,) = nets["flownet"].run({"input0": t(x0), "input1": t(x1)}, ["flow"])
    c0 = nets["contextnet"].run({"input.1": t(x0), "flow.0": flow}, ["f1", "f2", "f3", "f4"])
    c1 = nets["contextnet"].run({"input.1": t(x1), "flow.1": flow}, ["f1", "f2", "f3", "f4"])
    fus = {"img0": x0, "img1": x1, "flow": flow.numpy()}
    for k in range(4):
        fus[str(3 + k)] = c0[k].numpy()
        fus[str(7 + k)] = c1[k].numpy()
    return nets, {"flownet": {"input0": x0, "input1": x1}, "contextnet": {"input.1": x1, "flow.1": flow.numpy()}, "fusionnet": fus}
