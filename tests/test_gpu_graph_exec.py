"""The generic layer-wise graph executor (csrc/graph_exec.h, graph_run.h, graph_kernels.h: the v1 family) on micro-graphs, blob by blob, through
rife_hip_graph_eval - the product's graph_load and one graph_run per call.  References and graphs: tests/graph_ref.py (pinned to the CPU oracle by
tests/test_graph_plan_host.py).  Data movement and one-rounding arithmetic must be bit-exact; sigmoid, pooling and the convolutions have the bars
stated at each test.  RIFE_GRAPH_PARITY_OUT=<file>: every case appends its path (from the plan), bar and achieved distance there
(profiles/graph_exec/parity.txt is such a run)."""
import importlib
import os

import numpy as np
import pytest

import graph_ref as gr
from tools import gen_models

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()
EINVAL, EMODEL = 1, 4      # include/rife_hip.h


def record(case, path, bar, origin, got):
    out = os.environ.get("RIFE_GRAPH_PARITY_OUT")
    print("%-34s %-44s bar %-11.4g (%s) achieved %.4g" % (case, path, bar, origin, got))
    if out:
        with open(out, "a") as f:
            f.write("%-34s %-44s bar %-11.4g (%s) achieved %.4g\n" % (case, path, bar, origin, got))


def path_of(base):
    """the launches of a graph as the plan names them: kinds in file order, convolutions by profile class, folds marked"""
    parts = []
    for l in amd.graph_plan(base):
        if l["kind"] in ("Input", "Split"):
            continue
        parts.append((l["cls"] + ("+pad" if l["padded"] else "")) if l["cls"] else (l["kind"] + (">" + l["fold"] if l["fold"] else "")))
    return ",".join(parts)


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not gr.bits_equal(got, ref):
        bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != ref.view(np.uint32).reshape(-1))
        raise AssertionError("%s: %d of %d values differ, first at %d: %r vs %r" % (what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], ref.reshape(-1)[bad[0]]))


# ---- layer kinds, bit for bit ---------------------------------------------------------------------------------------------------------------
CHANNELS = (1, 2, 3, 5, 16, 17, 48)                     # pixel stride 16n > c, = c, and (at 1 x 1) the vector form
SIZES = ((1, 1), (5, 7), (7, 9), (9, 33), (24, 64))


@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("c", CHANNELS)
def test_layer_kinds_bit_for_bit(tmp_path, c, h, w):
    rng = np.random.default_rng(c * 1000 + h * 10 + w)
    g, want = gr.elementwise_graph(c, h, w)
    base, _ = gr.write(str(tmp_path), "ew", g, rng, fp16=False)
    ins = gr.elementwise_inputs(c, h, w, rng)
    ref = gr.run_f32(base, ins, want)
    got = amd.graph_eval(base, ins, want)
    for blob, a, r in zip(want, got, ref):
        assert_bits(a, r, "%s (%s)" % (blob, next(l["type"] for l in g.layers if blob in l["tops"])))
    record("kinds c=%d %dx%d" % (c, h, w), "%d blobs of every one-rounding kind" % len(want), 0.0, "bit-exact: one rounding per step", 0.0)


def test_blob_buffers_reused_across_sizes(tmp_path):
    """One instance at three sizes in one call sequence, large, small, medium: g_alloc re-uses the buffers of the first run (and clears them for the new
    geometry).  Every run must give the bytes of a fresh instance at that size."""
    c = 5
    rng = np.random.default_rng(11)
    g = gen_models.Graph()
    a = g.input("a")
    n1 = g.neg(a)
    y = g.convk(g.concat([n1, g.scalar(a, 2, 0.5)]), 2 * c, 6, 3)
    cat = g.concat([y, a])
    base, _ = gr.write(str(tmp_path), "reuse", g, rng, fp16=False)
    runs = []
    for k, (h, w) in enumerate(((24, 64), (5, 7), (9, 33))):
        x = rng.standard_normal((c, h, w)).astype(np.float32)
        runs.append((x, amd.graph_eval(base, {"a": x}, [n1, y, cat], keep=k < 2)))
    fresh = [amd.graph_eval(base, {"a": x}, [n1, y, cat]) for x, _ in runs]
    for (x, got), want in zip(runs, fresh):
        for a_, b_ in zip(got, want):
            assert_bits(a_, b_, "re-used instance against a fresh one")
    assert_bits(runs[1][1][2][6:], runs[1][0], "the neighbour behind a 6-channel convolution")
    # the same buffer with FEWER channels: what the 12-channel run left in channels 5 .. 11 is pad now, and the convolution behind reads its input in
    # 16-channel chunks - zero weights there, but 0 x inf is NaN unless g_alloc cleared the buffer for the new geometry
    g = gen_models.Graph()
    n1 = g.neg(g.input("a"))
    y = g.convk(n1, 5, 8, 3)
    base, _ = gr.write(str(tmp_path), "stale", g, rng, fp16=False)
    amd.graph_eval(base, {"a": np.full((12, 9, 33), np.inf, np.float32)}, [n1], keep=True)
    x = rng.standard_normal((5, 9, 33)).astype(np.float32)
    got = amd.graph_eval(base, {"a": x}, [y])[0]
    assert np.isfinite(got).all()
    assert_bits(got, amd.graph_eval(base, {"a": x}, [y])[0], "a convolution behind a blob that shrank")


# ---- sigmoid --------------------------------------------------------------------------------------------------------------------------------
def sigmoid_inputs(rng, shape):
    v = rng.uniform(-20.0, 20.0, shape).astype(np.float32)
    v.reshape(-1)[:5] = (-20.0, 20.0, 0.0, -1e-3, 1e-30)
    return v


def check_sigmoid(case, base, got, v):
    """|got - ref64| <= 2^-22 ref64 for |v| <= 20: expf 1 ulp, the add and the correctly rounded divide half an ulp each, doubled"""
    ref = 1.0 / (1.0 + np.exp(-v.astype(np.float64)))
    rel = (np.abs(got.astype(np.float64) - ref) / ref).max()
    record(case, path_of(base), 2.0 ** -22, "relative; expf 1 ulp + add, divide 1/2 ulp each, x 2", rel)
    assert got.shape == v.shape and rel <= 2.0 ** -22, (case, rel)


@pytest.mark.parametrize("shape", [(5, 9, 33), (17, 1, 1), (16, 24, 64)])
def test_sigmoid_layer(tmp_path, shape):
    rng = np.random.default_rng(shape[0])
    g = gen_models.Graph()
    s = g.sigmoid(g.input("v"))
    base, _ = gr.write(str(tmp_path), "sig", g, rng)
    v = sigmoid_inputs(rng, shape)
    check_sigmoid("sigmoid layer %dx%dx%d" % shape, base, amd.graph_eval(base, {"v": v}, [s])[0], v)


@pytest.mark.parametrize("k,c", [(3, 4), (5, 8), (1, 20)])
def test_sigmoid_fused_on_a_convolution(tmp_path, k, c):
    """9=4 on a convolution whose weights copy the input (one-hot centre taps, no bias; c is no multiple of 16, so the fp32 kernels run and the
    copy is exact): what remains is the pointwise pass behind the convolution."""
    rng = np.random.default_rng(k)
    g = gen_models.Graph()
    s = g.convk(g.input("v"), c, c, k, bias=False, act="sigmoid")
    w = np.zeros((c, c, k, k), np.float32)
    w[np.arange(c), np.arange(c), k // 2, k // 2] = 1.0
    base, _ = gr.write(str(tmp_path), "sigc", g, rng, weights={0: w})
    v = sigmoid_inputs(rng, (c, 9, 33))
    check_sigmoid("sigmoid on conv %dx%d" % (k, k), base, amd.graph_eval(base, {"v": v}, [s])[0], v)


def test_sigmoid_on_inner_product(tmp_path):
    rng = np.random.default_rng(3)
    c = 17
    g = gen_models.Graph()
    s = g.inner(g.input("v"), c, c, "sigmoid")
    base, _ = gr.write(str(tmp_path), "sigfc", g, rng, weights={0: np.eye(c, dtype=np.float32)[::-1]})      # out[o] = x[c - 1 - o], exactly
    v = sigmoid_inputs(rng, (c, 1, 1))
    check_sigmoid("sigmoid on InnerProduct", base, amd.graph_eval(base, {"v": v}, [s])[0][::-1], v)


# ---- global average pooling -----------------------------------------------------------------------------------------------------------------
POOLS = [(4, 1, 1), (4, 5, 7), (4, 33, 65), (4, 530, 512), (12, 5, 7), (12, 33, 65), (48, 33, 65), (48, 530, 512), (1024, 1, 1), (1024, 5, 7), (1024, 33, 65)]


@pytest.mark.parametrize("c,h,w", POOLS)
def test_pooling_is_the_rounded_float64_mean(tmp_path, c, h, w):
    """530 x 512 pixels are more than 512 chunks of 512: nchunks saturates.  The kernel accumulates in double, so the result is the float64 mean rounded
    once: |got - mean| <= 2^-23 |mean| + 2^-149."""
    rng = np.random.default_rng(c + h)
    g = gen_models.Graph()
    p = g.pool_global_avg(g.input("x"))
    base, _ = gr.write(str(tmp_path), "pool", g, rng)
    x = (rng.standard_normal((c, h, w)) + rng.uniform(-1, 1, (c, 1, 1))).astype(np.float32)
    got = amd.graph_eval(base, {"x": x}, [p])[0]
    mean = x.astype(np.float64).mean(axis=(1, 2)).reshape(c, 1, 1)
    over = (np.abs(got - mean) - (2.0 ** -23 * np.abs(mean) + 2.0 ** -149)).max()
    record("pooling c=%d %dx%d" % (c, h, w), path_of(base), 2.0 ** -23, "relative; double accumulation, one rounding", (np.abs(got - mean) / np.abs(mean)).max())
    assert got.shape == (c, 1, 1) and over <= 0, over


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------------
CONVS = gr.conv_cases()


@pytest.mark.parametrize("cs", CONVS, ids=[cs["name"] for cs in CONVS])
def test_convolution_through_the_executor(tmp_path, cs):
    """Bars of tests/test_gpu_kernels.py against float64 (graph_ref.conv_bar): conv_tol for the fp32 kernels and the direct kernel,
    4e-6 max|want| + 1e-6 for the split-f16 kernels."""
    rng = np.random.default_rng(len(cs["name"]) * 131 + cs["cin"] + cs["cout"])
    g, want = gr.conv_graph(cs)
    base, ws = gr.write(str(tmp_path), "cv", g, rng, fp16=cs["fp16"])
    plan = amd.graph_plan(base)
    conv = next(l for l in plan if l["cls"])
    k, s = cs["k"], cs["stride"]
    assert conv["cls"] == ("g_deconv4x4" if cs["deconv"] else "g_conv5x5" if k == 5 else ("g_conv3x3_s2" if s == 2 else "g_conv3x3") if k == 3 else "direct")
    assert conv["padded"] == (cs["cout"] % 4 != 0)
    assert [l["fold"] for l in plan if l["kind"] == "PReLU"] == ([conv["name"]] if cs["tail"] == "prelu" else [None] if cs["tail"] else [])
    ins = gr.conv_inputs(cs, rng)
    ref = gr.run_f64(base, ins, want)
    got = amd.graph_eval(base, ins, want)
    bar = gr.conv_bar(cs, ins["x"], ws[0][1], ref[0])
    origin = "4e-6 max|want| + 1e-6, split-f16" if gr.conv_is_split_f16(cs) else "conv_tol, fp32"
    for blob, a, r in zip(want, got, ref):
        assert a.shape == r.shape, (blob, a.shape, r.shape)
    err = max(np.abs(a - r).max() for a, r in zip(got, ref))
    record(cs["name"], path_of(base), bar, origin, err)
    assert err <= bar, (cs["name"], err, bar)
    if cs["cout"] % 4:                                   # zero filters pad the output channels: the Concat behind must not carry them into its neighbour
        cat = got[-1]
        assert_bits(cat[cs["cout"]:], ins["n"], "the neighbour's channels behind the padded convolution")
        assert_bits(cat[:cs["cout"]], got[0], "the convolution's channels through the Concat")


# ---- the SE tail as run ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fold", "swapped", "reader"])
@pytest.mark.parametrize("c,h,w", [(16, 9, 33), (48, 24, 64), (48, 5, 7)])
def test_se_tail_folded_and_unfolded_equal_the_three_steps(tmp_path, c, h, w, form):
    """The tail of tools/gen_models._se_res and _se_down (one _se_tail; they differ in where skip comes from) with y, the scale vector and skip bound:
    kg_se_tail (form "fold") and the three separate launches (the two forms the loader must not fold) both equal mul, add, PReLU rounded one by one."""
    rng = np.random.default_rng(c + h)
    g, out, m, extra = gr.se_graph(c, form)
    base, ws = gr.write(str(tmp_path), "se", g, rng)
    folds = [l for l in amd.graph_plan(base) if l["kind"] == "BinaryOp" and l["fold"]]
    assert len(folds) == (2 if form == "fold" else 0)
    ins = {"y": rng.standard_normal((c, h, w)).astype(np.float32), "skip": rng.standard_normal((c, h, w)).astype(np.float32),
           m: rng.uniform(0, 1, (c, 1, 1)).astype(np.float32)}
    want = [out] + ([extra] if extra else [])
    got = amd.graph_eval(base, ins, want)
    assert_bits(got[0], gr.se_tail_f32(ins["y"], ins[m], ins["skip"], ws[-1][3]), "SE tail, form " + form)
    for a, r in zip(got, gr.run_f32(base, ins, want)):
        assert_bits(a, r, "SE tail against the step evaluation, form " + form)
    record("se tail c=%d %dx%d %s" % (c, h, w, form), path_of(base), 0.0, "bit-exact: three roundings", 0.0)


def test_se_block_whole(tmp_path):
    """pooling, both InnerProducts (leaky, sigmoid) and the folded tail in one run against float64: the scale is a sigmoid of a 16-term sum of O(1) values
    (2^-22 relative plus the sum's 17 x 2^-24 relative to its terms), the tail adds three roundings: 2^-20 of max|want| covers it 4 times over."""
    rng = np.random.default_rng(5)
    c = 48
    g, out, m, _ = gr.se_graph(c, "fold")
    base, _ = gr.write(str(tmp_path), "se", g, rng)
    ins = {"y": rng.standard_normal((c, 33, 65)).astype(np.float32), "skip": rng.standard_normal((c, 33, 65)).astype(np.float32)}
    got = amd.graph_eval(base, ins, [out, m])
    ref = gr.run_f64(base, ins, [out, m])
    for a, r, name in zip(got, ref, ("out", "scale")):
        err, bar = np.abs(a - r).max(), 2.0 ** -20 * np.abs(r).max()
        record("se block c=48 33x65 " + name, path_of(base), bar, "2^-20 max|want|", err)
        assert a.shape == r.shape and err <= bar, (name, err, bar)


# ---- refusals: by name, before anything is launched -----------------------------------------------------------------------------------------
def refused(code, text, base, ins, want):
    with pytest.raises(amd.RifeError) as e:
        amd.graph_eval(base, ins, want)
    assert "(-%d)" % code in str(e.value) and text in str(e.value), str(e.value)


def test_refusals(tmp_path):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((16, 5, 7)).astype(np.float32)
    g, out, m, _ = gr.se_graph(16, "fold")
    base, _ = gr.write(str(tmp_path), "se", g, rng)
    ins = {"y": x, "skip": x, m: np.ones((16, 1, 1), np.float32)}
    for blob in (g.blobs["mul"], g.blobs["add"]):
        refused(EINVAL, "no launch writes blob " + blob, base, ins, [blob])
        refused(EINVAL, "binding blob " + blob, base, dict(ins, **{blob: x}), [out])
    g = gen_models.Graph()
    y = g.convk(g.input("x"), 16, 16, 3)
    p = g.prelu(y, 16)
    base, _ = gr.write(str(tmp_path), "pair", g, rng)
    refused(EINVAL, "no launch writes blob " + y, base, {"x": x}, [y])
    refused(EINVAL, "binding blob " + y, base, {y: x}, [p])
    assert amd.graph_eval(base, {"x": x}, [p])[0].shape == (16, 5, 7)      # the pair itself runs
    g = gen_models.Graph()
    i = g.interp(g.input("x"), 2.0)
    base, _ = gr.write(str(tmp_path), "interp", g, rng)
    for shape in ((3, 5, 1), (3, 1, 7)):
        refused(EMODEL, "Interp from a blob one pixel wide or high", base, {"x": np.ones(shape, np.float32)}, [i])
    g = gen_models.Graph()
    p = g.pool_global_avg(g.input("x"))
    base, _ = gr.write(str(tmp_path), "pool6", g, rng)
    refused(EMODEL, "global pooling needs a channel count that is a multiple of 4", base, {"x": np.ones((6, 5, 7), np.float32)}, [p])


# ---- the real nets, stage by stage ----------------------------------------------------------------------------------------------------------
REAL = [(fam, net, W, H) for fam in ("rife", "rife-HD") for net, sizes in (("flownet", ((64, 64), (96, 160))), ("contextnet", ((64, 64),)), ("fusionnet", ((64, 64),)))
        for W, H in sizes]


@pytest.mark.parametrize("fam,net,W,H", REAL, ids=["%s-%s-%dx%d" % r for r in REAL])
def test_real_nets_stage_by_stage(modeldirs, fam, net, W, H):
    """Every stage of the generated rife / rife-HD nets (graph_ref.real_net_stages) with its inputs bound from the float64 run, so that no error
    accumulates and both sides warp with the same flow.  The bar of a blob is measured on the reference side: d = max|oracle - float64| of that stage
    (the fp32 CPU oracle under the same bindings), bar = 8 d, floored at 2^-20 max|float64|.  The factor 8: tests/test_gpu_kernels.py holds the
    split-f16 kernels to 4e-6 where the fp32 path measures 0.7e-6, and a lost lo plane is about 5e-4."""
    from oracle import pyoracle
    import torch
    which = ("flownet", "contextnet", "fusionnet").index(net)
    base = os.path.join(modeldirs[fam], net)
    nets, inputs = gr.real_net_inputs(modeldirs[fam], W, H, 40 + which)
    stages = gr.real_net_stages(base + ".param", amd.graph_plan(base))
    assert len(stages) >= 4
    names = sorted({b for want, bind in stages for b in bind + [want]} - set(inputs[net]))
    vals = dict(inputs[net])
    vals.update(zip(names, (v.numpy() for v in nets[net].run({k: torch.from_numpy(v) for k, v in inputs[net].items()}, names))))
    o = pyoracle.OracleRIFE()
    o.load(modeldirs[fam])
    failures = []
    for i, (want, bind) in enumerate(stages):
        b32 = {k: np.ascontiguousarray(vals[k], np.float32) for k in bind}
        (ref,) = nets[net].run({k: torch.from_numpy(v.astype(np.float64)) for k, v in b32.items()}, [want])
        ref = ref.numpy()
        orc = o.net_extract(which, b32, want, ref.size + 16)
        (got,) = amd.graph_eval(base, b32, [want], keep=i + 1 < len(stages))
        assert orc.shape == ref.shape == got.shape, (want, orc.shape, ref.shape, got.shape)
        d = np.abs(orc - ref).max()
        bar = max(8 * d, 2.0 ** -20 * np.abs(ref).max())
        err = np.abs(got - ref).max()
        record("%s %s %dx%d %s" % (fam, net, W, H, want), "stage %d of %d" % (i + 1, len(stages)), bar,
               "8 d, d = %.3g" % d if bar == 8 * d else "2^-20 max|f64|, d = %.3g" % d, err)
        if err > bar:
            failures.append((want, err, bar))
    assert not failures, failures
