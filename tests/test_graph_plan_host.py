"""The generic graph executor's load-time rewrites, decided without a device (rife_hip_graph_plan), and the pins of the two references of
tests/graph_ref.py to the CPU oracle.  The GPU side is tests/test_gpu_graph_exec.py."""
import importlib
import os

import numpy as np
import pytest

import graph_ref as gr
from tools import gen_models

amd = importlib.import_module("rife-ncnn-vulkan_amd").test_build()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_of(g, tmp_path, name="net"):
    base = os.path.join(str(tmp_path), name)
    with open(base + ".param", "w") as f:
        f.write(g.emit())
    return {l["name"]: l for l in amd.graph_plan(base)}


def layer_named(g, blob):
    return next(l["name"] for l in g.layers if blob in l["tops"])


def test_entry_points_are_declared_and_listed():
    hdr = open(os.path.join(ROOT, "include", "rife_hip_test.h")).read()
    for s in ("rife_hip_graph_plan", "rife_hip_graph_eval"):
        assert s in amd.TEST_ABI_SYMBOLS and s + "(" in hdr


# ---- Convolution + PReLU ------------------------------------------------------------------------------------------------------------------
def conv_prelu(readers=1, act=None, slopes=32, k=3):
    g = gen_models.Graph()
    x = g.input("x")
    y = g.conv(x, 16, 32, 1, leaky=0.2) if act == "leaky" else g.convk(x, 16, 32, k, act=act)
    p = g.prelu(y, slopes)
    if readers > 1:
        g.neg(y)
    return g, y, p


@pytest.mark.parametrize("k,cls", [(3, "g_conv3x3"), (5, "g_conv5x5"), (7, "direct")])
def test_prelu_folds_into_a_convolution_read_once(tmp_path, k, cls):
    g, y, p = conv_prelu(k=k)
    plan = plan_of(g, tmp_path)
    conv, prelu = plan[layer_named(g, y)], plan[layer_named(g, p)]
    assert prelu["fold"] == conv["name"] and prelu["out"] is None
    assert conv["fold"] is None and conv["out"] == p and conv["cls"] == cls and not conv["padded"]


@pytest.mark.parametrize("kw", [dict(readers=2), dict(act="leaky"), dict(act="sigmoid"), dict(slopes=1), dict(slopes=31)])
def test_prelu_does_not_fold(tmp_path, kw):
    """a second reader of the convolution's top, a fused activation, a slope count that is not the output channel count"""
    g, y, p = conv_prelu(**kw)
    plan = plan_of(g, tmp_path)
    conv, prelu = plan[layer_named(g, y)], plan[layer_named(g, p)]
    assert prelu["fold"] is None and prelu["out"] == p
    assert conv["out"] == y


def test_plan_names_classes_and_padding(tmp_path):
    g = gen_models.Graph()
    x = g.input("x")
    a = g.convk(x, 8, 6, 3, 2)
    b = g.convk(x, 8, 18, 5)
    c = g.deconv(x, 8, 2)
    d = g.convk(x, 8, 20, 1)
    e = g.convk(x, 8, 32, 3)
    plan = plan_of(g, tmp_path)
    got = {blob: (plan[layer_named(g, blob)]["cls"], plan[layer_named(g, blob)]["padded"], plan[layer_named(g, blob)]["kind"]) for blob in (a, b, c, d, e)}
    assert got == {a: ("g_conv3x3_s2", True, "Convolution"), b: ("g_conv5x5", True, "Convolution"), c: ("g_deconv4x4", True, "Deconvolution"),
                   d: ("direct", False, "ConvolutionDirect"), e: ("g_conv3x3", False, "Convolution")}


# ---- the squeeze-and-excitation tail ------------------------------------------------------------------------------------------------------
def se_folds(g, tmp_path):
    plan = plan_of(g, tmp_path)
    return [l for l in plan.values() if l["kind"] == "BinaryOp" and l["fold"]], plan


def test_se_tail_folds_on_the_generated_pattern(tmp_path):
    g, out, m, _ = gr.se_graph(16, "fold")
    folded, plan = se_folds(g, tmp_path)
    prelu = layer_named(g, out)
    assert len(folded) == 2 and all(l["fold"] == prelu and l["out"] is None for l in folded)
    assert plan[prelu]["fold"] is None and plan[prelu]["out"] == out


def se_variant(kind):
    g = gen_models.Graph()
    y, skip = g.input("y"), g.input("skip")
    m = g.pool_global_avg(y)
    m = g.inner(m, 16, 16, "leaky", 0.25)
    m = g.sigmoid(g.inner(m, 16, 16, None)) if kind == "sigmoid_layer" else g.inner(m, 16, 16, "sigmoid")
    mul = g.binary(y, m, 2)
    add = g.binary(mul, skip, 0)
    g.prelu(add, 16)
    if kind == "mul_read_twice":
        g.neg(mul)
    if kind == "add_read_twice":
        g.neg(add)
    return g


@pytest.mark.parametrize("kind", ["swapped", "sigmoid_layer", "mul_read_twice", "add_read_twice"])
def test_se_tail_does_not_fold(tmp_path, kind):
    g = gr.se_graph(16, "swapped")[0] if kind == "swapped" else se_variant(kind)
    folded, plan = se_folds(g, tmp_path)
    assert not folded
    assert all(l["out"] is not None for l in plan.values() if l["kind"] in ("BinaryOp", "PReLU"))


@pytest.mark.parametrize("fam", ["rife", "rife-HD"])
def test_every_se_block_of_the_generated_nets_folds(modeldirs, fam, monkeypatch):
    calls = {}
    real = gen_models._se_tail

    def counting(*a, **kw):
        calls["n"] = calls.get("n", 0) + 1
        return real(*a, **kw)
    monkeypatch.setattr(gen_models, "_se_tail", counting)
    for net, builder in gen_models.FAMILIES[fam].items():
        calls["n"] = 0
        builder()
        plan = amd.graph_plan(os.path.join(modeldirs[fam], net))
        tails = {l["fold"] for l in plan if l["kind"] == "BinaryOp" and l["fold"]}
        assert calls["n"] > 0 and len(tails) == calls["n"], (fam, net, len(tails), calls["n"])
        assert sum(1 for l in plan if l["kind"] == "BinaryOp" and l["fold"]) == 2 * calls["n"]
        # and every PReLU behind a convolution read once rides that convolution
        assert all(l["fold"] for l in plan if l["kind"] == "PReLU" and l["name"] not in tails)


# ---- the references against the CPU oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w", [(1, 5, 7), (3, 7, 9), (17, 9, 33), (16, 1, 1), (5, 1, 1)])
def test_float32_steps_equal_the_oracle_bit_for_bit(modeldirs, tmp_path, c, h, w):
    rng = np.random.default_rng(c * 100 + h)
    g, want = gr.elementwise_graph(c, h, w)
    base, _ = gr.write(str(tmp_path), "ew", g, rng, fp16=False)
    ins = gr.elementwise_inputs(c, h, w, rng)
    ref = gr.run_f32(base, ins, want)
    o = gr.oracle_for(base, modeldirs, tmp_path)
    for blob, r in zip(want, ref):
        got = o.net_extract(0, ins, blob, r.size + 16)
        assert gr.bits_equal(got.reshape(r.shape), r), (blob, np.abs(got.reshape(r.shape) - r).max())


@pytest.mark.parametrize("c", [16, 48])
def test_se_tail_steps_equal_the_oracle_bit_for_bit(modeldirs, tmp_path, c):
    rng = np.random.default_rng(c)
    g, out, m, _ = gr.se_graph(c, "fold")
    base, ws = gr.write(str(tmp_path), "se", g, rng)
    ins = {"y": rng.standard_normal((c, 9, 33)).astype(np.float32), "skip": rng.standard_normal((c, 9, 33)).astype(np.float32),
           m: rng.uniform(0, 1, (c, 1, 1)).astype(np.float32)}
    o = gr.oracle_for(base, modeldirs, tmp_path)
    got = o.net_extract(0, ins, out, c * 9 * 33)
    assert gr.bits_equal(got, gr.se_tail_f32(ins["y"], ins[m], ins["skip"], ws[-1][3]))
    assert gr.bits_equal(got, gr.run_f32(base, ins, [out])[0])


SMALL_CONVS = [cs for cs in gr.conv_cases() if cs["h"] * cs["w"] <= 24 * 64]


@pytest.mark.parametrize("cs", SMALL_CONVS, ids=[cs["name"] for cs in SMALL_CONVS])
def test_float64_torch_is_within_the_oracle_bar_on_the_convolutions(modeldirs, tmp_path, cs):
    """the bar of tests/test_oracle_vs_torch.py: 2e-4 absolute between the fp32 oracle and torch"""
    rng = np.random.default_rng(len(cs["name"]) * 131 + cs["cin"] + cs["cout"])
    g, want = gr.conv_graph(cs)
    base, _ = gr.write(str(tmp_path), "cv", g, rng, fp16=cs["fp16"])
    ins = gr.conv_inputs(cs, rng)
    ref = gr.run_f64(base, ins, want)
    o = gr.oracle_for(base, modeldirs, tmp_path)
    for blob, r in zip(want, ref):
        got = o.net_extract(0, ins, blob, r.size + 16)
        assert got.shape == r.shape and np.abs(got - r).max() < 2e-4, (blob, np.abs(got - r).max())
