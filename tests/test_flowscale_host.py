"""Flow scale 2 without a GPU: the structural rewrite of flownet.param (tests/flowscale_ref.py), the oracle on the rewritten graph, that oracle against the
independent PyTorch executor (the bounds of tests/test_oracle_vs_torch.py), and the public surface (header, C_ABI_SYMBOLS)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import flowscale_ref
from oracle import pyoracle
from tools import gen_frames, ncnn_param
from torch_graph import TorchNet

amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scaled(modeldirs, tmp_path_factory):
    return flowscale_ref.scaled_modeldir(modeldirs["rife-v4.6"], tmp_path_factory.mktemp("v46_fs2"))


@pytest.fixture(scope="module")
def oracle2(scaled):
    o = pyoracle.OracleRIFE(rife_v4=True)
    o.load(scaled)
    return o


def test_rewritten_graph_structure(modeldirs, scaled):
    stock = ncnn_param.parse(os.path.join(modeldirs["rife-v4.6"], "flownet.param"))
    new = ncnn_param.parse(os.path.join(scaled, "flownet.param"))
    factors = [l["params"][1] for l in new if l["type"] == "Interp"]
    assert factors == flowscale_ref.SCALED_INTERPS
    assert all(l["params"][1] == l["params"][2] for l in new if l["type"] == "Interp")
    head = lambda d: [int(v) for v in open(os.path.join(d, "flownet.param")).read().split("\n")[1].split()]
    assert head(modeldirs["rife-v4.6"]) == [215, 276] and head(scaled) == [219, 280]
    assert len(new) == len(stock) + 4
    blobs = lambda ls: {t for l in ls for t in l["tops"]}
    assert len(blobs(new)) == len(blobs(stock)) + 4
    # the doubled scalars (mul 16, div 8, div 4) and block 3's own / 2; the rsub 1 of the mask is untouched
    scal = [(int(l["params"][0]), l["params"][2]) for l in new if l["type"] == "BinaryOp" and len(l["bottoms"]) == 1]
    assert scal == [(2, 16.0), (3, 8.0), (3, 4.0), (3, 2.0), (7, 1.0)]
    # the doubled coefficients, and F = F * 1 + u * 2 in place of block 3's plain add
    assert [list(l["arrays"][1]) for l in new if l["type"] == "Eltwise"] == [[1.0, 8.0], [1.0, 4.0], [1.0, 2.0]]
    assert sum(l["type"] == "BinaryOp" and len(l["bottoms"]) == 2 and int(l["params"].get(0, 0)) == 0 for l in stock) - \
        sum(l["type"] == "BinaryOp" and len(l["bottoms"]) == 2 and int(l["params"].get(0, 0)) == 0 for l in new) == 1
    # every other layer is the stock one, in order
    kept = [(l["type"], l["name"]) for l in new if not l["name"].startswith("fs2_")]
    assert [k[1] for k in kept] == [l["name"] for l in stock]
    assert sum(a[0] != l["type"] for a, l in zip(kept, stock)) == 1
    with open(os.path.join(modeldirs["rife-v4.6"], "flownet.bin"), "rb") as f0, open(os.path.join(scaled, "flownet.bin"), "rb") as f1:
        assert f0.read() == f1.read()


@pytest.mark.parametrize("fam", ["rife-v4", "rife-v2.3"])
def test_rewrite_refuses_other_families(modeldirs, fam):
    with open(os.path.join(modeldirs[fam], "flownet.param")) as f:
        text = f.read()
    with pytest.raises(ValueError):
        flowscale_ref.rewrite_param(text)


def test_rewrite_refuses_garbage():
    with pytest.raises(ValueError):
        flowscale_ref.rewrite_param("not a param file\n")


@pytest.mark.parametrize("w,h,wp,hp", [(96, 64, 128, 64), (33, 47, 64, 64), (1, 1, 64, 64)])
def test_oracle_shapes_on_the_rewritten_graph(oracle2, w, h, wp, hp):
    assert flowscale_ref.padded(w, h) == (wp, hp)
    a, b = gen_frames.smooth_pair(w, h, 5)
    for k, s in enumerate((16, 8, 4, 2)):
        f = flowscale_ref.extract(oracle2, a, b, 0.5, 8, "flow%d" % k)
        assert f.shape == (6, hp // s, wp // s)
    assert flowscale_ref.extract(oracle2, a, b, 0.5, 8, "out0").shape == (3, hp, wp)
    assert flowscale_ref.expected_frame(oracle2, a, b, 0.5, 8).shape == (h, w, 3)


@pytest.mark.parametrize("w,h,t,seed", [(96, 64, 0.5, 1), (100, 60, 0.7, 3)])
def test_rewritten_graph_oracle_matches_torch(scaled, oracle2, w, h, t, seed):
    net = TorchNet(os.path.join(scaled, "flownet.param"), os.path.join(scaled, "flownet.bin"))
    a, b = gen_frames.smooth_pair(w, h, seed)
    ins = {k: torch.from_numpy(v) for k, v in flowscale_ref.net_inputs(a, b, t, 8).items()}
    outs = net.run(ins, ["flow0", "flow1", "flow2", "flow3", "out0"])
    for k in range(4):
        f = flowscale_ref.extract(oracle2, a, b, t, 8, "flow%d" % k)
        assert f.shape == tuple(outs[k].shape)
        assert np.abs(f - outs[k].numpy()).max() < 1e-4, k
    o = outs[4][:, :h, :w] * 255.0 + 0.5
    tu8 = o.to(torch.int32).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    ou8 = flowscale_ref.expected_frame(oracle2, a, b, t, 8)
    diff = np.abs(ou8.astype(int) - tu8.astype(int))
    assert diff.max() <= 1
    assert (diff > 0).mean() < 0.02


def test_injected_blobs_reach_the_rewritten_graph(scaled, oracle2):
    """The oracle with flow0..3 injected at the mode's sizes is the torch executor with the same blobs: the reference of the injected-flow GPU tests."""
    w, h = 100, 60
    net = TorchNet(os.path.join(scaled, "flownet.param"), os.path.join(scaled, "flownet.bin"))
    a, b = gen_frames.smooth_pair(w, h, 7)
    inj = flowscale_ref.injected_flows(w, h, 11, 4)
    assert [f.shape for f in inj] == [(6, 4, 8), (6, 8, 16), (6, 16, 32), (6, 32, 64)]
    got = flowscale_ref.extract(oracle2, a, b, 0.4, 8, "out0", flows=inj)
    ins = {k: torch.from_numpy(v) for k, v in flowscale_ref.net_inputs(a, b, 0.4, 8, inj).items()}
    (want,) = net.run(ins, ["out0"])
    assert np.abs(got - want.numpy()).max() < 1e-4


def test_stage_blobs_of_the_rewritten_graph(modeldirs, scaled, oracle2):
    """flowscale_ref.stage_blobs: the names the gather tests of flow scale 2 extract - counts, the layers behind them, and their shapes on the oracle."""
    with open(os.path.join(scaled, "flownet.param")) as f:
        text = f.read()
    sb = flowscale_ref.stage_blobs(text)
    assert len(sb["block_in"]) == 3 and len(sb["stems"]) == 4 and len(sb["F"]) == 4 and len(sb["M"]) == 4
    names = [sb["block0_in"]] + sb["block_in"] + [n for p in sb["stems"] for n in p] + sb["F"] + sb["M"]
    assert len(set(names)) == len(names) == 20
    layers = ncnn_param.parse(os.path.join(scaled, "flownet.param"))
    prod = {t: l for l in layers for t in l["tops"]}
    assert prod[sb["block0_in"]]["type"] == "Interp" and prod[sb["block0_in"]]["params"][1] == 1 / 16
    assert all(prod[n]["type"] == "Concat" for n in sb["block_in"])
    assert [prod[n]["params"][0] for p in sb["stems"] for n in p] == [96, 192, 64, 128, 48, 96, 32, 64]
    assert [prod[n]["type"] for n in sb["F"]] == ["BinaryOp", "Eltwise", "Eltwise", "Eltwise"]
    assert [list(prod[n]["arrays"][1]) for n in sb["F"][1:]] == [[1.0, 8.0], [1.0, 4.0], [1.0, 2.0]]
    assert [prod[n]["type"] for n in sb["M"]] == ["Crop", "BinaryOp", "BinaryOp", "BinaryOp"]
    with open(os.path.join(modeldirs["rife-v4"], "flownet.param")) as f:
        with pytest.raises(ValueError):
            flowscale_ref.stage_blobs(f.read())
    for w, h, wp, hp in ((64, 64, 64, 64), (100, 60, 128, 64)):
        a, b = gen_frames.smooth_pair(w, h, 5)
        inj = flowscale_ref.injected_flows_scaled(w, h, 3, 4)
        assert [f.shape for f in inj] == [(6, hp // s, wp // s) for s in flowscale_ref.SCALES]
        ex = lambda n: flowscale_ref.extract(oracle2, a, b, 0.5, 8, n, flows=inj).shape
        assert ex(sb["block0_in"]) == (7, hp // 16, wp // 16)
        for k, s in enumerate((8, 4, 2)):
            assert ex(sb["block_in"][k]) == (12, hp // s, wp // s)
        for k, (s, C) in enumerate(zip(flowscale_ref.SCALES, (192, 128, 96, 64))):
            assert ex(sb["stems"][k][0]) == (C // 2, hp // s // 2, wp // s // 2) and ex(sb["stems"][k][1]) == (C, hp // s // 4, wp // s // 4)
        for k in range(4):
            assert ex(sb["F"][k]) == (4, hp, wp) and ex(sb["M"][k]) == (1, hp, wp)


def test_scaled_flows_keep_their_recipe_and_peak():
    """injected_flows_scaled is injected_flows with another amplitude: the same draws in the same order (channels 4 and 5 bit for bit), peaks tied to the frame."""
    for w, h in ((100, 60), (640, 360)):
        wp, hp = flowscale_ref.padded(w, h)
        old, new = flowscale_ref.injected_flows(w, h, 9, 4), flowscale_ref.injected_flows_scaled(w, h, 9, 4)
        for k, s in enumerate(flowscale_ref.SCALES):
            assert new[k].shape == old[k].shape and np.array_equal(new[k][4:], old[k][4:])
            ratio = flowscale_ref.PEAK[k] * min(wp, hp) / s / (40.0, 6.0, 3.0, 1.5)[k]
            assert np.allclose(new[k][:4], old[k][:4] * ratio, rtol=1e-5, atol=1e-6)
            assert np.abs(new[k][:4]).max() * s <= 1.5 * flowscale_ref.PEAK[k] * min(wp, hp)


_SHARE_CASES = [(w, h, flowscale_ref.FLOW_SEED + seed, n) for w, h, seed in flowscale_ref.GATHER_CASES for n in (1, 2, 3)] + \
               [(w, h, flowscale_ref.FLOW_SEED + seed, 4) for w, h, seed in flowscale_ref.FINAL_CASES]


@pytest.mark.parametrize("w,h,fseed,n", _SHARE_CASES)
def test_injected_flows_look_inside_the_frame_and_outside(scaled, oracle2, w, h, fseed, n):
    """The condition that keeps the injected-flow tests of flow scale 2 from looking at clamps only, or at none: for every case they use - the n blobs block n reads
    (n = 1..3), or all four for k_final_scaled - the sampling positions x + F of BOTH frames, from the oracle's F blob after the last injected update, lie inside the
    padded frame for at least a quarter and at most nine tenths of the pixels, and the largest displacement exceeds a quarter of the shorter padded side."""
    with open(os.path.join(scaled, "flownet.param")) as f:
        sb = flowscale_ref.stage_blobs(f.read())
    wp, hp = flowscale_ref.padded(w, h)
    a, b = gen_frames.smooth_pair(w, h, 1)
    inj = flowscale_ref.injected_flows_scaled(w, h, fseed, n)
    F = flowscale_ref.extract(oracle2, a, b, 0.5, 8, sb["F"][n - 1], flows=inj)
    s0, s1, peak = flowscale_ref.inside_share(F)
    print("flow scale 2 gather, %dx%d (%dx%d) %d blobs: inside share %.2f / %.2f, largest displacement %.1f px" % (w, h, wp, hp, n, s0, s1, peak))
    assert 0.25 <= s0 <= 0.90 and 0.25 <= s1 <= 0.90
    assert peak > min(wp, hp) / 4


def test_header_declares_and_python_lists_the_calls():
    with open(os.path.join(ROOT, "include", "rife_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+rife_hip_set_flow_scale\s*\(\s*rife_hip_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint\s+rife_hip_flow_scale\s*\(\s*const\s+rife_hip_t\s*\*\s*\w+\s*\)\s*;", header)
    assert "rife_hip_set_flow_scale" in amd.C_ABI_SYMBOLS and "rife_hip_flow_scale" in amd.C_ABI_SYMBOLS
    assert callable(getattr(amd.RIFE, "set_flow_scale", None)) and isinstance(amd.RIFE.flow_scale, property)
