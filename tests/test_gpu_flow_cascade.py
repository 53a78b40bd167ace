"""k_flow_cascade (csrc/flow_cascade.h): F and M after blocks 1 and 2 written from the coarse flows alone, staged through LDS, against the sequential
k_flow_update launches it replaces - bit for bit.

  1. tap 6 (k_flow_cascade<b> on b injected flows) against tap 4 (k_flow_update after every injected flow), b = 2 and 3, on frames from one 32-pixel unit
     (every pixel a border pixel) to sizes that are no multiple of the 64 x 16 tile, with flows whose amplitudes leave the frame; for b = 3 also against the
     oracle's block-3 input, whose channels 7..11 are M and F;
  2. whole frames: the pass with RIFE_HIP_FLOW_CASCADE=0 (test build: k_flow_update2 + k_flow_update<2, false>) against the default pass, same bytes, also
     under hipGraph replay in a child process;
  3. the profile class "flow_update" has two launches per pair in both settings.
"""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from tools import gen_frames

from test_gpu_gather import injected_flows

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
amd_t = amd.test_build()      # librife_hip_test.so: the taps and the RIFE_HIP_FLOW_CASCADE switch (the product ignores it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engines(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    gt = amd_t.RIFE(0, rife_v4=True); gt.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.load(d)
    name3 = None      # block 3's input: the top of the third two-input Concat (cat_12 of the reference's flownet.param:165)
    n = 0
    for line in open(os.path.join(d, "flownet.param")):
        f = line.split()
        if len(f) > 6 and f[0] == "Concat" and f[2] == "2" and f[3] == "1":
            n += 1
            if n == 3:
                name3 = f[6]
    assert name3 is not None
    return g, gt, o, name3


TAP_SIZES = [(32, 32, 1), (33, 47, 2), (100, 60, 3), (333, 241, 4), (640, 360, 5)]


@pytest.mark.parametrize("w,h,seed", TAP_SIZES)
@pytest.mark.parametrize("b", [2, 3])
def test_cascade_writes_the_F_M_of_the_sequential_updates(engines, w, h, seed, b):
    _, gt, o, name3 = engines
    a, c = gen_frames.noise_pair(w, h, seed) if seed % 2 else gen_frames.smooth_pair(w, h, seed)
    inj = injected_flows(w, h, 500 + seed, b)
    want = gt.v4_tap(a, c, 0.5, 4, b, inj)
    got = gt.v4_tap(a, c, 0.5, 6, b, inj)
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    assert got.shape == want.shape == (5, hp, wp)
    assert np.abs(want[:4]).max() > min(100, w), "injected flows too small to leave the frame"
    assert np.array_equal(got, want), "%d of %d floats differ, first at %s" % (int((got != want).sum()), want.size, np.argwhere(got != want)[0])
    if b == 3:      # scale 1: channels 7..11 of the oracle's block input ARE M and F
        blob = o.v4_extract(a, c, 0.5, name3, flows=inj)
        assert np.array_equal(got[4], blob[7]) and np.array_equal(got[:4], blob[8:12])


@pytest.mark.parametrize("w,h,seed", [(33, 47, 1), (100, 60, 2), (640, 360, 3), (1920, 1080, 4)])
def test_pass_without_the_cascade_is_bit_identical(engines, w, h, seed, monkeypatch):
    g, gt, _, _ = engines
    for pair in (gen_frames.noise_pair, gen_frames.smooth_pair):
        a, b = pair(w, h, 70 + seed)
        for t in (0.5, 0.2):
            monkeypatch.delenv("RIFE_HIP_FLOW_CASCADE", raising=False)
            x1, x1t = g.process(a, b, t), gt.process(a, b, t)
            monkeypatch.setenv("RIFE_HIP_FLOW_CASCADE", "0")      # read by every plain pass of the test build
            x0 = gt.process(a, b, t)
            assert np.array_equal(x0, x1), "%d bytes differ" % int((x0 != x1).sum())
            assert np.array_equal(x0, x1t), "%d bytes differ (test build)" % int((x0 != x1t).sum())


def test_cascade_under_graph_replay(engines, modeldirs, monkeypatch):
    """The default pass captured and replayed as a hipGraph (RIFE_HIP_GRAPH=1 is read once per process: a child) against the pass without the cascade here."""
    _, gt, _, _ = engines
    code = (
        "import sys, hashlib, importlib\n"
        "sys.path.insert(0, %r)\n"
        "from tools import gen_frames\n"
        "amd = importlib.import_module('rife-ncnn-vulkan_amd')\n"
        "g = amd.RIFE(0, rife_v4=True); g.load(%r)\n"
        "for (w, h) in ((100, 60), (640, 360), (100, 60)):\n"
        "    for i, t in enumerate((0.5, 0.25)):\n"
        "        a, b = gen_frames.smooth_pair(w, h, 90 + i)\n"
        "        print('MD5', w, h, i, hashlib.md5(g.process(a, b, t).tobytes()).hexdigest())\n") % (ROOT, modeldirs["rife-v4.6"])
    env = dict(os.environ, RIFE_HIP_GRAPH="1")
    env.pop("RIFE_HIP_FLOW_CASCADE", None)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    got = [l.split() for l in p.stdout.splitlines() if l.startswith("MD5")]
    assert len(got) == 6
    monkeypatch.setenv("RIFE_HIP_FLOW_CASCADE", "0")
    for _, w, h, i, md5 in got:
        a, b = gen_frames.smooth_pair(int(w), int(h), 90 + int(i))
        assert md5 == hashlib.md5(gt.process(a, b, (0.5, 0.25)[int(i)]).tobytes()).hexdigest(), (w, h, i)


@pytest.mark.parametrize("setting", [None, "0"])
def test_flow_update_class_has_two_launches_per_pair(engines, setting, monkeypatch):
    _, gt, _, _ = engines
    if setting is None: monkeypatch.delenv("RIFE_HIP_FLOW_CASCADE", raising=False)
    else: monkeypatch.setenv("RIFE_HIP_FLOW_CASCADE", setting)
    a, b = gen_frames.smooth_pair(640, 360, 5)
    gt.process(a, b, 0.5)
    gt.profile_enable(True)
    try:
        gt.process(a, b, 0.5)
        prof = gt.profile_read()
    finally:
        gt.profile_enable(False)
    assert prof["flow_update"]["launches"] == 2, prof["flow_update"]
