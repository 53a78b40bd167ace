"""tests/tail_ref.py without a GPU: the float64 definition of the fused tails against a scalar loop and against the rife.Warp of tests/torch_graph.py, the
workgroup ranges every tail_rs_kernel row of the table reaches, and the precondition, the POWER and the boundary-set cap of every case
tests/test_gpu_tail_parity.py uses - a case that would prove nothing (a partial sum past 2^24 grid steps, a split that does not return the planted lo, a lost lo
plane that moves too few codes, a boundary set over 8 % of the codes) fails here, where no GPU is needed."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import s16_ends_ref as ends
import s16_ref
import tail_ref as tr
import torch_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None
_SHAPES = tr.shapes()


def test_case_table_is_the_issues():
    rs = [(w, h, cus) for k, w, h, cus in tr.CASES if k == tr.TAIL_RS]
    assert rs == [(1, 1, 0), (32, 32, 1), (100, 60, 0), (100, 60, 3), (130, 9, 7), (257, 130, 1), (257, 130, 7), (288, 32, 1), (288, 32, 7)]
    for k in (tr.TAIL_HEAD_S16, tr.TAIL_HEAD_F32, tr.TAIL_UNFUSED):
        assert [(w, h, cus) for kk, w, h, cus in tr.CASES if kk == k] == [(1, 1, 0), (100, 60, 0), (130, 9, 0), (257, 130, 0)]
    assert len(tr.CASES) == 9 + 3 * 4
    assert sorted(tr.DENSE_CASES) == sorted([(0, 100, 60, 0), (0, 257, 130, 0), (0, 257, 130, 7), (1, 100, 60, 0), (1, 257, 130, 0)])
    assert sorted(tr.FAR_CASES) == sorted([(0, 100, 60, 3), (0, 257, 130, 7), (1, 257, 130, 0)])
    wp, hp = tr.padded(257, 130)
    assert (wp // 4 + 31) // 32 * ((hp // 4 + 7) // 8) == 15 and 15 % 8 != 0      # head_h2_kernel's tiles: the XCD remap has a remainder
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    assert (amd.TAIL_RS, amd.TAIL_HEAD_S16, amd.TAIL_HEAD_F32, amd.TAIL_UNFUSED, amd.TAIL_GUARD) == (0, 1, 2, 3, tr.GUARD)
    assert (amd.PIX_RGB8, amd.PIX_RGB10_U16, amd.PIX_A2B10G10R10, amd.PIX_RGBA8) == tr.FORMATS
    hdr = open(os.path.join(ROOT, "include", "rife_hip_test.h")).read()
    assert re.search(r"RIFE_HIP_TAIL_RS = 0, RIFE_HIP_TAIL_HEAD_S16 = 1, RIFE_HIP_TAIL_HEAD_F32 = 2, RIFE_HIP_TAIL_UNFUSED = 3", hdr)
    assert re.search(r"RIFE_HIP_TAIL_GUARD = %d\b" % tr.GUARD, hdr) and "rife_hip_op_tail" in amd.TEST_ABI_SYMBOLS


def test_rows_reach_the_ranges_the_issue_names():
    """u0 = nunits wg / nwg restated: what every tail_rs_kernel row reaches, for 256 and for 304 compute units."""
    fig = tr.check_ranges()
    for chip in tr.CHIP_CUS:
        assert fig[(1, 1, 0, chip)]["smax"] == 1 and fig[(100, 60, 0, chip)]["smax"] == 1                      # S = 1 everywhere: the block after the loop alone
        assert fig[(257, 130, 1, chip)] == dict(nunits=120, nwg=2, smin=60, smax=60, strip_changes=2, mid_starts=1, last_strip_cols=8)
        assert fig[(257, 130, 7, chip)]["mid_starts"] == 13 and fig[(257, 130, 7, chip)]["strip_changes"] > 0 and fig[(257, 130, 7, chip)]["smin"] == 8
        assert fig[(288, 32, 7, chip)]["strip_changes"] == 1 and fig[(288, 32, 7, chip)]["smax"] == 2
    # the product's own regime (run_block_convs: strips x Hq >= 32 CUs): every workgroup walks 16 steps and more, across strips - (257, 130) at cus = 1 is in it
    r = tr.tail_rs_ranges(257, 130, 1, 256)
    assert r["nunits"] >= 32 * 1 and r["smin"] >= 16
    for row in tr.TAIL_RS_ROWS:
        print("tail_ref ranges", row, {k: v for k, v in fig[row + (256,)].items()}, "| 304 CUs:", fig[row + (304,)]["nwg"], "workgroups")


def test_reference_matches_a_scalar_loop():
    """tail() against the definition written out per pixel, on the planted 32 x 32 case at depth 8 (all four channels)."""
    w = h = 32
    c = tr.cached("planted", w, h, 8)
    d, F, M, top = c["d"], c["F"].astype(np.float64), c["M"].astype(np.float64), 255.0
    img = [c["p0"] / top, c["p1"] / top]
    got = np.zeros((h, w, 4), np.int64)
    for y in range(h):
        for x in range(w):
            m = 1.0 / (1.0 + math.exp(-(M[y, x] + d[4, y, x])))
            v = np.zeros(4)
            for k, wt in ((0, m), (1, 1.0 - m)):
                sx, sy = x + F[y, x, 2 * k] + d[2 * k, y, x], y + F[y, x, 2 * k + 1] + d[2 * k + 1, y, x]
                x0, y0 = min(max(math.floor(sx), 0), w - 1), min(max(math.floor(sy), 0), h - 1)
                x1, y1 = min(max(math.floor(sx) + 1, 0), w - 1), min(max(math.floor(sy) + 1, 0), h - 1)
                a, b = sx - x0, sy - y0
                v += wt * ((img[k][:, y0, x0] * (1 - a) + img[k][:, y0, x1] * a) * (1 - b) + (img[k][:, y1, x0] * (1 - a) + img[k][:, y1, x1] * a) * b)
            got[y, x] = np.clip(np.floor(v * top + 0.5), 0, top)
    # two float64 evaluations in different orders: they may part only where the value sits on a boundary to 1e-9
    differ = got != c["ref"]["code"]
    assert not (differ & (np.abs(c["ref"]["val"] - np.rint(c["ref"]["val"])) > 1e-9)).any() and differ.mean() < 0.01
    assert np.array_equal(tr.reference(c["x"], c["wgt"], c["b"], c["F"], c["M"], c["p0"], c["p1"], w, h, 8)["code"], c["ref"]["code"])


@pytest.mark.parametrize("amp", [0.0, 0.75, 3.0, 40.0, 700.0])
def test_warp_matches_the_graph_executors(amp):
    """tail_ref.warp against tests/torch_graph.py's restatement of the reference's Warp::forward, in float64 on flows of the grid (both are exact there to the last
    rounding), in frame and far out of it; alpha and beta are the clamped first tap's."""
    rng = np.random.default_rng(int(amp * 4))
    H, W = 32, 64
    img = rng.integers(0, 256, (3, H, W)) / 255.0
    flow = rng.integers(-1024, 1025, (2, H, W)) * 2.0 ** -10 * amp
    got, alpha, beta, outside = tr.warp(img, flow[0], flow[1])
    want = torch_graph.warp(torch.from_numpy(img), torch.from_numpy(flow)).numpy()
    assert want.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * max(1.0, amp)
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.array_equal(alpha, xs + flow[0] - np.clip(np.floor(xs + flow[0]), 0, W - 1)) and np.array_equal(beta, ys + flow[1] - np.clip(np.floor(ys + flow[1]), 0, H - 1))
    if amp >= 40:
        assert outside.mean() > 0.25 and np.abs(alpha).max() > amp / 2
        # a clamped tap pair returns the edge pixel itself, whatever alpha is
        far_left = xs + flow[0] < -1
        assert np.abs(got - (img[:, np.clip(np.floor(ys + flow[1]).astype(int), 0, H - 1), 0] * (1 - beta) +
                             img[:, np.clip(np.floor(ys + flow[1]).astype(int) + 1, 0, H - 1), 0] * beta))[:, far_left].max() < 1e-9
    if amp == 0:
        assert np.array_equal(got, img) and not outside.any()


@pytest.mark.parametrize("pixfmt", tr.FORMATS)
def test_pack_and_unpack_are_the_formats_layouts(pixfmt):
    rng = np.random.default_rng(pixfmt)
    h, w, n, top = 3, 5, tr.channels_of(pixfmt), tr.top_of(tr.depth_of(pixfmt))
    code = rng.integers(0, top + 1, (h, w, 4))
    b = tr.pack_frame(code, pixfmt)
    assert b.dtype == np.uint8 and b.size == w * h * {0: 3, 1: 6, 2: 4, 4: 4}[pixfmt]
    back, ok = tr.unpack_frame(b, w, h, pixfmt)
    assert ok and np.array_equal(back, code[..., :n])
    px = code[1, 2]
    if pixfmt == tr.PIX_A2B10G10R10:
        assert int(b.view("<u4")[1 * w + 2]) == px[0] | px[1] << 10 | px[2] << 20 | 3 << 30
        bad = b.copy(); bad[3] &= 0x3f
        assert not tr.unpack_frame(bad, w, h, pixfmt)[1]
    elif pixfmt == tr.PIX_RGB10_U16:
        assert b.view("<u2")[(1 * w + 2) * 3:(1 * w + 2) * 3 + 3].tolist() == px[:3].tolist()
    else:
        assert b[(1 * w + 2) * n:(1 * w + 2) * n + n].tolist() == px[:n].tolist()
    # the resident frames: depth 8 R | G << 8 | B << 16 | A << 24, depth 10 R | G << 10 | B << 20
    d = tr.depth_of(pixfmt)
    p = tr.frame_planes(40, 33, d, 1)
    r = tr.pack_resident(p, d)
    assert r.dtype == np.uint32 and r.shape == (64, 64) and p.min() == 0 and p.max() == top
    y, x = 17, 43
    assert int(r[y, x]) == (p[0, y, x] | p[1, y, x] << 10 | p[2, y, x] << 20 if d == 10 else p[0, y, x] | p[1, y, x] << 8 | p[2, y, x] << 16 | p[3, y, x] << 24)
    assert tr.largest_step(p) in (top // 8, top // 8 + 1)                       # period 16, full amplitude
    assert not np.array_equal(p, tr.frame_planes(40, 33, d, 0))


def _assert_common(c, w, h, depth):
    wp, hp = tr.padded(w, h)
    n = 4 if depth == 8 else 3
    assert c["x"].shape == (64, hp // 4, wp // 4) and c["x"].dtype == np.float32 and c["wgt"].shape == (24, 64, 4, 4) and c["b"].shape == (24,)
    assert c["F"].shape == (hp, wp, 4) and c["F"].dtype == np.float32 and c["M"].shape == (hp, wp) and np.abs(c["M"]).max() < 1
    assert np.array_equal(c["wgt"].astype(np.float16).astype(np.float32), c["wgt"])
    assert np.array_equal(s16_ref.value(s16_ref.pack(c["x"], hp // 4, wp // 4), 64, hp // 4, wp // 4), c["x"].astype(np.float64))      # the S16 tensor holds exactly these values
    ref = c["ref"]
    assert ref["code"].shape == ref["val"].shape == (h, w, n) and ref["amax"].shape == c["tau"].shape == (h, w) and ref["amax"].min() >= 1
    assert np.array_equal(ref["code"], tr.reference(c["x"], c["wgt"], c["b"], c["F"], c["M"], c["p0"], c["p1"], w, h, depth)["code"])
    # the cap, restated from the arrays
    frac = (np.abs(ref["val"] - np.rint(ref["val"])) <= c["tau"][..., None]).mean()
    assert frac == c["boundary_frac"] < tr.CAP == 0.08
    lo, hi = tr.allowed_range(ref, c["tau"], depth)
    assert np.all(lo <= ref["code"]) and np.all(ref["code"] <= hi) and np.array_equal((lo != hi) | False, (lo != hi) & c["boundary"])
    assert np.array_equal(c["img0"], tr.pack_resident(c["p0"], depth)) and c["img0"].shape == (hp, wp)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("shape", _SHAPES["planted"], ids=_ids)
def test_planted_case_holds_its_precondition_and_has_power(shape, depth):
    """planted_case() asserts these itself; restated from the arrays it returns."""
    w, h = shape
    c = tr.cached("planted", w, h, depth)
    _assert_common(c, w, h, depth)
    hi, lo = s16_ref.split(c["x"])
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    assert np.array_equal(lo, c["lo"]) and np.array_equal(hi, c["hi"])                                          # the split returns the planted lo
    assert np.array_equal(hi[0::2], -hi[1::2]) and hi[0::2].min() > 16 and hi[0::2].max() < 32                   # pairs +h, -h inside one binade, never 16 itself
    k = lo * 2.0 ** 10
    assert np.array_equal(k, np.round(k)) and k.min() >= 1 and k.max() <= 7
    assert np.array_equal(c["wgt"][:, 0::2], c["wgt"][:, 1::2]) and set(np.unique(c["wgt"])) == {-2.0, -1.0, 1.0, 2.0} and 0.75 < (c["wgt"] > 0).mean() < 0.85
    for a in (c["b"], c["F"], c["M"]):
        s = a.astype(np.float64) * 2.0 ** 10
        assert np.array_equal(s, np.round(s))
    assert np.abs(c["F"]).max() < 3
    assert ends.head_abs_sum(*s16_ref.split(c["x"]), c["wgt"], c["b"]) * 2.0 ** 10 < 2.0 ** 24 and 0 < c["bound"] < 1
    assert not ends.head_ps(hi, c["wgt"], np.zeros(24)).any()                                                     # the hi planes alone give no delta at all
    d = ends.head_ps(c["x"], c["wgt"], c["b"])[:5]
    assert np.array_equal(d, c["d"]) and np.array_equal(d.astype(np.float32).astype(np.float64), d)
    # power, restated: every figure from a reference evaluation of its own
    run = lambda dd: tr.tail(dd, c["F"], c["M"], c["p0"], c["p1"], w, h, depth)["code"][..., :3]
    want = c["ref"]["code"][..., :3]
    d_b = np.broadcast_to(c["b"].astype(np.float64).reshape(6, 2, 2)[:, None, :, None, :], (6, d.shape[1] // 2, 2, d.shape[2] // 2, 2)).reshape(6, d.shape[1], d.shape[2])[:5]
    assert (np.abs(run(d_b) - want) >= 4).mean() == c["power_all"] > 0.75
    for q in range(4):
        x = c["x"].astype(np.float64).copy(); x[16 * q:16 * q + 16] = hi[16 * q:16 * q + 16]
        assert (np.abs(run(ends.head_ps(x, c["wgt"], c["b"])[:5]) - want) >= 2).mean() == c["power_chunk"][q] > 0.5
    for p in range(5):
        dd = d.copy(); dd[p] = d_b[p]
        assert (np.abs(run(dd) - want) >= 2).any(axis=-1).mean() == c["power_plane"][p] > 0.75
    print("tail_ref planted %dx%d depth %d: seed %d, bound %.3f of 2^24, lo part of a delta %.3f +- %.3f px, boundary set %.4f, all lo dropped moves %.3f (4 codes), "
          "a chunk %.3f .. %.3f (2 codes), a delta plane %s of the pixels (2 codes)" % (w, h, depth, c["seed"], c["bound"], c["lo_part"][0], c["lo_part"][1],
          c["boundary_frac"], c["power_all"], min(c["power_chunk"]), max(c["power_chunk"]), " ".join("%.3f" % v for v in c["power_plane"])))


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("shape", _SHAPES["dense"], ids=_ids)
def test_dense_case_is_what_the_kernel_reads(shape, depth):
    w, h = shape
    c = tr.cached("dense", w, h, depth)
    _assert_common(c, w, h, depth)
    d = ends.head_ps(c["x"], c["wgt"], c["b"])[:5]
    assert 1.0 < np.abs(d).max() == c["dmax"] < 4.0 and np.abs(c["F"]).max() < 3
    hi = s16_ref.split(c["x"])[0].astype(np.float64)
    assert np.abs(ends.head_ps(hi, c["wgt"], c["b"])[:5]).max() > 1.0                                              # the hi path carries the deltas here
    top = tr.top_of(depth)
    assert c["gslope"] == max(tr.largest_step(c["p0"]), tr.largest_step(c["p1"]), top / 4.0) == top / 4.0
    assert np.allclose(c["tau"], 2.0 ** -6 * c["ref"]["amax"] + c["gslope"] * (4e-6 * c["dmax"] + 1e-6), rtol=1e-15, atol=0)
    print("tail_ref dense %dx%d depth %d: seed %d, max|d| %.3f px, tau - 2^-6 amax = %.2e code, boundary set %.4f" % (
        w, h, depth, c["seed"], c["dmax"], c["gslope"] * (4e-6 * c["dmax"] + 1e-6), c["boundary_frac"]))


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("shape", _SHAPES["far"], ids=_ids)
def test_far_case_leaves_the_frame(shape, depth):
    w, h = shape
    c = tr.cached("far", w, h, depth)
    _assert_common(c, w, h, depth)
    wp, hp = tr.padded(w, h)
    s = c["F"].astype(np.float64) * 2.0 ** 10
    assert np.array_equal(s, np.round(s)) and np.abs(s).max() < 2.0 ** 24
    assert c["F"].min() < -wp / 2 and c["F"].max() > wp / 2 and np.abs(c["F"]).max() > 200                        # several hundred px, both signs
    assert min(c["outside"]) > 0.25 and np.array_equal([c["ref"]["outside"][k].mean() for k in range(2)], c["outside"])
    assert c["max_alpha"] == c["ref"]["amax"].max() > 100                                                         # alpha in the hundreds
    assert np.array_equal(c["tau"], 2.0 ** -6 * c["ref"]["amax"])
    print("tail_ref far %dx%d depth %d: seed %d, amplitude %d px, largest |alpha| %.1f, samples outside %.3f / %.3f, boundary set %.4f" % (
        w, h, depth, c["seed"], c["amplitude"], c["max_alpha"], c["outside"][0], c["outside"][1], c["boundary_frac"]))
