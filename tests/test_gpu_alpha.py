"""RGBA frames (RIFE_HIP_PIX_RGBA8, include/rife_hip.h) through the rife-v4.6 engine, on the GPU.

What the header states, checked in its words: the colour bytes of an RGBA call are those of the RGB8 call (exact); alpha goes through the tail of the graph in
the colour channels' arithmetic (alpha := a colour plane gives that plane back, exact, where no padding exists); alpha is edge-padded (opaque stays opaque);
against the recipe of tests/alpha_ref.py at most 1 code, the project's contract.  The share of off-by-one alpha samples is printed next to the colour
channels' share of the same call and, at 1080p and 4K, bounded by twice that share: the alpha plane takes the colour planes' path, the factor 2 is for the
different content."""
import importlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import alpha_ref
import deep_ref
from oracle import pyoracle
from test_gpu_gather import injected_flows
from tools import gen_frames

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
amd_t = amd.test_build()
RGBA = amd.PIX_RGBA8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engines(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    return g, o


def _switched(d, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        g = amd_t.RIFE(0, rife_v4=True); g.load(d)
    finally:
        for k, v in old.items():
            if v is None: del os.environ[k]
            else: os.environ[k] = v
    return g


def rgb_of(x):
    return np.ascontiguousarray(x[..., :3])


def with_alpha(rgb, alpha):
    return np.ascontiguousarray(np.dstack([rgb, alpha]))


# ---- 1. colour identity, exact ---------------------------------------------------------------------------------------------------------------

SIZES_ID = [(1, 1), (2, 3), (31, 33), (33, 47), (100, 60), (130, 9), (8, 300), (333, 241), (640, 360), (1000, 520), (1920, 1080), (3840, 2160)]


@pytest.mark.parametrize("w,h", SIZES_ID)
def test_colour_of_an_rgba_call_is_the_rgb8_call(engines, w, h):
    g, _ = engines
    a, b = alpha_ref.rgba_pair(w, h, 300 + w, "random")
    for t in (0.5, 0.3):
        got = g.process(a, b, t)
        assert got.dtype == np.uint8 and got.shape == (h, w, 4)
        want = g.process(rgb_of(a), rgb_of(b), t)
        assert np.array_equal(got[..., :3], want), "%d colour bytes differ" % int((got[..., :3] != want).sum())


@pytest.mark.parametrize("w,h", [(33, 47), (100, 60), (640, 360), (1000, 520)])
def test_colour_identity_on_the_tile_paths(modeldirs, w, h):
    """The same with the tile kernels selected: head_h2_kernel<EPI_FINAL, true, 4> behind the tile stems, and <EPI_FINAL, false, 4> on the tile trunk path."""
    d = modeldirs["rife-v4.6"]
    a, b = alpha_ref.rgba_pair(w, h, 17, "random")
    for env in (dict(RIFE_HIP_TAIL_RS="0", RIFE_HIP_STEM_RS="0"), dict(RIFE_HIP_TAIL_RS="0", RIFE_HIP_STEM_RS="0", RIFE_HIP_T64="0")):
        g = _switched(d, **env)
        got = g.process(a, b, 0.5)
        assert np.array_equal(got[..., :3], g.process(rgb_of(a), rgb_of(b), 0.5)), env


CHILD = (
    "import sys, importlib, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import alpha_ref\n"
    "amd = importlib.import_module('rife-ncnn-vulkan_amd')\n"
    "g = amd.RIFE(0, rife_v4=True); g.load(%r)\n"
    "for (w, h) in ((100, 60), (256, 192), (64, 64)):\n"
    "    a, b = alpha_ref.rgba_pair(w, h, 50, 'smooth')\n"
    "    x = g.process(a, b, 0.4)\n"
    "    assert np.array_equal(x[..., :3], g.process(np.ascontiguousarray(a[..., :3]), np.ascontiguousarray(b[..., :3]), 0.4)), 'colour identity'\n"
    "    for ch in range(3):\n"
    "        y = g.process(np.ascontiguousarray(np.dstack([a[..., :3], a[..., ch]])), np.ascontiguousarray(np.dstack([b[..., :3], b[..., ch]])), 0.4)\n"
    "        if w %% 32 == 0 and h %% 32 == 0: assert np.array_equal(y[..., 3], y[..., ch]), 'alpha == channel %%d' %% ch\n"
    "    np.save(%r %% (w, h), x)\n")


def test_unfused_fallbacks(modeldirs, engines, tmp_path):
    """RIFE_HIP_TRUNK=f32 (a product switch, read once per process): the pass runs the unfused fall-backs and k_final_px<4>, in a child process.  Colour identity
    and alpha == channel hold there exactly (asserted in the child); its frames against the recipe: at most 1 code."""
    _, o = engines
    d = modeldirs["rife-v4.6"]
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), d, str(tmp_path / "f32_%dx%d.npy"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, RIFE_HIP_TRUNK="f32"), timeout=600)
    assert p.returncode == 0, p.stderr[-1200:]
    for (w, h) in ((100, 60), (256, 192)):
        a, b = alpha_ref.rgba_pair(w, h, 50, "smooth")
        got = np.load(str(tmp_path / ("f32_%dx%d.npy" % (w, h))))
        mx, p1 = alpha_ref.report(got, alpha_ref.expected_rgba(o, a, b, 0.4))
        assert mx <= 1, (w, h, mx, p1)


# ---- 2. alpha equals a colour channel, exact ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,src", [(64, 64, (64, 64)), (640, 352, (640, 352)), (1920, 1088, (1920, 1080)), (3840, 2176, (3840, 2160))])
def test_alpha_equal_to_a_colour_plane_comes_back_as_that_plane(engines, w, h, src):
    """32n sizes (the 1080p and 4K test frames padded by replicating their last rows): no padding, so alpha := R gives output alpha == output R in every pixel;
    likewise G and B.  Pins the alpha arithmetic to the colour arithmetic with no tolerance."""
    g, _ = engines
    a, b = alpha_ref.rgb_pair(src[0], src[1], 400 + w)
    a = np.pad(a, ((0, h - src[1]), (0, w - src[0]), (0, 0)), mode="edge"); b = np.pad(b, ((0, h - src[1]), (0, w - src[0]), (0, 0)), mode="edge")
    for ch in range(3):
        got = g.process(with_alpha(a, a[..., ch]), with_alpha(b, b[..., ch]), 0.5)
        assert np.array_equal(got[..., 3], got[..., ch]), "channel %d: %d alpha samples differ" % (ch, int((got[..., 3] != got[..., ch]).sum()))


@pytest.mark.parametrize("w,h", [(64, 64), (640, 352)])
def test_alpha_equal_to_a_colour_plane_on_the_tile_paths(modeldirs, w, h):
    d = modeldirs["rife-v4.6"]
    a, b = alpha_ref.rgb_pair(w, h, 23)
    for env in (dict(RIFE_HIP_TAIL_RS="0", RIFE_HIP_STEM_RS="0"), dict(RIFE_HIP_TAIL_RS="0", RIFE_HIP_STEM_RS="0", RIFE_HIP_T64="0")):
        g = _switched(d, **env)
        for ch in range(3):
            got = g.process(with_alpha(a, a[..., ch]), with_alpha(b, b[..., ch]), 0.35)
            assert np.array_equal(got[..., 3], got[..., ch]), (env, ch)


# ---- 3. opaque stays opaque, clear stays clear ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(100, 60), (33, 47), (1, 1), (333, 241), (1920, 1080)])
def test_opaque_stays_opaque_and_clear_stays_clear(engines, w, h):
    g, _ = engines
    for code in (255, 0):
        a, b = alpha_ref.rgba_pair(w, h, 500 + w, code)
        for t in (0.5, 0.2):
            got = g.process(a, b, t)
            assert np.all(got[..., 3] == code), "alpha %d in: %d pixels came back different, extremes %d..%d" % (
                code, int((got[..., 3] != code).sum()), int(got[..., 3].min()), int(got[..., 3].max()))


# ---- 4. against the recipe: at most 1 code -------------------------------------------------------------------------------------------------------

PARITY = [(640, 360, 0.5, 1000), (256, 192, 0.125, 1001), (100, 60, 0.7, 1002), (33, 47, 0.9, 1003), (1, 1, 0.5, 77), (31, 33, 0.5, 77), (8, 300, 0.5, 77), (520, 16, 0.5, 77),
          (33, 32, 0.5, 77), (1920, 1080, 0.5, 2000), (3840, 2160, 0.5, 3000)]


@pytest.mark.parametrize("w,h,t,seed", PARITY)
@pytest.mark.parametrize("kind", ["smooth", "hard"])
def test_alpha_within_1_code_of_the_recipe(engines, w, h, t, seed, kind):
    """Alpha (smooth mattes, and hard 0 / 255 mattes that move with the scene) against the recipe: at most 1 code.  The off-by-one share of the alpha samples is
    printed for every size and, at 1080p and 4K, bounded by twice the colour channels' share of the same call (floor 1e-5 as in tests/test_gpu_deep.py)."""
    g, o = engines
    a, b = alpha_ref.rgba_pair(w, h, seed, kind)
    got = g.process(a, b, t)
    want = alpha_ref.expected_rgba(o, a, b, t)
    mxc, pc = alpha_ref.report(got[..., :3], want[..., :3])
    mxa, pa = alpha_ref.report(got[..., 3], want[..., 3])
    print("alpha parity %dx%d t=%g %s: alpha max %d, off-by-one %.3e; colour max %d, off-by-one %.3e; ratio %.2f"
          % (w, h, t, kind, mxa, pa, mxc, pc, pa / max(pc, 1e-5)))
    out = os.environ.get("RIFE_HIP_ALPHA_REPORT")
    if out:
        with open(out, "a") as f:
            f.write("%dx%d t=%g %s: alpha max %d share %.3e | colour max %d share %.3e | ratio %.2f\n" % (w, h, t, kind, mxa, pa, mxc, pc, pa / max(pc, 1e-5)))
    assert mxa <= 1 and mxc <= 1, (mxa, mxc)
    if w * h >= 1920 * 1080:      # a share of 1e-4 is a handful of samples below a million of them: bounded where it is a statistic (as tests/test_gpu_deep.py does)
        assert pa <= 2 * max(pc, 1e-5), (pa, pc)


# ---- 5. before quantisation ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,seed", [(100, 60, 1), (256, 192, 2), (640, 360, 3), (333, 241, 4)])
def test_float_tap_of_the_unfused_tail_on_injected_flows(modeldirs, w, h, seed):
    """Flows that leave the frame by hundreds of pixels: the alpha plane of the tap within 2e-6 of the recipe (expf is the only operation that may differ by an
    ulp), the colour planes too, and the colour planes equal the RGB8 tap's bit for bit."""
    d = modeldirs["rife-v4.6"]
    g = amd_t.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.load(d)
    a, b = alpha_ref.rgba_pair(w, h, 40 + seed, "smooth" if seed % 2 else "random")
    inj = injected_flows(w, h, 200 + seed, 4)
    got = g.v4_tap(a, b, 0.45, 2, 0, inj)
    assert got.shape[0] == 4
    want_c = deep_ref.extract(o, rgb_of(a), rgb_of(b), 0.45, 8, "out0", flows=inj)
    want_a = alpha_ref.alpha_out0(o, a[..., 3], b[..., 3], 0.45, inj)[0]
    da, dc = float(np.abs(got[3] - want_a).max()), float(np.abs(got[:3] - want_c).max())
    print("float tap %dx%d: alpha max %g, colour max %g" % (w, h, da, dc))
    assert da < 2e-6 and dc < 2e-6, (da, dc)
    assert np.array_equal(got[:3], g.v4_tap(rgb_of(a), rgb_of(b), 0.45, 2, 0, inj))


# ---- 6. paths agree, exact -------------------------------------------------------------------------------------------------------------------------

def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


@pytest.mark.parametrize("w,h,n", [(1920, 1080, 5), (640, 360, 4), (100, 60, 3)])
def test_host_device_resident_batch_and_partition_streams_agree(engines, w, h, n):
    import torch
    g, _ = engines
    prs = [alpha_ref.rgba_pair(w, h, 40 + i, "smooth" if i & 1 else "random") for i in range(n)]
    ts = [0.5, 0.25, 1.0, 0.7, 0.125][:n]
    want = [g.process(p[0], p[1], t) for p, t in zip(prs, ts)]
    for p, t, wnt in zip(prs, ts, want):
        f0, f1 = g.upload(p[0]), g.upload(p[1])
        assert f0.pixfmt == RGBA
        assert np.array_equal(g.process_frames(f0, f1, t), wnt)
        f0.release(); f1.release()
    d0 = [_dev(p[0]) for p in prs]; d1 = [_dev(p[1]) for p in prs]
    part = g.stream_create(1, 4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, st.cuda_stream, part):
        outs = [torch.zeros_like(x) for x in d0]
        torch.cuda.synchronize()                                         # the zero fill runs on torch's stream, the engine's work on others
        for i in range(n):
            g.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], outs[i].data_ptr(), stream, pixfmt=RGBA)
        torch.cuda.synchronize()
        for i in range(n):
            assert np.array_equal(_host(outs[i], want[i]), want[i]), (i, stream)
    g.stream_destroy(part)
    for k in range(1, n + 1):
        outs = [torch.zeros_like(x) for x in d0[:k]]
        torch.cuda.synchronize()
        g.process_device_batch([x.data_ptr() for x in d0[:k]], [x.data_ptr() for x in d1[:k]], w, h, ts[:k], [o.data_ptr() for o in outs], st.cuda_stream, pixfmt=RGBA)
        st.synchronize()
        for i in range(k):
            assert np.array_equal(_host(outs[i], want[i]), want[i]), (k, i)
    outs = [torch.zeros_like(x) for x in d0]
    torch.cuda.synchronize()
    g.process_device_batch([x.data_ptr() for x in d0], [x.data_ptr() for x in d1], w, h, ts, [o.data_ptr() for o in outs], None, pixfmt=RGBA)
    for i in range(n):
        assert np.array_equal(_host(outs[i], want[i]), want[i]), i


@pytest.mark.parametrize("w,h", [(128, 72), (100, 60)])
def test_device_frames_at_less_aligned_addresses_equal_aligned_ones(engines, w, h):
    """The one-pixel-per-lane pre-processing kernel (byte loads: any address; also every width that is not a multiple of 4) against the four-pixel form."""
    import torch
    g, _ = engines
    a, b = alpha_ref.rgba_pair(w, h, 4242, "random")
    want = g.process(a, b, 0.5)
    n = a.nbytes
    for off in (0, 1, 2, 3, 4, 8, 12, 16):
        b0 = torch.zeros(n + 32, dtype=torch.uint8, device="cuda"); b1 = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        b0[off:off + n] = _dev(a); b1[off:off + n] = _dev(b)
        out = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.process_device(b0.data_ptr() + off, b1.data_ptr() + off, w, h, 0.5, out.data_ptr() + off, None, pixfmt=RGBA)
        torch.cuda.synchronize()
        assert np.array_equal(_host(out[off:off + n], want), want), off
        assert not out[:off].any() and not out[off + n:].any(), "bytes outside the frame were written"


def test_timestep_endpoints_return_the_inputs(engines):
    import torch
    g, _ = engines
    a, b = alpha_ref.rgba_pair(64, 48, 3, "random")
    assert np.array_equal(g.process(a, b, 0.0), a) and np.array_equal(g.process(a, b, 1.0), b)
    f0, f1 = g.upload(a), g.upload(b)
    assert np.array_equal(g.process_frames(f0, f1, 0.0), a) and np.array_equal(g.process_frames(f0, f1, 1.0), b)
    d0, d1 = _dev(a), _dev(b); out = torch.zeros_like(d0)
    torch.cuda.synchronize()
    g.process_device(d0.data_ptr(), d1.data_ptr(), 64, 48, 1.0, out.data_ptr(), None, pixfmt=RGBA)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out, a), b)
    g.process_device_batch([d0.data_ptr()], [d1.data_ptr()], 64, 48, [0.0], [out.data_ptr()], None, pixfmt=RGBA)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out, a), a)


@pytest.mark.parametrize("w,h", [(256, 192), (1000, 520)])
def test_a_workspace_serves_rgb8_rgba8_and_rgb10_in_turn(modeldirs, w, h):
    import torch
    d = modeldirs["rife-v4.6"]
    a, b = alpha_ref.rgba_pair(w, h, 12, "smooth")
    a10, b10 = deep_ref.deep_pair(w, h, 12)
    fresh = amd.RIFE(0, rife_v4=True); fresh.load(d)
    cases = {"rgba": (a, b, RGBA), "rgb": (rgb_of(a), rgb_of(b), amd.PIX_RGB8), "deep": (a10, b10, amd.PIX_RGB10_U16)}
    want = {k: fresh.process(v[0], v[1], 0.5) for k, v in cases.items()}
    dev = {k: (_dev(v[0]), _dev(v[1])) for k, v in cases.items()}
    for order in (("rgb", "rgba", "deep", "rgba", "rgb"), ("rgba", "deep", "rgb", "rgba"), ("deep", "rgba", "rgb")):
        g = amd.RIFE(0, rife_v4=True); g.load(d)
        for k in order:
            out = torch.zeros_like(dev[k][0]); torch.cuda.synchronize()
            g.process_device(dev[k][0].data_ptr(), dev[k][1].data_ptr(), w, h, 0.5, out.data_ptr(), None, pixfmt=cases[k][2])
            torch.cuda.synchronize()
            assert np.array_equal(_host(out, want[k]), want[k]), (order, k)
        for k in order:                                                  # the pooled workspaces of the host path as well
            assert np.array_equal(g.process(cases[k][0], cases[k][1], 0.5), want[k]), (order, k)


def test_reentrant_and_4k_run_to_run_identical(engines):
    g, _ = engines
    a, b = alpha_ref.rgba_pair(3840, 2160, 705, "smooth")
    ref = g.process(a, b, 0.5)
    outs = [None] * 4

    def work(i):
        outs[i] = g.process(a, b, 0.5)
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in th]; [t.join() for t in th]
    for o in outs:
        assert np.array_equal(o, ref)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife-v3.1", {}, "rife-v3"), ("rife", {}, "v1"), ("rife-HD", {}, "v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal"),
                                         ("rife-v4.6", dict(uhd_mode=True), "UHD")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    g = amd.RIFE(0, **fl); g.load(modeldirs[fam])
    x, y = alpha_ref.rgba_pair(64, 64, 1, "random")
    out = np.full_like(x, 0x5a)
    keep = out.copy()
    for t in (0.5, 0.0):
        with pytest.raises(amd.RifeError) as e:
            g.process(x, y, t, outimage=out)
        assert "(-6)" in str(e.value) and word in str(e.value) and "RGBA" in str(e.value), str(e.value)
        assert np.array_equal(out, keep), "the output buffer was written"
    with pytest.raises(amd.RifeError) as e:
        g.upload(x)
    assert "(-6)" in str(e.value)
    d0, d1 = _dev(x), _dev(y); do = _dev(out)
    torch.cuda.synchronize()
    with pytest.raises(amd.RifeError) as e:
        g.process_device(d0.data_ptr(), d1.data_ptr(), 64, 64, 0.5, do.data_ptr(), None, pixfmt=RGBA)
    assert "(-6)" in str(e.value)
    with pytest.raises(amd.RifeError) as e:
        g.process_device_batch([d0.data_ptr()] * 2, [d1.data_ptr()] * 2, 64, 64, [0.5, 0.3], [do.data_ptr()] * 2, None, pixfmt=RGBA)
    assert "(-6)" in str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(_host(do, out), keep)
    # the RGB8 path of the same engine still works
    a8, b8 = gen_frames.smooth_pair(64, 64, 2)
    r = g.process(a8, b8, 0.5)
    assert r.shape == (64, 64, 3) and r.dtype == np.uint8 and r.any()
