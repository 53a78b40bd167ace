"""Flow scale 2 (include/rife_hip.h rife_hip_set_flow_scale) on the GPU: every IFBlock of rife-v4.6 at half its resolution, frames padded to 64n.

Expected values: the oracle on the rewritten graph (tests/flowscale_ref.py; tests/test_flowscale_host.py pins that recipe without a GPU).
  1  parity: at most 1 code per channel against the oracle, RGB8 and both 10-bit formats
  2  stage flows flow0..3 within 1e-3 of the oracle's blobs
  3  the final kernel (k_final_scaled) on injected flows that leave the frame, and on scaled ones that stay inside it for most pixels, RGB8 / A2B10G10R10 / RGBA8 /
     RGB10_U16 (the gather code and the flow updates of the mode on injected flows: tests/test_gpu_flowscale_gather.py)
  4  identities, byte for byte: every entry point against process(), YUV against the A2B10G10R10 call, threads, repeat runs, timestep 0 / 1, scale 1
  5  refusals
  6  the command line (-d)"""
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import deep_ref
import flowscale_ref as fr
import yuv_ref as yr
from oracle import pyoracle
from tools import gen_frames

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIFE_HIP = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")
U16, PACKED, RGBA8, NV12 = amd.PIX_RGB10_U16, amd.PIX_A2B10G10R10, amd.PIX_RGBA8, amd.PIX_NV12


@pytest.fixture(scope="module")
def g2(modeldirs):
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    assert g.flow_scale == 1
    g.set_flow_scale(2)
    assert g.flow_scale == 2
    return g


@pytest.fixture(scope="module")
def g1(modeldirs):
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    return g


@pytest.fixture(scope="module")
def t2(modeldirs):
    """A scale-2 engine of the test build: the stage taps."""
    g = amd.test_build().RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    g.set_flow_scale(2)
    return g


@pytest.fixture(scope="module")
def oracle2(modeldirs, tmp_path_factory):
    o = pyoracle.OracleRIFE(rife_v4=True)
    o.load(fr.scaled_modeldir(modeldirs["rife-v4.6"], tmp_path_factory.mktemp("v46_fs2")))
    return o


def codes_off(got, want):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d > 0).mean())


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,t", [(640, 360, 0.5), (256, 192, 0.125), (100, 60, 0.7), (96, 64, 0.5), (33, 47, 0.9),
                                   (1, 1, 0.5), (31, 33, 0.5), (65, 64, 0.5), (8, 300, 0.5), (520, 16, 0.5)])
def test_rgb8_frame_within_one_code_of_the_rewritten_graph(g2, oracle2, w, h, t):
    a, b = gen_frames.smooth_pair(w, h, 7 + w)
    want = fr.expected_frame(oracle2, a, b, t, 8)
    got = g2.process(a, b, t)
    worst, share = codes_off(got, want)
    print("flow scale 2, %dx%d t=%g: max |diff| %d codes, %.3f %% of the channels differ" % (w, h, t, worst, 100 * share))
    assert got.shape == want.shape and worst <= 1


@pytest.mark.parametrize("w,h", [(256, 192), (33, 47)])
def test_ten_bit_frames_within_one_code_and_equal_in_both_formats(g2, oracle2, w, h):
    a, b = deep_ref.deep_pair(w, h, 31)
    want = fr.expected_frame(oracle2, a, b, 0.5, 10)
    got = g2.process(a, b, 0.5)
    assert got.dtype == np.uint16
    worst, share = codes_off(got, want)
    print("flow scale 2, RGB10_U16 %dx%d: max |diff| %d codes, %.3f %% differ" % (w, h, worst, 100 * share))
    assert worst <= 1
    packed = g2.process(amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b), 0.5)
    assert np.array_equal(amd.unpack_a2b10g10r10(packed), got)


# ---- 2. stage flows ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", [(64, 64), (160, 96)])
def test_stage_flows_match_the_rewritten_graph(t2, oracle2, w, h, depth):
    a, b = gen_frames.smooth_pair(w, h, 3) if depth == 8 else deep_ref.deep_pair(w, h, 33)
    wp, hp = fr.padded(w, h)
    for k, s in enumerate((16, 8, 4, 2)):
        want = fr.extract(oracle2, a, b, 0.5, depth, "flow%d" % k)
        got = t2.v4_extract_flow(a, b, 0.5, k)
        assert got.shape == want.shape == (6, hp // s, wp // s)
        err = float(np.abs(got - want).max())
        print("flow scale 2, depth %d, %dx%d flow%d: max |diff| %.3g" % (depth, w, h, k, err))
        assert err < 1e-3, k


# ---- 3. the final kernel on injected flows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,seed,scaled", [pytest.param(100, 60, 1, False, id="100-60-1"), pytest.param(333, 241, 4, False, id="333-241-4")] +
                         [pytest.param(w, h, seed, True, id="%d-%d-%d-scaled" % (w, h, seed)) for w, h, seed in fr.FINAL_CASES])
def test_final_kernel_on_injected_flows_that_leave_the_frame(t2, oracle2, w, h, seed, scaled):
    """scaled: flowscale_ref.injected_flows_scaled - between a quarter and nine tenths of the sampling positions of each frame lie INSIDE the padded frame
    (tests/test_flowscale_host.py holds that for these cases); the unscaled blobs copy the scale-1 amplitudes and at 100x60 leave the frame nearly everywhere."""
    if scaled:
        inj = fr.injected_flows_scaled(w, h, fr.FLOW_SEED + seed, 4)
        assert np.abs(inj[0][:4]).max() * 16 > min(fr.padded(w, h)) / 4, "injected flows too small to exercise the clamps"
    else:
        inj = fr.injected_flows(w, h, 100 + seed, 4)
        assert np.abs(inj[0][:4]).max() * 16 > 100, "injected flows too small to exercise the clamps"
    t = 0.4
    # PX 0
    a, b = gen_frames.noise_pair(w, h, seed) if seed % 2 else gen_frames.smooth_pair(w, h, seed)
    f_full = fr.extract(oracle2, a, b, t, 8, "out0", flows=inj)
    want = deep_ref.quantise(f_full, w, h, 8)
    got = t2.v4_process_injected(a, b, t, inj)
    worst, share = codes_off(got, want)
    print("k_final_scaled<0> %dx%d: max |diff| %d, %.3f %% differ" % (w, h, worst, 100 * share))
    assert worst <= 1
    # PX 4: the colour bytes are the RGB8 call's, alpha within one code of its own plane through the same flows
    rng = np.random.default_rng(seed)
    al = [rng.integers(0, 256, (h, w, 1), dtype=np.uint8) for _ in range(2)]
    rgba = t2.v4_process_injected(np.concatenate([a, al[0]], -1), np.concatenate([b, al[1]], -1), t, inj, pixfmt=RGBA8)
    assert rgba.shape == (h, w, 4) and np.array_equal(rgba[..., :3], got)
    # PX 2
    a10, b10 = deep_ref.deep_pair(w, h, 50 + seed)
    want10 = deep_ref.quantise(fr.extract(oracle2, a10, b10, t, 10, "out0", flows=inj), w, h, 10)
    got10 = amd.unpack_a2b10g10r10(t2.v4_process_injected(amd.pack_a2b10g10r10(a10), amd.pack_a2b10g10r10(b10), t, inj, pixfmt=PACKED))
    worst, share = codes_off(got10, want10)
    print("k_final_scaled<2> %dx%d: max |diff| %d, %.3f %% differ" % (w, h, worst, 100 * share))
    assert worst <= 1
    # PX 1: the RGB10_U16 frame is the unpacked A2B10G10R10 frame
    got16 = t2.v4_process_injected(a10, b10, t, inj, pixfmt=U16)
    assert got16.dtype == np.uint16 and got16.shape == (h, w, 3)
    assert np.array_equal(got16, got10), "k_final_scaled<1>: %d of %d codes differ from k_final_scaled<2>'s" % (int((got16 != got10).sum()), got10.size)


# ---- 4. identities -----------------------------------------------------------------------------------------------------------------------------------

def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


@pytest.mark.parametrize("w,h", [(100, 60), (640, 360)])
def test_every_entry_point_gives_the_bytes_of_process(g2, w, h):
    import torch
    prs = [gen_frames.smooth_pair(w, h, 20 + i) for i in range(3)]
    ts = [0.5, 0.25, 0.7]
    want = [g2.process(p[0], p[1], t) for p, t in zip(prs, ts)]
    for p, t, wnt in zip(prs, ts, want):
        f0, f1 = g2.upload(p[0]), g2.upload(p[1])
        assert np.array_equal(g2.process_frames(f0, f1, t), wnt)
        f0.release(); f1.release()
    d0 = [_dev(p[0]) for p in prs]; d1 = [_dev(p[1]) for p in prs]
    part = g2.stream_create(1, 4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, st.cuda_stream, part):
        outs = [torch.zeros_like(x) for x in d0]
        for i in range(3):
            g2.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], outs[i].data_ptr(), stream)
        torch.cuda.synchronize()
        for i in range(3):
            assert np.array_equal(outs[i].cpu().numpy().reshape(h, w, 3), want[i]), (i, stream)
    g2.stream_destroy(part)
    for k in range(1, 4):
        outs = [torch.zeros_like(x) for x in d0[:k]]
        g2.process_device_batch([x.data_ptr() for x in d0[:k]], [x.data_ptr() for x in d1[:k]], w, h, ts[:k], [o.data_ptr() for o in outs], st.cuda_stream)
        st.synchronize()
        for i in range(k):
            assert np.array_equal(outs[i].cpu().numpy().reshape(h, w, 3), want[i]), (k, i)
    # the host batch
    for o, wnt in zip(g2.process_batch([p[0] for p in prs], [p[1] for p in prs], ts), want):
        assert np.array_equal(o, wnt)
    # row-padded planes: an image call
    pad = [np.full((h, w + 5, 3), 0x5a, np.uint8) for _ in range(3)]
    pad[0][:, :w] = prs[0][0]; pad[1][:, :w] = prs[0][1]
    g2.process(pad[0][:, :w], pad[1][:, :w], ts[0], outimage=pad[2][:, :w])
    assert np.array_equal(pad[2][:, :w], want[0]) and (pad[2][:, w:] == 0x5a).all()


def test_nv12_call_is_the_packed_call_on_the_converted_frames(g2):
    w, h = 130, 98
    y0, y1 = (yr.rgb10_to_yuv(c, NV12) for c in deep_ref.deep_pair(w, h, 61))
    got = g2.process_yuv(y0, y1, w, h, 0.5, NV12)
    r0, r1 = (amd.pack_a2b10g10r10(yr.yuv_to_rgb10(y, w, h, NV12)) for y in (y0, y1))
    want = yr.rgb10_to_yuv(amd.unpack_a2b10g10r10(g2.process(r0, r1, 0.5)), NV12)
    assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1))


def test_reentrant_repeatable_and_timestep_0_1(g2):
    w, h = 256, 192
    a, b = gen_frames.smooth_pair(w, h, 9)
    first = g2.process(a, b, 0.5)
    assert np.array_equal(g2.process(a, b, 0.5), first)
    outs = [None] * 4
    def work(i):
        outs[i] = g2.process(a, b, 0.5)
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for x in th: x.start()
    for x in th: x.join()
    assert all(np.array_equal(o, first) for o in outs)
    assert np.array_equal(g2.process(a, b, 0.0), a) and np.array_equal(g2.process(a, b, 1.0), b)


def test_scale_1_is_the_default_engine_and_scale_2_is_not(g1, g2, modeldirs):
    w, h = 256, 192
    a, b = gen_frames.smooth_pair(w, h, 9)
    base = g1.process(a, b, 0.5)
    g = amd.RIFE(0, rife_v4=True); g.load(modeldirs["rife-v4.6"])
    g.set_flow_scale(1)
    assert g.flow_scale == 1 and np.array_equal(g.process(a, b, 0.5), base)
    assert not np.array_equal(g2.process(a, b, 0.5), base)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------

def _set(g, n):
    rc = g._L.rife_hip_set_flow_scale(g._h, n)
    return rc, g._L.rife_hip_last_error().decode()


def test_bad_arguments_are_einval(modeldirs):
    g = amd.RIFE(0, rife_v4=True)
    assert _set(g, 2)[0] == -1 and _set(g, 1)[0] == -1          # before load: the family is not known
    g.load(modeldirs["rife-v4.6"])
    for n in (0, -1, 3):
        rc, msg = _set(g, n)
        assert rc == -1 and msg
    with pytest.raises(amd.RifeError):
        g.set_flow_scale(3)
    assert g.flow_scale == 1
    a, b = gen_frames.smooth_pair(64, 48, 2)
    assert g.process(a, b, 0.5).shape == a.shape


@pytest.mark.parametrize("fam,kw,word", [("rife-v4", dict(rife_v4=True), "rife-v4 (4.0)"), ("rife-v2.3", dict(rife_v2=True), "rife-v2"),
                                         ("rife-v3.1", dict(rife_v2=True), "rife-v3"), ("rife", dict(), "rife (v1"),
                                         ("rife-v4.6", dict(rife_v4=True, tta_mode=True), "-x"), ("rife-v4.6", dict(rife_v4=True, tta_temporal_mode=True), "-z")])
def test_other_families_and_modes_are_enosys(modeldirs, fam, kw, word):
    g = amd.RIFE(0, **kw); g.load(modeldirs[fam])
    rc, msg = _set(g, 2)
    assert rc == -amd.ENOSYS and word in msg, msg
    assert g.flow_scale == 1 and _set(g, 1)[0] == 0
    a, b = gen_frames.smooth_pair(64, 64, 2)
    assert g.process(a, b, 0.5).shape == a.shape


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------------------

def test_cli_d2_writes_the_scale_2_frame_and_refusals_write_nothing(g2, modeldirs, tmp_path):
    from PIL import Image
    assert os.path.exists(RIFE_HIP), "rife-hip is not built"
    a, b = gen_frames.smooth_pair(100, 60, 4)
    Image.fromarray(a).save(tmp_path / "a.png"); Image.fromarray(b).save(tmp_path / "b.png")
    base = [RIFE_HIP, "-0", str(tmp_path / "a.png"), "-1", str(tmp_path / "b.png")]
    r = subprocess.run(base + ["-o", str(tmp_path / "o.png"), "-m", modeldirs["rife-v4.6"], "-d", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o.png").convert("RGB")), g2.process(a, b, 0.5))
    for name, extra in (("v23.png", ["-m", modeldirs["rife-v2.3"], "-d", "2"]), ("d3.png", ["-m", modeldirs["rife-v4.6"], "-d", "3"]),
                        ("v40.png", ["-m", modeldirs["rife-v4"], "-d", "2"])):
        r = subprocess.run(base + ["-o", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stderr.strip() and not os.path.exists(tmp_path / name), (name, r.returncode, r.stderr)
