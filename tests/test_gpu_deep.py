"""Deep colour: 10-bit RGB frames (RGB10_U16 / A2B10G10R10, include/rife_hip.h) through the rife-v4.6 engine, on the GPU.

Expected frames come from the oracle's network on planes code * (1 / 1023.f) (tests/deep_ref.py).  The contract is the project's, carried to depth 10: at most
1 code per channel.  The share of off-by-one channels is bounded relative to the 8-bit path on the same scene: p10 <= 8 * max(p8, 1e-5) (a fixed arithmetic
error crosses a rounding boundary 1023 / 255 = 4.01 times as often at depth 10; 2x on top for the different frames)."""
import importlib
import os
import threading

import numpy as np
import pytest

import deep_ref
from oracle import pyoracle
from test_gpu_gather import injected_flows
from tools import gen_frames

pytestmark = pytest.mark.gpu
amd = importlib.import_module("rife-ncnn-vulkan_amd")
amd_t = amd.test_build()
U16, PACKED = amd.PIX_RGB10_U16, amd.PIX_A2B10G10R10


@pytest.fixture(scope="module")
def engines(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    return g, o


@pytest.fixture(scope="module")
def tap_engines(modeldirs):
    d = modeldirs["rife-v4.6"]
    g = amd_t.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.load(d)
    names = []
    for line in open(os.path.join(d, "flownet.param")):
        f = line.split()
        if len(f) > 6 and f[0] == "Concat" and f[2] == "2" and f[3] == "1":
            names.append(f[6])
    assert len(names) == 3
    return g, o, names


def both_formats(g, a, b, t):
    """The pass in both 10-bit formats; they must give the same codes.  Returns (h, w, 3) uint16."""
    u = g.process(a, b, t)
    p = g.process(amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b), t)
    assert u.dtype == np.uint16 and p.dtype == np.uint32
    assert np.all(p >> 30 == 3), "alpha bits must be written as 3"
    assert np.array_equal(amd.unpack_a2b10g10r10(p), u), "RGB10_U16 and A2B10G10R10 disagree"
    return u


# ---- 1. frame parity: at most 1 code per channel against the recipe ----------------------------------------------------------------

@pytest.mark.parametrize("w,h,t,seed", [(640, 360, 0.5, 1000), (256, 192, 0.125, 1001), (100, 60, 0.7, 1002), (33, 47, 0.9, 1003)])
def test_process_within_1_code(engines, w, h, t, seed):
    g, o = engines
    a, b = deep_ref.deep_pair(w, h, seed)
    got = both_formats(g, a, b, t)
    want = deep_ref.expected_frame(o, a, b, t)
    mx, f0, f1, psnr = deep_ref.report(got, want)
    print("deep parity %dx%d t=%g: max %d, exact %.6f, off-by-one %.6f, PSNR %.2f dB" % (w, h, t, mx, f0, f1, psnr))
    assert mx <= 1, (mx, f0, f1, psnr)


@pytest.mark.parametrize("w,h", [(1, 1), (31, 33), (8, 300), (520, 16), (33, 32)])
def test_extreme_sizes_within_1_code(engines, w, h):
    g, o = engines
    a, b = deep_ref.deep_pair(w, h, 77)
    got = both_formats(g, a, b, 0.5)
    mx, f0, f1, psnr = deep_ref.report(got, deep_ref.expected_frame(o, a, b, 0.5))
    print("deep parity %dx%d: max %d, exact %.6f" % (w, h, mx, f0))
    assert mx <= 1, (w, h, mx)


@pytest.mark.parametrize("w,h,seed", [(1920, 1080, 2000), (3840, 2160, 3000)])
def test_large_frames_within_1_code_and_share_bounded_by_depth_8(engines, w, h, seed):
    """1080p and 4K: <= 1 code, and the off-by-one share p10 against the 8-bit path's p8 on the same scene rounded to 8 bits: p10 <= 8 * max(p8, 1e-5)."""
    g, o = engines
    a, b = deep_ref.deep_pair(w, h, seed)
    got = both_formats(g, a, b, 0.5)
    mx, f0, p10, psnr = deep_ref.report(got, deep_ref.expected_frame(o, a, b, 0.5))
    a8, b8 = deep_ref.to_depth8(a), deep_ref.to_depth8(b)
    mx8, f08, p8, psnr8 = deep_ref.report(g.process(a8, b8, 0.5), o.process(a8, b8, 0.5), 8)
    print("deep parity %dx%d: depth 10 max %d, p10 %.3e, PSNR %.2f dB; depth 8 max %d, p8 %.3e, PSNR %.2f dB; p10 / max(p8, 1e-5) = %.2f"
          % (w, h, mx, p10, psnr, mx8, p8, psnr8, p10 / max(p8, 1e-5)))
    assert mx <= 1 and mx8 <= 1, (mx, mx8)
    assert p10 <= 8 * max(p8, 1e-5), (p10, p8)


# ---- 2. before quantisation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(64, 64), (160, 96)])
def test_stage_flows_match_oracle(tap_engines, w, h):
    g, o, _ = tap_engines
    a, b = deep_ref.deep_pair(w, h, 21)
    for fmt in (U16, PACKED):
        fa, fb = (a, b) if fmt == U16 else (amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b))
        for fi in range(4):
            got = g.v4_extract_flow(fa, fb, 0.5, fi)
            want = deep_ref.extract(o, a, b, 0.5, 10, "flow%d" % fi)
            assert got.shape == want.shape
            assert np.abs(got - want).max() < 1e-3, (fmt, fi, float(np.abs(got - want).max()))


@pytest.mark.parametrize("w,h,seed", [(100, 60, 1), (256, 192, 2), (640, 360, 3), (333, 241, 4)])
@pytest.mark.parametrize("b", [1, 2, 3])
def test_block_input_bit_exact_and_through_the_stem_kernels(tap_engines, w, h, seed, b):
    """The 10-bit gather code on injected flows that leave the frame by hundreds of pixels: k_assemble<S, 10> bit for bit, the fused stem kernel to 2^-22
    relative, block 3 also through the row-streaming stem kernel (2^-21)."""
    g, o, names = tap_engines
    a, c = deep_ref.deep_pair(w, h, seed, amp=512 if seed % 2 else 6)      # odd seeds: every pixel is an edge
    inj = injected_flows(w, h, 100 + seed, b)
    t = 0.3 + 0.1 * b
    want = deep_ref.extract(o, a, c, t, 10, names[b - 1], flows=inj)
    assert want.shape[0] == 12
    S = (4, 2, 1)[b - 1]
    assert np.abs(want[8:12]).max() * S > 100, "injected flows too small to exercise the clamps"
    got0 = g.v4_tap(a, c, t, 0, b, inj)
    assert np.array_equal(got0, want), "k_assemble<%d, 10>: %d of %d floats differ, max %g" % (S, int((got0 != want).sum()), want.size, float(np.abs(got0 - want).max()))
    got0p = g.v4_tap(amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(c), t, 0, b, inj)
    assert np.array_equal(got0p, want)
    got1 = g.v4_tap(a, c, t, 1, b, inj)
    err = np.abs(got1 - want) - (3e-7 * np.abs(want) + 1.2e-7)       # hi + lo of a value: 2^-22 relative, f16 subnormal floor
    assert err.max() <= 0, "fused stem kernel of block %d: worst excess %g" % (b, float(err.max()))
    if b == 3:
        got5 = g.v4_tap(a, c, t, 5, 3, inj)
        err = np.abs(got5 - want) - (6e-7 * np.abs(want) + 2.4e-7)   # twice through the split-f16 path: 2^-21 relative
        assert err.max() <= 0, "stem_rs_kernel<0, 10>: worst excess %g" % float(err.max())


@pytest.mark.parametrize("w,h,seed", [(100, 60, 1), (256, 192, 2), (640, 360, 3), (333, 241, 4)])
def test_tail_on_injected_flows(tap_engines, w, h, seed):
    g, o, _ = tap_engines
    a, c = deep_ref.deep_pair(w, h, 40 + seed)
    inj = injected_flows(w, h, 200 + seed, 4)
    want = deep_ref.extract(o, a, c, 0.45, 10, "out0", flows=inj)
    got = g.v4_tap(a, c, 0.45, 2, 0, inj)
    d = np.abs(got - want)
    assert d.max() < 2e-6, "unfused tail at depth 10: max %g (expf is the only operation that may differ by an ulp)" % float(d.max())


# ---- 3. exact identities --------------------------------------------------------------------------------------------------------------

def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


@pytest.mark.parametrize("w,h,n", [(1920, 1080, 5), (640, 360, 4), (100, 60, 3)])
@pytest.mark.parametrize("fmt", [U16, PACKED])
def test_host_device_resident_batch_and_partition_streams_agree(engines, w, h, n, fmt):
    import torch
    g, _ = engines
    conv = (lambda x: x) if fmt == U16 else amd.pack_a2b10g10r10
    prs = [tuple(conv(f) for f in deep_ref.deep_pair(w, h, 40 + i)) for i in range(n)]
    ts = [0.5, 0.25, 1.0, 0.7, 0.125][:n]
    want = [g.process(p[0], p[1], t) for p, t in zip(prs, ts)]
    # resident frames
    for p, t, wnt in zip(prs, ts, want):
        f0, f1 = g.upload(p[0]), g.upload(p[1])
        assert f0.pixfmt == fmt
        assert np.array_equal(g.process_frames(f0, f1, t), wnt)
        f0.release(); f1.release()
    # device pointers: the engine's own stream, a caller stream, a stream that owns a quarter of the compute units
    d0 = [_dev(p[0]) for p in prs]; d1 = [_dev(p[1]) for p in prs]
    part = g.stream_create(1, 4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, st.cuda_stream, part):
        outs = [torch.zeros_like(x) for x in d0]
        for i in range(n):
            g.process_device(d0[i].data_ptr(), d1[i].data_ptr(), w, h, ts[i], outs[i].data_ptr(), stream, pixfmt=fmt)
        torch.cuda.synchronize()
        for i in range(n):
            assert np.array_equal(_host(outs[i], want[i]), want[i]), (i, stream)
    g.stream_destroy(part)
    # batches of 1..n pairs (lockstep groups of two, an odd pair left over, timestep 1 copies)
    for k in range(1, n + 1):
        outs = [torch.zeros_like(x) for x in d0[:k]]
        g.process_device_batch([x.data_ptr() for x in d0[:k]], [x.data_ptr() for x in d1[:k]], w, h, ts[:k], [o.data_ptr() for o in outs], st.cuda_stream, pixfmt=fmt)
        st.synchronize()
        for i in range(k):
            assert np.array_equal(_host(outs[i], want[i]), want[i]), (k, i)
    outs = [torch.zeros_like(x) for x in d0]
    g.process_device_batch([x.data_ptr() for x in d0], [x.data_ptr() for x in d1], w, h, ts, [o.data_ptr() for o in outs], None, pixfmt=fmt)
    for i in range(n):
        assert np.array_equal(_host(outs[i], want[i]), want[i]), i


@pytest.mark.parametrize("fmt", [U16, PACKED])
def test_device_frames_at_less_aligned_addresses_equal_aligned_ones(engines, fmt):
    """The one-pixel-per-lane pre-processing kernels (frames whose address is not 8- / 16-byte aligned) against the four-pixel forms and the host call."""
    import torch
    g, _ = engines
    w, h = 128, 72
    a, b = deep_ref.deep_pair(w, h, 4242)
    if fmt == PACKED:
        a, b = amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b)
    want = g.process(a, b, 0.5)
    n = a.nbytes
    for off in ((0, 2, 4, 6) if fmt == U16 else (0, 4, 8, 12)):
        b0 = torch.zeros(n + 16, dtype=torch.uint8, device="cuda"); b1 = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        b0[off:off + n] = _dev(a); b1[off:off + n] = _dev(b)
        out = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.process_device(b0.data_ptr() + off, b1.data_ptr() + off, w, h, 0.5, out.data_ptr() + off, None, pixfmt=fmt)
        torch.cuda.synchronize()
        assert np.array_equal(_host(out[off:off + n], want), want), off


def test_timestep_endpoints_return_the_inputs_in_canonical_form(engines):
    import torch
    g, _ = engines
    a, b = deep_ref.deep_pair(64, 48, 3)
    a = a.copy(); a[0, 0] = (1024, 4095, 65535)                       # codes above 1023 come back as 1023
    ac = np.minimum(a, 1023)
    assert np.array_equal(g.process(a, b, 0.0), ac) and np.array_equal(g.process(a, b, 1.0), b)
    pa, pb = amd.pack_a2b10g10r10(a) & np.uint32(0x3fffffff), amd.pack_a2b10g10r10(b) & np.uint32(0x7fffffff)      # alpha 0 and 1 on input
    assert np.array_equal(g.process(pa, pb, 0.0), amd.pack_a2b10g10r10(a)) and np.array_equal(g.process(pa, pb, 1.0), amd.pack_a2b10g10r10(b))
    f0, f1 = g.upload(a), g.upload(b)
    assert np.array_equal(g.process_frames(f0, f1, 0.0), ac) and np.array_equal(g.process_frames(f0, f1, 1.0), b)
    d0, d1 = _dev(a), _dev(b); out = torch.zeros_like(d0)
    torch.cuda.synchronize()
    g.process_device(d0.data_ptr(), d1.data_ptr(), 64, 48, 0.0, out.data_ptr(), None, pixfmt=U16)
    assert np.array_equal(_host(out, a), ac)
    g.process_device_batch([d0.data_ptr()], [d1.data_ptr()], 64, 48, [0.0], [out.data_ptr()], None, pixfmt=U16)
    assert np.array_equal(_host(out, a), ac)


def test_codes_above_1023_read_as_1023_and_alpha_is_ignored(engines):
    g, _ = engines
    a, b = deep_ref.deep_pair(160, 96, 5)
    a2 = a.copy(); a2[::3, ::5] = 1023
    hot = a2.copy(); hot[::3, ::5] = (1024, 40000, 65535)
    assert np.array_equal(g.process(hot, b, 0.4), g.process(a2, b, 0.4))
    rng = np.random.default_rng(1)
    pa, pb = amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b)
    ra = (pa & np.uint32(0x3fffffff)) | (rng.integers(0, 4, pa.shape).astype(np.uint32) << 30)
    rb = (pb & np.uint32(0x3fffffff)) | (rng.integers(0, 4, pb.shape).astype(np.uint32) << 30)
    got = g.process(ra, rb, 0.4)
    assert np.array_equal(got, g.process(pa, pb, 0.4)) and np.all(got >> 30 == 3)


def test_reentrant_and_4k_run_to_run_identical(engines):
    g, _ = engines
    a, b = deep_ref.deep_pair(320, 192, 4)
    ref = g.process(a, b, 0.5)
    outs = [None] * 4

    def work(i):
        outs[i] = g.process(a, b, 0.5)
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in th]; [t.join() for t in th]
    for o in outs:
        assert np.array_equal(o, ref)
    a, b = deep_ref.deep_pair(3840, 2160, 705)
    pa, pb = amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b)
    x = g.process(pa, pb, 0.5)
    assert np.array_equal(x, g.process(pa, pb, 0.5))


@pytest.mark.parametrize("fam", ["rife-v4.6", "rife-v4", "rife-v2.3", "rife-v3.1", "rife", "rife-HD"])
def test_px_calls_with_rgb8_are_the_old_entry_points(modeldirs, fam):
    import ctypes
    import torch
    kw = dict(rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    g = amd.RIFE(0, **kw); g.load(modeldirs[fam])
    w, h = 96, 64
    a, b = gen_frames.smooth_pair(w, h, 9)
    want = g.process(a, b, 0.5)
    assert np.array_equal(g.process(a, b, 0.5, pixfmt=amd.PIX_RGB8), want)
    L, p = g._L, amd._p
    out = np.zeros_like(a)
    assert L.rife_hip_process_px(g._h, p(a), p(b), w, h, 0.5, p(out), 0) == 0 and np.array_equal(out, want)
    fr = [ctypes.c_void_p(), ctypes.c_void_p()]
    assert L.rife_hip_frame_upload_px(g._h, p(a), w, h, 0, ctypes.byref(fr[0])) == 0 and L.rife_hip_frame_upload_px(g._h, p(b), w, h, 0, ctypes.byref(fr[1])) == 0
    out[:] = 0
    assert L.rife_hip_process_frames(g._h, fr[0], fr[1], 0.5, p(out)) == 0 and np.array_equal(out, want)
    L.rife_hip_frame_release(fr[0]); L.rife_hip_frame_release(fr[1])
    d0, d1 = _dev(a), _dev(b); do = torch.zeros_like(d0)
    torch.cuda.synchronize()
    assert L.rife_hip_process_device_px(g._h, d0.data_ptr(), d1.data_ptr(), w, h, 0.5, do.data_ptr(), 0, None) == 0
    assert np.array_equal(_host(do, a), want)
    do.zero_(); torch.cuda.synchronize()
    pa, pb, po = (ctypes.c_void_p * 1)(d0.data_ptr()), (ctypes.c_void_p * 1)(d1.data_ptr()), (ctypes.c_void_p * 1)(do.data_ptr())
    assert L.rife_hip_process_device_batch_px(g._h, 1, pa, pb, (ctypes.c_float * 1)(0.5), po, w, h, 0, None) == 0
    assert np.array_equal(_host(do, a), want)
    assert amd.frame_bytes(w, h, 0) == w * h * 3 and amd.frame_bytes(w, h, 1) == w * h * 6 and amd.frame_bytes(w, h, 2) == w * h * 4 and amd.frame_bytes(w, h, 3) == 0


@pytest.mark.parametrize("w,h", [(256, 192), (1000, 520)])
def test_a_workspace_serves_both_depths_in_turn(modeldirs, w, h):
    """One stream workspace: a 10-bit call, then an 8-bit call of the same size, and the reverse, against fresh engines."""
    import torch
    d = modeldirs["rife-v4.6"]
    a, b = deep_ref.deep_pair(w, h, 12)
    a8, b8 = deep_ref.to_depth8(a), deep_ref.to_depth8(b)
    fresh = amd.RIFE(0, rife_v4=True); fresh.load(d)
    want10, want8 = fresh.process(a, b, 0.5), fresh.process(a8, b8, 0.5)
    d10 = (_dev(a), _dev(b)); d8 = (_dev(a8), _dev(b8))
    for order in ((10, 8, 10), (8, 10, 8)):
        g = amd.RIFE(0, rife_v4=True); g.load(d)
        for depth in order:
            src, like, want = (d10, a, want10) if depth == 10 else (d8, a8, want8)
            out = torch.zeros_like(src[0]); torch.cuda.synchronize()
            g.process_device(src[0].data_ptr(), src[1].data_ptr(), w, h, 0.5, out.data_ptr(), None, pixfmt=U16 if depth == 10 else amd.PIX_RGB8)
            assert np.array_equal(_host(out, like), want), (order, depth)
        # the pooled workspaces of the host path as well
        assert np.array_equal(g.process(a, b, 0.5), want10) and np.array_equal(g.process(a8, b8, 0.5), want8) and np.array_equal(g.process(a, b, 0.5), want10)


# ---- 4. row-streaming kernels == tile kernels at depth 10 ----------------------------------------------------------------------------

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


@pytest.mark.parametrize("w,h,seed", [(256, 192, 1), (640, 360, 2), (333, 241, 3), (100, 60, 4), (33, 47, 5), (130, 9, 7), (1000, 520, 8), (1920, 1080, 9), (3840, 2160, 11)])
def test_row_streaming_kernels_match_the_tile_kernels(modeldirs, w, h, seed):
    """tail_rs_kernel<0, PX> against head_h2_kernel<EPI_FINAL, true, PX> and stem_rs_kernel<0, 10> against the tile stems.  The kernels sum in different
    orders: within 1 code, and at most 4.01e-3 of the channels touched - the 8-bit tests' 1e-3 times the 1023 / 255 rounding boundaries a fixed difference
    crosses at depth 10."""
    d = modeldirs["rife-v4.6"]
    rs = _switched(d, RIFE_HIP_TAIL_RS="2", RIFE_HIP_STEM_RS="1")
    tile = _switched(d, RIFE_HIP_TAIL_RS="0", RIFE_HIP_STEM_RS="0")
    a, c = deep_ref.deep_pair(w, h, 20 + seed, amp=512 if seed % 3 == 0 else 6)
    for fmt in (U16, PACKED):
        x, y = (a, c) if fmt == U16 else (amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(c))
        p1, p0 = rs.process(x, y, 0.5), tile.process(x, y, 0.5)
        if fmt == PACKED:
            p1, p0 = amd.unpack_a2b10g10r10(p1), amd.unpack_a2b10g10r10(p0)
        dd = np.abs(p1.astype(np.int32) - p0.astype(np.int32))
        print("rs vs tile %dx%d fmt %d: %d of %d codes differ, max %d" % (w, h, fmt, int((dd > 0).sum()), dd.size, int(dd.max())))
        assert dd.max() <= 1 and (dd > 0).mean() < 4.01e-3, (w, h, fmt, int(dd.max()), float((dd > 0).mean()))
        assert np.array_equal(rs.process(x, y, 0.5), rs.process(x, y, 0.5))


@pytest.mark.parametrize("w,h", [(100, 60), (640, 360)])
def test_tile_trunk_path_within_1_code(modeldirs, w, h):
    """RIFE_HIP_T64=0: no S16 trunk tensors, so the tail is head_h2_kernel<EPI_FINAL, false, PX> on the NHWC trunk - against the oracle."""
    d = modeldirs["rife-v4.6"]
    g = _switched(d, RIFE_HIP_TAIL_RS="0", RIFE_HIP_STEM_RS="0", RIFE_HIP_T64="0")
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    a, b = deep_ref.deep_pair(w, h, 31)
    mx, f0, f1, psnr = deep_ref.report(both_formats(g, a, b, 0.5), deep_ref.expected_frame(o, a, b, 0.5))
    assert mx <= 1, (mx, f0, f1)


def test_unfused_fallbacks_within_1_code(modeldirs, tmp_path):
    """RIFE_HIP_TRUNK=f32 (a product switch, read once per process): no split-f16 kernels, so the pass runs k_assemble0_d10 / k_assemble<S, 10>, the fp32 convolutions
    and k_final_px<1 | 2> - the unfused fall-backs behind every fused kernel - in a child process; its frames against the oracle."""
    import subprocess
    import sys
    d = modeldirs["rife-v4.6"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, importlib, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import deep_ref\n"
        "amd = importlib.import_module('rife-ncnn-vulkan_amd')\n"
        "g = amd.RIFE(0, rife_v4=True); g.load(%r)\n"
        "for (w, h) in ((100, 60), (256, 192)):\n"
        "    a, b = deep_ref.deep_pair(w, h, 50)\n"
        "    u = g.process(a, b, 0.4); p = g.process(amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b), 0.4)\n"
        "    assert np.array_equal(amd.unpack_a2b10g10r10(p), u) and np.all(p >> 30 == 3)\n"
        "    np.save(%r %% (w, h), u)\n") % (root, os.path.join(root, "tests"), d, str(tmp_path / "f32_%dx%d.npy"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, RIFE_HIP_TRUNK="f32"), timeout=600)
    assert p.returncode == 0, p.stderr[-800:]
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    for (w, h) in ((100, 60), (256, 192)):
        a, b = deep_ref.deep_pair(w, h, 50)
        mx, f0, f1, psnr = deep_ref.report(np.load(str(tmp_path / ("f32_%dx%d.npy" % (w, h)))), deep_ref.expected_frame(o, a, b, 0.4))
        assert mx <= 1, (w, h, mx, f0, f1)


@pytest.mark.parametrize("w,h", [(256, 192), (640, 360)])
def test_fused_flow_updates_are_bit_identical_at_depth_10(modeldirs, w, h):
    """RIFE_HIP_FUSE_FLOW=1 (stem0_fused_kernel<S, NS, ABL, 1, 10>: the flow update inside the stem) against the update kernels, both on the tile stems."""
    d = modeldirs["rife-v4.6"]
    a, c = deep_ref.deep_pair(w, h, 11)
    g0 = _switched(d, RIFE_HIP_STEM_RS="0", RIFE_HIP_FUSE_FLOW="0")
    g1 = _switched(d, RIFE_HIP_STEM_RS="0", RIFE_HIP_FUSE_FLOW="1")
    for t in (0.5, 0.2):
        x0, x1 = g0.process(a, c, t), g1.process(a, c, t)
        assert np.array_equal(x0, x1), "%d codes differ" % int((x0 != x1).sum())


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,kw,word", [("rife-v4", {}, "rife-v4"), ("rife-v2.3", {}, "rife-v2"), ("rife-v3.1", {}, "rife-v3"), ("rife", {}, "v1"), ("rife-HD", {}, "v1"),
                                         ("rife-v4.6", dict(tta_mode=True), "TTA"), ("rife-v4.6", dict(tta_temporal_mode=True), "temporal"),
                                         ("rife-v4.6", dict(uhd_mode=True), "UHD")])
def test_other_families_and_modes_are_refused_with_enosys(modeldirs, fam, kw, word):
    import torch
    fl = dict(kw, rife_v2=fam.startswith(("rife-v2", "rife-v3")), rife_v4=fam.startswith("rife-v4"))
    g = amd.RIFE(0, **fl); g.load(modeldirs[fam])
    a, b = deep_ref.deep_pair(64, 64, 1)
    for x, y in ((a, b), (amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b))):
        out = np.full_like(x, 0x5a5a if x.dtype == np.uint16 else 0x5a5a5a5a)
        keep = out.copy()
        for t in (0.5, 0.0):
            with pytest.raises(amd.RifeError) as e:
                g.process(x, y, t, outimage=out)
            assert "(-6)" in str(e.value) and word in str(e.value), str(e.value)
            assert np.array_equal(out, keep), "the output buffer was written"
        with pytest.raises(amd.RifeError) as e:
            g.upload(x)
        assert "(-6)" in str(e.value)
        d0, d1 = _dev(x), _dev(y); do = _dev(out)
        torch.cuda.synchronize()
        fmt = U16 if x.dtype == np.uint16 else PACKED
        with pytest.raises(amd.RifeError) as e:
            g.process_device(d0.data_ptr(), d1.data_ptr(), 64, 64, 0.5, do.data_ptr(), None, pixfmt=fmt)
        assert "(-6)" in str(e.value)
        with pytest.raises(amd.RifeError) as e:
            g.process_device_batch([d0.data_ptr()] * 2, [d1.data_ptr()] * 2, 64, 64, [0.5, 0.3], [do.data_ptr()] * 2, None, pixfmt=fmt)
        assert "(-6)" in str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(_host(do, out), keep)
    # the 8-bit path of the same engine is untouched by the refusals
    a8, b8 = gen_frames.smooth_pair(64, 64, 2)
    assert g.process(a8, b8, 0.5).shape == a8.shape
