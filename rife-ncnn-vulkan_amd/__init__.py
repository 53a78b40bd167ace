"""rife-ncnn-vulkan_amd — MI355X-native RIFE frame interpolation behind the reference's `RIFE` surface.

Python host-side mirror of the reference's C++ class (nihui/rife-ncnn-vulkan src/rife.h:11-52):

    r = RIFE(gpuid, tta_mode=False, tta_temporal_mode=False, uhd_mode=False, num_threads=1, rife_v2=False, rife_v4=False)
    r.load(modeldir)                       # RIFE::load,    src/rife.cpp:127-379
    out = r.process(in0, in1, timestep)    # RIFE::process, src/rife.cpp:381-1212 / 2462-3202

Everything is computed by the hand-written HIP kernels in csrc/ through the C-ABI of include/rife_hip.h
(librife_hip.so).  There is no CPU or PyTorch fallback: importing works without a GPU, computing does not.
The package name contains '-' and '.', so import it with importlib.import_module("rife-ncnn-vulkan_amd").
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RIFE_HIP_LIB: load another build of the same sources as "the product" (tools/*.py A/B two builds with it; the tests never set it)
LIB_PATH = os.environ.get("RIFE_HIP_LIB") or os.path.join(_HERE, "librife_hip.so")
# the TEST build: same sources + -DRIFE_HIP_TEST_BUILD = include/rife_hip_test.h's parity taps / single-kernel entry points and the kernel-selection
# switches (RIFE_HIP_T64, _RS, _KS, _STEM_RS, _TAIL_RS, _FUSE_FLOW, ...) the kernel-vs-kernel tests flip.  The product exports include/rife_hip.h only.
TEST_LIB_PATH = os.path.join(_HERE, "librife_hip_test.so")
_lib = None
_testlib = None

# every symbol include/rife_hip.h declares (= everything the product library exports)
C_ABI_SYMBOLS = [
    "rife_hip_device_count", "rife_hip_create", "rife_hip_destroy", "rife_hip_load", "rife_hip_process",
    "rife_hip_process_device", "rife_hip_process_device_batch", "rife_hip_stream_create", "rife_hip_stream_destroy", "rife_hip_process_batch", "rife_hip_frame_upload", "rife_hip_process_frames", "rife_hip_frame_release",
    "rife_hip_last_error", "rife_hip_profile_enable", "rife_hip_profile_read",
    "rife_hip_host_alloc", "rife_hip_host_free", "rife_hip_host_register", "rife_hip_host_unregister",
    "rife_hip_graph_check", "rife_hip_param_hash",
    "rife_hip_frame_bytes", "rife_hip_process_px", "rife_hip_process_device_px", "rife_hip_process_device_batch_px", "rife_hip_frame_upload_px",
    "rife_hip_image_check", "rife_hip_image_row_bytes", "rife_hip_process_image", "rife_hip_process_device_image", "rife_hip_frame_upload_image", "rife_hip_process_frames_image",
    "rife_hip_set_flow_scale", "rife_hip_flow_scale",
    "rife_hip_set_precision", "rife_hip_precision",
    "rife_hip_motion_check", "rife_hip_process_motion", "rife_hip_process_device_motion", "rife_hip_process_frames_motion",
    "rife_hip_planes_check", "rife_hip_padded_size", "rife_hip_apply_device_motion", "rife_hip_apply_motion", "rife_hip_process_apply", "rife_hip_process_device_apply",
    "rife_hip_apply_set_check", "rife_hip_apply_device_motion_sets", "rife_hip_apply_motion_sets", "rife_hip_process_apply_sets", "rife_hip_process_device_apply_sets",
    "rife_hip_hbd_check", "rife_hip_process_hbd", "rife_hip_process_device_hbd",
    "rife_hip_packed_check", "rife_hip_process_hbd_packed", "rife_hip_process_device_hbd_packed",
    "rife_hip_semiplanar_check", "rife_hip_process_hbd_semiplanar", "rife_hip_process_device_hbd_semiplanar",
]
# include/rife_hip.h RIFE_HIP_PRECISION_*: FULL = two f16 products per weight tap of the residual trunks (fp32-equivalent), FAST = one, the skip at full precision
PRECISION_FULL, PRECISION_FAST = 0, 1
_PRECISION_NAMES = {"full": PRECISION_FULL, "fast": PRECISION_FAST}
# pixel formats at the C boundary (include/rife_hip.h RIFE_HIP_PIX_*)
PIX_RGB8, PIX_RGB10_U16, PIX_A2B10G10R10 = 0, 1, 2
PIX_RGBA8 = 4      # 3 is reserved
# Y'CbCr (flat arrays: uint8 for NV12 / I420, uint16 for P010 / I420P10); the colour description is OR-ed into the format
PIX_NV12, PIX_I420, PIX_P010, PIX_I420P10 = 16, 17, 18, 19      # 5 .. 15 are reserved
# 4:2:2 and 4:4:4, planar (16 * class + 2 * (10 bits) + planar; class 2 = 4:2:2, 3 = 4:4:4): Y (h, w), then Cb and Cr of (h, cw) / (h, w) samples
PIX_I422, PIX_I422P10, PIX_I444, PIX_I444P10 = 33, 35, 49, 51
_YUV_FORMATS = (PIX_NV12, PIX_I420, PIX_P010, PIX_I420P10, PIX_I422, PIX_I422P10, PIX_I444, PIX_I444P10)
# planar RGB (class 4; k = 0 u8, 1 u16, 2 half, 3 float): three (h, w) planes R, G, B of uint8 / uint16 (codes 0..1023) / float16 / float32 (nominal range [0, 1])
PIX_RGBP8, PIX_RGBP10, PIX_RGBPH, PIX_RGBPF = 65, 67, 69, 71
_RGBP_DTYPE = {PIX_RGBP8: np.uint8, PIX_RGBP10: np.uint16, PIX_RGBPH: np.float16, PIX_RGBPF: np.float32}
CSP_BT709, CSP_BT601, CSP_BT2020NCL = 0 << 8, 1 << 8, 2 << 8
CSP_FULL = 1 << 12
ENOSYS = 6      # RIFE_HIP_ENOSYS: calls return its negative
# motion export (include/rife_hip.h RIFE_HIP_MOTION_*): the sample type of the flow and mask buffers
MOTION_F32, MOTION_F16 = 0, 1
_MOTION_DTYPE = {MOTION_F32: np.float32, MOTION_F16: np.float16}
# apply motion (include/rife_hip.h RIFE_HIP_SAMPLE_*): the sample type of the planes a motion field is applied to
SAMPLE_U8, SAMPLE_U16, SAMPLE_F16, SAMPLE_F32 = 0, 1, 2, 3
_SAMPLE_DTYPE = {SAMPLE_U8: np.uint8, SAMPLE_U16: np.uint16, SAMPLE_F16: np.float16, SAMPLE_F32: np.float32}
_SAMPLE_OF = {np.dtype(v): k for k, v in _SAMPLE_DTYPE.items()}
# include/rife_hip_test.h: exported by librife_hip_test.so (and the bench build) only
TEST_ABI_SYMBOLS = ["rife_hip_v4_extract_flow", "rife_hip_v4_flow_dims", "rife_hip_v4_tap", "rife_hip_v4_process_injected", "rife_hip_op_conv3x3", "rife_hip_op_deconv4x4", "rife_hip_op_warp", "rife_hip_pool_state",
                    "rife_hip_v4_extract_flow_px", "rife_hip_v4_tap_px", "rife_hip_op_yuv_to_rgb10", "rife_hip_op_rgb10_to_yuv",
                    "rife_hip_op_image_to_resident", "rife_hip_op_resident_to_image", "rife_hip_op_s16_geom", "rife_hip_op_trunk", "rife_hip_v4_process_injected_px",
                    "rife_hip_op_trunk_prec", "rife_hip_op_stem1_s16", "rife_hip_op_head_ps", "rife_hip_op_tail", "rife_hip_op_tail_motion", "rife_hip_op_apply", "rife_hip_op_apply_scaled", "rife_hip_op_hbd_to_rgb10", "rife_hip_op_apply_yuv",
                    "rife_hip_op_packed_to_rgb10", "rife_hip_op_apply_packed", "rife_hip_op_sp_to_rgb10", "rife_hip_op_apply_sp",
                    "rife_hip_graph_plan", "rife_hip_graph_eval",
                    "rife_hip_op_v2_assemble", "rife_hip_op_v2_stem", "rife_hip_op_v2_flow_accum", "rife_hip_op_v2_ctx_warps", "rife_hip_op_v2_final", "rife_hip_op_v2_uhd",
                    "rife_hip_op_v2_conv_img", "rife_hip_op_conv_pair"]
# rife_hip_op_v2_stem: which launches run the stem (include/rife_hip_test.h RIFE_HIP_V2_STEM_*)
V2_STEM_PRODUCT, V2_STEM_NO_R64, V2_STEM_UNFUSED = 0, 1, 2
# rife_hip_op_tail: which kernel writes the frame (include/rife_hip_test.h RIFE_HIP_TAIL_*), and the guard bytes on either side of the frame
TAIL_RS, TAIL_HEAD_S16, TAIL_HEAD_F32, TAIL_UNFUSED = 0, 1, 2, 3
TAIL_GUARD = 256
# rife_hip_op_trunk: which S16 trunk kernel (include/rife_hip_test.h RIFE_HIP_TRUNK_*)
TRUNK_T64, TRUNK_RS, TRUNK_RS2, TRUNK_ROW, TRUNK_KS = 0, 1, 2, 3, 4
EINVAL = 1      # RIFE_HIP_EINVAL: calls return its negative


class rife_hip_image(ctypes.Structure):
    """rife_hip_image_t of include/rife_hip.h: a frame as a pointer and a pitch in BYTES per plane."""
    _fields_ = [("w", ctypes.c_int), ("h", ctypes.c_int), ("pixfmt", ctypes.c_int), ("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_ssize_t * 3)]


class rife_hip_motion(ctypes.Structure):
    """rife_hip_motion_t of include/rife_hip.h: where a motion call puts the final flows (h rows of w pixels of dx0, dy0, dx1, dy1) and the blend mask (h rows of
    w samples); pitches in BYTES, either pointer may be null (not wanted)."""
    _fields_ = [("flow", ctypes.c_void_p), ("flow_pitch", ctypes.c_size_t), ("mask", ctypes.c_void_p), ("mask_pitch", ctypes.c_size_t), ("format", ctypes.c_int)]


class rife_hip_planes(ctypes.Structure):
    """rife_hip_planes_t of include/rife_hip.h: n (1..4) planes of w x h samples of one type, a pointer and a pitch in BYTES each; maxval for integer samples, else 0."""
    _fields_ = [("w", ctypes.c_int), ("h", ctypes.c_int), ("n", ctypes.c_int), ("sample", ctypes.c_int), ("maxval", ctypes.c_int), ("plane", ctypes.c_void_p * 4),
                ("pitch", ctypes.c_ssize_t * 4)]


class rife_hip_packed(ctypes.Structure):
    """rife_hip_packed_t of include/rife_hip.h: h rows of w pixels of `channels` (3, 4) interleaved u16 samples of `depth` bits, a pointer and a pitch in BYTES."""
    _fields_ = [("w", ctypes.c_int), ("h", ctypes.c_int), ("channels", ctypes.c_int), ("depth", ctypes.c_int), ("data", ctypes.c_void_p), ("pitch", ctypes.c_ssize_t)]


class rife_hip_semiplanar(ctypes.Structure):
    """rife_hip_semiplanar_t of include/rife_hip.h: a Y plane and one plane of interleaved Cb, Cr pairs, codes of `depth` bits in the HIGH bits of u16; chroma 1 = 4:2:0,
    2 = 4:2:2; a pointer and a pitch in BYTES per plane."""
    _fields_ = [("w", ctypes.c_int), ("h", ctypes.c_int), ("chroma", ctypes.c_int), ("csp", ctypes.c_int), ("depth", ctypes.c_int), ("y", ctypes.c_void_p),
                ("pitch_y", ctypes.c_ssize_t), ("cbcr", ctypes.c_void_p), ("pitch_c", ctypes.c_ssize_t)]


class rife_hip_apply_set(ctypes.Structure):
    """rife_hip_apply_set_t of include/rife_hip.h: three plane descriptors, the shift of the planes relative to the motion per axis and the extent in plane pixels."""
    _fields_ = [("p0", ctypes.POINTER(rife_hip_planes)), ("p1", ctypes.POINTER(rife_hip_planes)), ("out", ctypes.POINTER(rife_hip_planes)),
                ("shift_x", ctypes.c_int), ("shift_y", ctypes.c_int), ("wp", ctypes.c_int), ("hp", ctypes.c_int)]


def build(force=False):
    """Compile librife_hip.so (+ the test build, the class shim and the CLI) for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(_HERE, "..", "include", "rife_hip.h"), os.path.join(_HERE, "..", "include", "rife_hip_test.h")]
    outs = [os.path.join(_HERE, "librife_hip.so"), TEST_LIB_PATH]
    stale = any(not os.path.exists(o) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs) for o in outs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", csrc] + (["-B"] if force else []))
    return os.path.join(_HERE, "librife_hip.so")


def _load(path, with_test_surface):
    if not os.path.exists(path):
        raise RuntimeError("%s is not built (run __graft_entry__.build() or make -C rife-ncnn-vulkan_amd/csrc); there is no fallback path" % os.path.basename(path))
    try:
        import torch  # noqa: F401   (if PyTorch-ROCm is importable it is imported first so that both share one libamdhip64)
    except Exception:
        pass
    L = ctypes.CDLL(path)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.rife_hip_device_count.restype = ci
    L.rife_hip_create.restype = vp
    L.rife_hip_create.argtypes = [ci] * 7
    L.rife_hip_destroy.argtypes = [vp]
    L.rife_hip_load.argtypes = [vp, ctypes.c_char_p]
    L.rife_hip_process.argtypes = [vp, vp, vp, ci, ci, cf, vp]
    L.rife_hip_process_device.argtypes = [vp, vp, vp, ci, ci, cf, vp, vp]
    L.rife_hip_process_device_batch.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, vp]
    L.rife_hip_stream_create.argtypes = [vp, ci, ci, ctypes.POINTER(vp)]
    L.rife_hip_stream_destroy.argtypes = [vp, vp]
    L.rife_hip_last_error.restype = ctypes.c_char_p
    L.rife_hip_profile_enable.argtypes = [vp, ci]
    L.rife_hip_profile_read.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, vp, vp, vp, ci]
    L.rife_hip_graph_check.argtypes = [ctypes.c_char_p]
    L.rife_hip_process_batch.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci]
    L.rife_hip_frame_upload.argtypes = [vp, vp, ci, ci, vp]
    L.rife_hip_process_frames.argtypes = [vp, vp, vp, cf, vp]
    L.rife_hip_frame_release.argtypes = [vp]
    L.rife_hip_param_hash.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    L.rife_hip_host_alloc.restype = vp
    L.rife_hip_host_alloc.argtypes = [ctypes.c_size_t]
    L.rife_hip_host_free.argtypes = [vp]
    L.rife_hip_host_register.argtypes = [vp, ctypes.c_size_t]
    L.rife_hip_host_unregister.argtypes = [vp]
    L.rife_hip_frame_bytes.restype = ctypes.c_size_t
    L.rife_hip_frame_bytes.argtypes = [ci, ci, ci]
    L.rife_hip_process_px.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci]
    L.rife_hip_process_device_px.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, vp]
    L.rife_hip_process_device_batch_px.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, vp]
    L.rife_hip_frame_upload_px.argtypes = [vp, vp, ci, ci, ci, vp]
    ip = ctypes.POINTER(rife_hip_image)
    L.rife_hip_image_check.argtypes = [ip]
    L.rife_hip_image_row_bytes.restype = ctypes.c_size_t
    L.rife_hip_image_row_bytes.argtypes = [ci, ci, ci]
    L.rife_hip_process_image.argtypes = [vp, ip, ip, cf, ip]
    L.rife_hip_process_device_image.argtypes = [vp, ip, ip, cf, ip, vp]
    L.rife_hip_frame_upload_image.argtypes = [vp, ip, vp]
    L.rife_hip_process_frames_image.argtypes = [vp, vp, vp, cf, ip]
    L.rife_hip_set_flow_scale.argtypes = [vp, ci]
    L.rife_hip_flow_scale.argtypes = [vp]
    L.rife_hip_set_precision.argtypes = [vp, ci]
    L.rife_hip_precision.argtypes = [vp]
    mp = ctypes.POINTER(rife_hip_motion)
    L.rife_hip_motion_check.argtypes = [mp, ci, ci]
    L.rife_hip_process_motion.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, mp]
    L.rife_hip_process_device_motion.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, mp, vp]
    L.rife_hip_process_frames_motion.argtypes = [vp, vp, vp, cf, vp, mp]
    pp = ctypes.POINTER(rife_hip_planes)
    L.rife_hip_planes_check.argtypes = [pp]
    L.rife_hip_padded_size.argtypes = [vp, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.rife_hip_apply_device_motion.argtypes = [vp, pp, pp, mp, ci, ci, pp, vp]
    L.rife_hip_apply_motion.argtypes = [vp, pp, pp, mp, ci, ci, pp]
    L.rife_hip_process_apply.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, pp, pp, ci, ci, pp]
    L.rife_hip_process_device_apply.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, pp, pp, ci, ci, pp, vp]
    sp = ctypes.POINTER(rife_hip_apply_set)
    L.rife_hip_apply_set_check.argtypes = [sp, ci, ci]
    L.rife_hip_apply_device_motion_sets.argtypes = [vp, ci, sp, mp, ci, ci, vp]
    L.rife_hip_apply_motion_sets.argtypes = [vp, ci, sp, mp, ci, ci]
    L.rife_hip_process_apply_sets.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, ci, sp]
    L.rife_hip_process_device_apply_sets.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, ci, sp, vp]
    L.rife_hip_hbd_check.argtypes = [ip, ci]
    L.rife_hip_process_hbd.argtypes = [vp, ip, ip, cf, ip, ci]
    L.rife_hip_process_device_hbd.argtypes = [vp, ip, ip, cf, ip, ci, vp]
    kp = ctypes.POINTER(rife_hip_packed)
    L.rife_hip_packed_check.argtypes = [kp]
    L.rife_hip_process_hbd_packed.argtypes = [vp, kp, kp, cf, kp]
    L.rife_hip_process_device_hbd_packed.argtypes = [vp, kp, kp, cf, kp, vp]
    qp = ctypes.POINTER(rife_hip_semiplanar)
    L.rife_hip_semiplanar_check.argtypes = [qp]
    L.rife_hip_process_hbd_semiplanar.argtypes = [vp, qp, qp, cf, qp]
    L.rife_hip_process_device_hbd_semiplanar.argtypes = [vp, qp, qp, cf, qp, vp]
    if with_test_surface:
        L.rife_hip_op_apply.argtypes = [ci, pp, pp, mp, ci, ci, pp, ci]
        L.rife_hip_op_apply_scaled.argtypes = [ci, sp, mp, ci, ci, ci]
        L.rife_hip_op_hbd_to_rgb10.argtypes = [ci, ip, ci, vp, ci]
        L.rife_hip_op_apply_yuv.argtypes = [ci, sp, sp, mp, ci, ci]
        L.rife_hip_op_packed_to_rgb10.argtypes = [ci, kp, vp, ci]
        L.rife_hip_op_apply_packed.argtypes = [ci, kp, kp, kp, mp, ci]
        L.rife_hip_op_sp_to_rgb10.argtypes = [ci, qp, vp, ci]
        L.rife_hip_op_apply_sp.argtypes = [ci, qp, qp, qp, mp, ci, ci, ci]
        L.rife_hip_op_image_to_resident.argtypes = [ci, ip, ci, vp]
        L.rife_hip_op_resident_to_image.argtypes = [ci, vp, ip, ci]
        L.rife_hip_v4_extract_flow.argtypes = [vp, vp, vp, ci, ci, cf, ci, vp, ci, vp]
        L.rife_hip_v4_flow_dims.argtypes = [vp, ci, ci, ci, vp, vp, vp]
        L.rife_hip_v4_tap.argtypes = [vp, vp, vp, ci, ci, cf, ci, ci, vp, ci, vp]
        L.rife_hip_v4_process_injected.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, vp]
        L.rife_hip_v4_process_injected_px.argtypes = [vp, vp, vp, ci, ci, cf, vp, ci, vp, ci]
        L.rife_hip_op_conv3x3.argtypes = [ci, vp, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp]
        L.rife_hip_op_deconv4x4.argtypes = [ci, vp, ci, ci, ci, vp, vp, ci, vp, vp]
        L.rife_hip_op_warp.argtypes = [ci, vp, vp, ci, ci, ci, vp]
        L.rife_hip_pool_state.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.rife_hip_v4_extract_flow_px.argtypes = [vp, vp, vp, ci, ci, cf, ci, vp, ci, vp, ci]
        L.rife_hip_v4_tap_px.argtypes = [vp, vp, vp, ci, ci, cf, ci, ci, vp, ci, vp, ci]
        L.rife_hip_op_yuv_to_rgb10.argtypes = [ci, vp, ci, ci, ci, vp]
        L.rife_hip_op_rgb10_to_yuv.argtypes = [ci, vp, ci, ci, ci, vp]
        L.rife_hip_op_s16_geom.argtypes = [ci, ci, ci, vp, vp, vp, vp]
        L.rife_hip_op_trunk.argtypes = [ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, ci, ci, vp, vp]
        L.rife_hip_op_trunk_prec.argtypes = [ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, ci, ci, vp, vp, ci]
        L.rife_hip_op_stem1_s16.argtypes = [ci, ci, ci, ci, vp, vp, vp, cf, vp]
        L.rife_hip_op_head_ps.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp]
        L.rife_hip_op_tail.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp]
        L.rife_hip_op_tail_motion.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, ctypes.c_size_t, vp, ctypes.c_size_t]
        L.rife_hip_graph_plan.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        L.rife_hip_graph_eval.argtypes = [ci, ctypes.c_char_p, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci]
        L.rife_hip_op_v2_assemble.argtypes = [ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp]
        L.rife_hip_op_v2_stem.argtypes = [ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, ci, ci, vp]
        L.rife_hip_op_v2_flow_accum.argtypes = [ci, ci, ci, ci, vp, ci, ci, vp]
        L.rife_hip_op_v2_ctx_warps.argtypes = [ci, ci, vp, ci, ci, vp, vp, vp]
        L.rife_hip_op_v2_final.argtypes = [ci, ci, vp, vp, ci, ci, vp, vp, vp]
        L.rife_hip_op_v2_uhd.argtypes = [ci, ci, vp, ci, ci, vp]
        L.rife_hip_op_v2_conv_img.argtypes = [ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.rife_hip_op_conv_pair.argtypes = [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci]
    return L


def lib():
    """The PRODUCT C-ABI library (include/rife_hip.h)."""
    global _lib
    if _lib is None:
        surface = False
        if os.environ.get("RIFE_HIP_LIB") and os.path.exists(LIB_PATH):      # a test / bench build standing in for the product (tools/*.py): bind the taps it exports
            surface = hasattr(ctypes.CDLL(LIB_PATH), "rife_hip_v4_tap")
        _lib = _load(LIB_PATH, surface)
    return _lib


def testlib():
    """The TEST build (include/rife_hip.h + include/rife_hip_test.h + kernel-selection switches)."""
    global _testlib
    if _testlib is None:
        _testlib = _load(TEST_LIB_PATH, True)
    return _testlib


class _TestBuild:
    """`amd.test_build()`: the same Python surface on librife_hip_test.so - RIFE(...) engines with the parity taps and the RIFE_HIP_* kernel-selection switches,
    op_conv3x3 / op_deconv4x4 / op_warp / op_trunk.  Everything else resolves to the package itself."""

    def __init__(self, mod):
        self._mod = mod

    def RIFE(self, *a, **kw):
        return RIFE(*a, test_build=True, **kw)

    def lib(self):
        return testlib()

    def __getattr__(self, name):
        return getattr(self._mod, name)


def test_build():
    import sys
    testlib()
    return _TestBuild(sys.modules[__name__])


class RifeError(RuntimeError):
    pass


def _check(rc, what, L=None):
    if rc != 0:
        raise RifeError("%s failed (%d): %s" % (what, rc, (L or lib()).rife_hip_last_error().decode()))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def graph_check(param_base):
    """Raise RifeError if the generic graph executor has no kernel for some layer of <param_base>.param (CPU-only check)."""
    _check(lib().rife_hip_graph_check(param_base.encode()), "graph_check")


def pack_a2b10g10r10(rgb10):
    """(h, w, 3) uint16 codes -> (h, w) uint32 A2B10G10R10 (alpha 3); codes above 1023 are clamped like the engine reads them."""
    c = np.minimum(np.asarray(rgb10, np.uint32), 1023)
    return (c[..., 0] | (c[..., 1] << 10) | (c[..., 2] << 20) | np.uint32(0xc0000000)).astype(np.uint32)


def unpack_a2b10g10r10(packed):
    """(h, w) uint32 A2B10G10R10 -> (h, w, 3) uint16 codes."""
    p = np.asarray(packed, np.uint32)
    return np.stack([p & 1023, (p >> 10) & 1023, (p >> 20) & 1023], axis=-1).astype(np.uint16)


def device_count():
    return lib().rife_hip_device_count()


class _PinnedOwner:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        if self.ptr and _lib is not None:
            _lib.rife_hip_host_free(self.ptr)
        self.ptr = None


def pinned_empty(shape, dtype=np.uint8):
    """A numpy array in page-locked host memory (rife_hip_host_alloc): copies to / from it are asynchronous DMA at PCIe rate.
    The memory is released when the last array that views it is collected."""
    shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = lib().rife_hip_host_alloc(max(1, nbytes))
    if not ptr:
        raise RifeError("rife_hip_host_alloc(%d) failed: %s" % (nbytes, lib().rife_hip_last_error().decode()))
    buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(ptr)
    buf._owner = _PinnedOwner(ptr)        # arr.base -> buf -> owner: freed when the last view is collected
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def frame_bytes(w, h, pixfmt=PIX_RGB8):
    """rife_hip_frame_bytes: size of one w x h frame in `pixfmt` (0 for an unknown format)."""
    return int(lib().rife_hip_frame_bytes(int(w), int(h), int(pixfmt)))


def _yuv_base(pixfmt):
    b = int(pixfmt) & 0xff
    if int(pixfmt) < 0 or b not in _YUV_FORMATS:
        raise ValueError("%r is not a YUV pixfmt" % (pixfmt,))
    return b


def yuv_dtype(pixfmt):
    return np.uint16 if _yuv_base(pixfmt) & 2 else np.uint8


def yuv_chroma_dims(w, h, pixfmt):
    """(cw, ch) of a w x h frame: 4:2:0 ((w + 1) // 2, (h + 1) // 2), 4:2:2 ((w + 1) // 2, h), 4:4:4 (w, h)."""
    cls = _yuv_base(pixfmt) >> 4
    return (w if cls == 3 else (w + 1) // 2), (h if cls >= 2 else (h + 1) // 2)


def yuv_frame_bytes(w, h, pixfmt):
    """Size of one w x h YUV frame: (w * h + 2 * cw * ch) samples of 1 or 2 bytes, cw, ch = yuv_chroma_dims(w, h, pixfmt)."""
    cw, ch = yuv_chroma_dims(w, h, pixfmt)
    return (w * h + 2 * cw * ch) * np.dtype(yuv_dtype(pixfmt)).itemsize


def _yuv_buf(buf, w, h, pixfmt, what):
    dt = yuv_dtype(pixfmt)
    n = yuv_frame_bytes(w, h, pixfmt) // np.dtype(dt).itemsize
    if w <= 0 or h <= 0 or not isinstance(buf, np.ndarray) or buf.dtype != dt or buf.size != n or not buf.flags.c_contiguous:
        raise ValueError("%s must be a contiguous %s array of %d samples (a %dx%d frame)" % (what, np.dtype(dt).name, n, w, h))
    return buf


def planar_rgb_dtype(pixfmt):
    """The sample type of a planar RGB format (PIX_RGBP8 / RGBP10 / RGBPH / RGBPF); ValueError for anything else (a colour description included)."""
    if pixfmt not in _RGBP_DTYPE:
        raise ValueError("%r is not a planar RGB pixfmt" % (pixfmt,))
    return _RGBP_DTYPE[pixfmt]


_PIX_LAYOUT = {PIX_RGB8: (np.uint8, 3), PIX_RGB10_U16: (np.uint16, 3), PIX_A2B10G10R10: (np.uint32, 2), PIX_RGBA8: (np.uint8, 3)}      # dtype, ndim
_PIX_NAME = {PIX_RGB10_U16: "RGB10_U16", PIX_A2B10G10R10: "A2B10G10R10", PIX_RGBA8: "RGBA8"}


def _pix_shape(pixfmt, h, w):
    return (h, w) if pixfmt == PIX_A2B10G10R10 else (h, w, 4) if pixfmt == PIX_RGBA8 else (h, w, 3)


def _pix_of(image, pixfmt=None):
    """The pixel format of a frame array: a uint16 (h, w, 3) array is RGB10_U16, a uint32 (h, w) array A2B10G10R10, a uint8 (h, w, 4) array RGBA8; None =
    none of them (the 8-bit RGB path, which converts whatever it is given to uint8 as it always did).  An explicit `pixfmt` must match the array exactly.
    Raises before any library call."""
    a = image
    if pixfmt is None:
        if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4:
            pixfmt = PIX_RGBA8
        elif not isinstance(a, np.ndarray) or a.dtype not in (np.uint16, np.uint32):
            return None
        else:
            pixfmt = PIX_RGB10_U16 if a.dtype == np.uint16 else PIX_A2B10G10R10
    if pixfmt not in _PIX_LAYOUT:
        raise ValueError("unknown pixfmt %r" % (pixfmt,))
    if pixfmt == PIX_RGB8:
        return None
    dt, nd = _PIX_LAYOUT[pixfmt]
    nch = 4 if pixfmt == PIX_RGBA8 else 3
    if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != nd or (nd == 3 and a.shape[2] != nch) or a.size == 0:
        raise ValueError("a %s frame is a %s array of shape %s" % (_PIX_NAME[pixfmt], np.dtype(dt).name, "(h, w, %d)" % nch if nd == 3 else "(h, w)"))
    return pixfmt


_ELEM = {PIX_RGB8: 1, PIX_RGB10_U16: 2, PIX_A2B10G10R10: 4, PIX_RGBA8: 1, PIX_NV12: 1, PIX_I420: 1, PIX_P010: 2, PIX_I420P10: 2,
         PIX_I422: 1, PIX_I422P10: 2, PIX_I444: 1, PIX_I444P10: 2, PIX_RGBP8: 1, PIX_RGBP10: 2, PIX_RGBPH: 2, PIX_RGBPF: 4}


def image_row_bytes(w, pixfmt, plane):
    """rife_hip_image_row_bytes: bytes of one row of that plane of a frame w pixels wide (0 for a plane the format does not have)."""
    return int(lib().rife_hip_image_row_bytes(int(w), int(pixfmt), int(plane)))


def image_check(img):
    """rife_hip_image_check (host only): raises RifeError with the fault."""
    _check(lib().rife_hip_image_check(ctypes.byref(img)), "image_check")


def device_image(w, h, pixfmt, planes):
    """A rife_hip_image from a list of (pointer, pitch in bytes) per plane - for process_device_image() (device pointers) or any of the C calls."""
    im = rife_hip_image(int(w), int(h), int(pixfmt))
    for i, (ptr, pitch) in enumerate(planes):
        im.plane[i] = int(ptr) or None
        im.pitch[i] = int(pitch)
    return im


def _rows_strided(a):
    """True if the pixels of each row of `a` are contiguous and the rows follow each other at a positive stride: what a crop big[y0:y1, x0:x1], an array with
    padded rows or a plane view of a video frame is.  (A one-row array has no row stride to speak of; its own width stands in.)"""
    if not isinstance(a, np.ndarray) or a.ndim not in (2, 3) or a.size == 0:
        return False
    inner = a.itemsize
    for n, st in zip(a.shape[:0:-1], a.strides[:0:-1]):
        if n > 1 and st != inner:
            return False
        inner *= n
    return a.shape[0] == 1 or a.strides[0] >= inner


def _pitch(a):
    return a.strides[0] if a.shape[0] > 1 else max(a.strides[0], a.itemsize * int(np.prod(a.shape[1:])))


def image_of(a, pixfmt=None):
    """The descriptor process() / upload() pass for a frame array WITHOUT copying it, or None where they fall back to a contiguous copy as they always did:
    an RGB-format array ((h, w, 3) uint8 / uint16, (h, w) uint32, (h, w, 4) uint8) whose rows are strided but whose pixels are contiguous, with a pitch and a
    base address the format's element size divides."""
    px = _pix_of(a, pixfmt)
    if px is None:
        px = PIX_RGB8
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            return None
    if not _rows_strided(a):
        return None
    pitch = _pitch(a)
    if pitch % _ELEM[px] or a.ctypes.data % _ELEM[px] or pitch > 0x7fffffff:
        return None
    im = device_image(a.shape[1], a.shape[0], px, [(a.ctypes.data, pitch)])
    im._keep = a      # the descriptor holds raw addresses: the array lives as long as it does
    return im


def planes_image(planes, w, h, pixfmt, what="planes", writable=False):
    """The descriptor of a YUV frame given as a tuple of 2-D arrays, each with its own base and row stride: (h, w) luma and, cw, ch = yuv_chroma_dims(w, h, pixfmt),
    one (ch, 2 * cw) array of interleaved pairs (NV12, P010) or two (ch, cw) arrays Cb, Cr (I420, I422, I444 and their P10 forms; swap them for YV12 / YV16 /
    YV24).  Planar RGB (PIX_RGBP8 / RGBP10 / RGBPH / RGBPF): three (h, w) arrays R, G, B of planar_rgb_dtype(pixfmt) (permute them for ffmpeg's G, B, R order), or one
    (3, h, w) array.  Raises ValueError."""
    if pixfmt in _RGBP_DTYPE:
        dt = planar_rgb_dtype(pixfmt)
        shapes = [(h, w)] * 3
        if isinstance(planes, np.ndarray) and planes.ndim == 3:
            planes = tuple(planes)
    else:
        base = _yuv_base(pixfmt)
        dt = yuv_dtype(pixfmt)
        cw, ch = yuv_chroma_dims(w, h, pixfmt)
        shapes = [(h, w), (ch, 2 * cw)] if base in (PIX_NV12, PIX_P010) else [(h, w), (ch, cw), (ch, cw)]
    if w <= 0 or h <= 0 or len(planes) != len(shapes):
        raise ValueError("%s: %d arrays of shapes %s" % (what, len(shapes), shapes))
    for a, shp in zip(planes, shapes):
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shp or not _rows_strided(a) or (writable and not a.flags.writeable):
            raise ValueError("%s: each plane is a%s %s array of shape %s whose rows are contiguous" % (what, " writable" if writable else "", np.dtype(dt).name, shp))
    im = device_image(w, h, pixfmt, [(a.ctypes.data, _pitch(a)) for a in planes])
    im._keep = tuple(planes)
    return im


def hbd_check(img, depth):
    """rife_hip_hbd_check (host only): raises RifeError with the fault of the high-bit-depth image `img` (a rife_hip_image of u16 planes: planes_image() with
    PIX_I420P10 / I422P10 / I444P10 / RGBP10, or device_image()) whose samples carry `depth` bits, 10..16."""
    _check(lib().rife_hip_hbd_check(ctypes.byref(img) if img is not None else None, int(depth)), "hbd_check")


def packed_desc(w, h, channels, depth, data, pitch):
    """A rife_hip_packed from a raw address (int; device memory for process_device_hbd_packed(), or any of the C calls) and a pitch in bytes."""
    return rife_hip_packed(int(w), int(h), int(channels), int(depth), int(data) or None, int(pitch))


def packed_of(arr, depth, what="frame", writable=False):
    """The descriptor of a packed 16-bit frame WITHOUT copying it: an (h, w, 3 | 4) uint16 array of `depth`-bit samples whose last two axes are contiguous - a tight
    array, a crop or an array with padded rows.  Raises ValueError."""
    if (not isinstance(arr, np.ndarray) or arr.dtype != np.uint16 or arr.ndim != 3 or arr.shape[2] not in (3, 4) or arr.size == 0 or not _rows_strided(arr)
            or (writable and not arr.flags.writeable)):
        raise ValueError("%s: a%s uint16 array of shape (h, w, 3) or (h, w, 4) whose last two axes are contiguous" % (what, " writable" if writable else ""))
    d = packed_desc(arr.shape[1], arr.shape[0], arr.shape[2], depth, arr.ctypes.data, _pitch(arr))
    d._keep = arr      # the descriptor holds a raw address: the array lives as long as it does
    return d


def packed_check(arr, depth):
    """rife_hip_packed_check (host only): raises RifeError with the fault of the packed frame `arr` - an (h, w, 3 | 4) uint16 array as packed_of() takes it, or a
    rife_hip_packed descriptor (packed_desc()) - whose samples carry `depth` bits, 10..16."""
    d = arr if isinstance(arr, rife_hip_packed) or arr is None else packed_of(arr, depth)
    _check(lib().rife_hip_packed_check(ctypes.byref(d) if d is not None else None), "packed_check")


def semiplanar_desc(w, h, chroma, depth, y, pitch_y, cbcr, pitch_c, csp=0):
    """A rife_hip_semiplanar from raw addresses (ints; device memory for process_device_hbd_semiplanar(), or any of the C calls) and pitches in bytes."""
    return rife_hip_semiplanar(int(w), int(h), int(chroma), int(csp), int(depth), int(y) or None, int(pitch_y), int(cbcr) or None, int(pitch_c))


def semiplanar_of(y, cbcr, depth, chroma, csp=0, what="surface", writable=False):
    """The descriptor of a semi-planar surface WITHOUT copying it: an (h, w) uint16 luma array and a (ch, 2 * cw) uint16 array of interleaved Cb, Cr pairs (cw = (w + 1)
    // 2; ch = (h + 1) // 2 for chroma 1, h for chroma 2), `depth`-bit codes in the HIGH bits, rows contiguous - tight arrays, crops or arrays with padded rows.  Raises
    ValueError."""
    ok = all(isinstance(a, np.ndarray) and a.dtype == np.uint16 and a.ndim == 2 and a.size > 0 and _rows_strided(a) and (not writable or a.flags.writeable) for a in (y, cbcr))
    if ok:
        h, w = y.shape
        ok = chroma in (1, 2) and cbcr.shape == ((h + 1) // 2 if chroma == 1 else h, 2 * ((w + 1) // 2))
    if not ok:
        raise ValueError("%s: a%s uint16 array of shape (h, w) and one of shape (ch, 2 * cw) whose rows are contiguous, chroma 1 (ch = (h + 1) // 2) or 2 (ch = h)"
                         % (what, " writable" if writable else ""))
    d = semiplanar_desc(w, h, chroma, depth, y.ctypes.data, _pitch(y), cbcr.ctypes.data, _pitch(cbcr), csp)
    d._keep = (y, cbcr)      # the descriptor holds raw addresses: the arrays live as long as it does
    return d


def semiplanar_check(y, cbcr=None, w=None, h=None, chroma=1, depth=10, csp=0):
    """rife_hip_semiplanar_check (host only): raises RifeError with the fault of a semi-planar surface - two uint16 arrays as semiplanar_of() takes them (w, h, when
    given, must be their size), or a rife_hip_semiplanar descriptor (semiplanar_desc()) as the only argument."""
    if isinstance(y, rife_hip_semiplanar) or y is None:
        d = y
    else:
        d = semiplanar_of(y, cbcr, depth, chroma, csp)
        if (w is not None and int(w) != d.w) or (h is not None and int(h) != d.h):
            raise ValueError("surface: the luma array is not (h, w) = (%s, %s)" % (h, w))
    _check(lib().rife_hip_semiplanar_check(ctypes.byref(d) if d is not None else None), "semiplanar_check")


def _plane_tuple(planes):
    """A (3, h, w) array stands for its three planes."""
    return tuple(planes) if isinstance(planes, np.ndarray) and planes.ndim == 3 else planes


def motion_desc(flow=None, mask=None, fmt=MOTION_F32, flow_pitch=0, mask_pitch=0):
    """A rife_hip_motion from raw addresses (ints; None or 0 = not wanted) and pitches in bytes - device buffers for process_device_motion(), or any of the C calls."""
    return rife_hip_motion(int(flow) if flow else None, int(flow_pitch), int(mask) if mask else None, int(mask_pitch), int(fmt))


def motion_check(m, w, h):
    """rife_hip_motion_check (host only): raises RifeError with the fault."""
    _check(lib().rife_hip_motion_check(ctypes.byref(m), int(w), int(h)), "motion_check")


def _motion_host(w, h, dtype, flow, mask):
    """The descriptor of a host motion call and the arrays it fills.  flow / mask: None = a new (h, w, 4) / (h, w) array of `dtype`; False = not wanted; an array
    or view of that shape and dtype whose rows are strided but whose pixels are contiguous (row-padded arrays, crops) is written in place, without a copy."""
    dt = np.dtype(dtype)
    fmt = {np.dtype(np.float32): MOTION_F32, np.dtype(np.float16): MOTION_F16}.get(dt)
    if fmt is None:
        raise ValueError("the motion dtype is np.float32 or np.float16")
    out = []
    for a, shape, what in ((flow, (h, w, 4), "flow"), (mask, (h, w), "mask")):
        if a is None:
            a = np.empty(shape, dt)
        elif a is False:
            out.append(None)
            continue
        if not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != dt or not a.flags.writeable or not _rows_strided(a):
            raise ValueError("%s must be a writable %s array of shape %s whose rows are contiguous" % (what, dt.name, shape))
        out.append(a)
    f, m = out
    if f is None and m is None:
        raise ValueError("flow and mask are both unwanted")
    d = motion_desc(f.ctypes.data if f is not None else None, m.ctypes.data if m is not None else None, fmt, _pitch(f) if f is not None else 0, _pitch(m) if m is not None else 0)
    d._keep = (f, m)
    return d, f, m


def planes_desc(w, h, sample, planes, maxval=None):
    """A rife_hip_planes from raw addresses: planes = [(address, pitch in bytes), ...] (1..4), device or host.  maxval: None = the sample type's maximum (0 for the
    float types)."""
    if maxval is None:
        maxval = {SAMPLE_U8: 255, SAMPLE_U16: 65535}.get(sample, 0)
    d = rife_hip_planes()
    d.w, d.h, d.n, d.sample, d.maxval = int(w), int(h), len(planes), int(sample), int(maxval)
    for i, (ptr, pitch) in enumerate(planes[:4]):
        d.plane[i] = int(ptr) if ptr else None
        d.pitch[i] = int(pitch)
    return d


def planes_check(d):
    """rife_hip_planes_check (host only): raises RifeError with the fault."""
    _check(lib().rife_hip_planes_check(ctypes.byref(d)), "planes_check")


def planes_of(planes, maxval=None, what="planes", writable=False):
    """The descriptor of host planes WITHOUT copying them: a tuple of 1..4 2-D arrays of one shape and dtype (uint8, uint16, float16, float32), or one (n, h, w) array;
    row-padded arrays and views whose pixels are contiguous are taken as they are.  The dtype selects the sample type.  Raises ValueError."""
    if isinstance(planes, np.ndarray) and planes.ndim == 3:
        planes = tuple(planes)
    elif isinstance(planes, np.ndarray) and planes.ndim == 2:
        planes = (planes,)
    planes = tuple(planes)
    if not 1 <= len(planes) <= 4 or not all(isinstance(a, np.ndarray) and a.ndim == 2 and a.size for a in planes):
        raise ValueError("%s: 1..4 two-dimensional arrays, or one (n, h, w) array" % what)
    a0 = planes[0]
    sample = _SAMPLE_OF.get(a0.dtype)
    if sample is None:
        raise ValueError("%s: the dtype is uint8, uint16, float16 or float32" % what)
    for a in planes:
        if a.dtype != a0.dtype or a.shape != a0.shape or not _rows_strided(a) or (writable and not a.flags.writeable):
            raise ValueError("%s: each plane is a%s %s array of shape %s whose rows are contiguous" % (what, " writable" if writable else "", a0.dtype.name, a0.shape))
    d = planes_desc(a0.shape[1], a0.shape[0], sample, [(a.ctypes.data, _pitch(a)) for a in planes], maxval)
    d._keep = planes
    return d


def _planes_out(like, out):
    """The output planes of an apply call: `out` (planes as for planes_of, written in place), or new tight arrays shaped like the input planes `like`."""
    if out is None:
        out = tuple(np.empty(a.shape, a.dtype) for a in like._keep)
    d = planes_of(out, like.maxval, "out", writable=True)
    return d, d._keep


def _motion_in(w, h, flow, mask):
    """The descriptor of host motion an apply call READS: flow (h, w, 4) and mask (h, w) of one dtype, float32 or float16; rows may be strided."""
    if not isinstance(flow, np.ndarray) or not isinstance(mask, np.ndarray) or flow.dtype != mask.dtype:
        raise ValueError("flow and mask are arrays of one dtype")
    fmt = {np.dtype(np.float32): MOTION_F32, np.dtype(np.float16): MOTION_F16}.get(flow.dtype)
    if fmt is None:
        raise ValueError("the motion dtype is np.float32 or np.float16")
    if flow.shape != (h, w, 4) or mask.shape != (h, w):
        raise ValueError("flow is (h, w, 4) and mask (h, w) of the planes' size")
    if not _rows_strided(flow):
        flow = np.ascontiguousarray(flow)
    if not _rows_strided(mask):
        mask = np.ascontiguousarray(mask)
    d = motion_desc(flow.ctypes.data, mask.ctypes.data, fmt, _pitch(flow), _pitch(mask))
    d._keep = (flow, mask)
    return d


def _packed_pair(in0image, in1image, pixfmt):
    """The two frames of a host call as contiguous arrays and their pixel format: (h, w, 3) uint8 by default, else a packed RGB format as process_motion() takes it."""
    px = _pix_of(in0image, pixfmt)
    if px is None:
        a = np.ascontiguousarray(in0image, dtype=np.uint8); b = np.ascontiguousarray(in1image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
            raise ValueError("frames must be (h, w, 3) uint8 arrays of equal size")
        return a, b, PIX_RGB8
    if _pix_of(in1image, px) != px or in1image.shape != in0image.shape:
        raise ValueError("both frames must have the same pixel format and size")
    return np.ascontiguousarray(in0image), np.ascontiguousarray(in1image), px


def apply_set_desc(planes0, planes1, planes_out, shift=(0, 0), extent=None):
    """A rife_hip_apply_set from three rife_hip_planes descriptors (planes_desc() for device planes, planes_of() for host planes): shift = the planes relative to the
    motion per axis, (0, 0), (-1, -1) 4:2:0 chroma, (-1, 0) 4:2:2 chroma or (1, 1) proxy upscaling; extent = (wp, hp) in the planes' own pixels, None = the plane size."""
    wp, hp = extent if extent is not None else (0, 0)
    s = rife_hip_apply_set(ctypes.pointer(planes0), ctypes.pointer(planes1), ctypes.pointer(planes_out), int(shift[0]), int(shift[1]), int(wp), int(hp))
    s._keep = (planes0, planes1, planes_out)
    return s


def apply_set(planes0, planes1, shift=(0, 0), maxval=None, extent=None, out=None):
    """One set of a sets call over HOST planes, as planes_of takes them (include/rife_hip.h "apply motion at another resolution"); out: planes to fill in place, None =
    new tight arrays.  The output planes are `.planes` of the set."""
    d0 = planes_of(planes0, maxval, "planes0"); d1 = planes_of(planes1, maxval, "planes1")
    do, res = _planes_out(d0, out)
    s = apply_set_desc(d0, d1, do, shift, extent)
    s.planes = res
    return s


def apply_set_check(s, mw, mh):
    """rife_hip_apply_set_check (host only): raises RifeError with the fault of set `s` against a motion of mw x mh."""
    _check(lib().rife_hip_apply_set_check(ctypes.byref(s), int(mw), int(mh)), "apply_set_check")


def _set_array(sets):
    """1..n rife_hip_apply_set -> a C array (the count is checked by the library)."""
    sets = list(sets)
    arr = (rife_hip_apply_set * max(len(sets), 1))()
    for k, s in enumerate(sets):
        ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(s), ctypes.sizeof(rife_hip_apply_set))
    arr._keep = sets
    return len(sets), arr


class Frame:
    """A frame resident in device memory (rife_hip_frame_t): upload once, use as either side of any number of pairs."""

    def __init__(self, handle, w, h, L=None, pixfmt=PIX_RGB8):
        self._f, self.w, self.h, self._L, self.pixfmt = handle, w, h, L or lib(), pixfmt

    def release(self):
        if getattr(self, "_f", None) and getattr(self, "_L", None) is not None:
            self._L.rife_hip_frame_release(self._f)
        self._f = None

    __del__ = release


class RIFE:
    """Same constructor arguments, in the same order, as the reference's `RIFE` (src/rife.h:14)."""

    def __init__(self, gpuid, tta_mode=False, tta_temporal_mode=False, uhd_mode=False, num_threads=1, rife_v2=False, rife_v4=False, test_build=False):
        # test_build (not a reference argument): the engine lives in librife_hip_test.so - parity taps (v4_*) and kernel-selection switches
        self._L = testlib() if test_build else lib()
        self._taps = test_build or hasattr(self._L, "rife_hip_v4_tap")
        self._h = self._L.rife_hip_create(int(gpuid), int(tta_mode), int(tta_temporal_mode), int(uhd_mode), int(num_threads),
                                          int(rife_v2), int(rife_v4))
        if not self._h:
            raise RifeError("rife_hip_create: " + self._L.rife_hip_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_L", None) is not None:       # at interpreter shutdown the module globals may be gone already
            try:
                self._L.rife_hip_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def load(self, modeldir):
        _check(self._L.rife_hip_load(self._h, os.fspath(modeldir).encode()), "load", self._L)
        return 0

    def set_flow_scale(self, divisor):
        """Estimate flow at 1 / divisor of the usual resolution (include/rife_hip.h: 1 = the reference's graph, 2 = every IFBlock at half resolution, frames
        padded to 64n; rife-v4.6, plain mode - for UHD material).  Call after load() and while no call on the engine is in flight.  A refusal raises
        RifeError with the C code (-1 bad divisor / before load, -6 another family or -x / -z) and leaves the engine unchanged."""
        _check(self._L.rife_hip_set_flow_scale(self._h, int(divisor)), "set_flow_scale", self._L)
        return 0

    @property
    def flow_scale(self):
        """The flow scale divisor in force."""
        return int(self._L.rife_hip_flow_scale(self._h))

    def set_precision(self, precision):
        """"full" / PRECISION_FULL (the default: fp32-equivalent residual trunks) or "fast" / PRECISION_FAST (include/rife_hip.h: one f16 product per weight tap of
        the trunk convolutions, the skip connection at full precision; rife-v4.6, plain mode).  Call after load() and while no call on the engine is in flight.
        Anything else is a ValueError; a refusal of the engine raises RifeError with the C code (-1 before load, -6 another family or -x / -z) and leaves the
        engine unchanged."""
        if isinstance(precision, str):
            if precision not in _PRECISION_NAMES:
                raise ValueError("precision must be 'full' or 'fast' (or PRECISION_FULL / PRECISION_FAST), not %r" % (precision,))
            value = _PRECISION_NAMES[precision]
        elif isinstance(precision, (bool, float)) or not isinstance(precision, (int, np.integer)) or int(precision) not in (PRECISION_FULL, PRECISION_FAST):
            raise ValueError("precision must be 'full' or 'fast' (or PRECISION_FULL / PRECISION_FAST), not %r" % (precision,))
        else:
            value = int(precision)
        _check(self._L.rife_hip_set_precision(self._h, value), "set_precision", self._L)
        return 0

    @property
    def precision(self):
        """The precision in force: PRECISION_FULL or PRECISION_FAST."""
        return int(self._L.rife_hip_precision(self._h))

    def process(self, in0image, in1image, timestep, outimage=None, pixfmt=None):
        """in0image / in1image: (h, w, 3) uint8 RGB arrays (the ncnn::Mat the CLI builds, src/main.cpp:187).
        Deep colour (rife-v4.6, plain mode): (h, w, 3) uint16 arrays of codes 0..1023 (RGB10_U16) or (h, w) uint32 arrays (A2B10G10R10), selected by the
        arrays' dtype or by pixfmt=; the result has the inputs' format.
        Alpha (rife-v4.6, plain mode): (h, w, 4) uint8 RGBA arrays (RGBA8); the colour bytes are those of the RGB call, alpha is warped and blended with it."""
        px = _pix_of(in0image, pixfmt)
        strided = self._strided(in0image, in1image, outimage, px)
        if strided is not None:
            done = strided(float(timestep))
            if done is not None:
                return done      # else: this engine does not serve strided images (another family, -x / -z / -u) and wrote nothing - the contiguous copies below, as ever
        if px is not None:
            if _pix_of(in1image, px) != px or in1image.shape != in0image.shape:
                raise ValueError("both frames must have the same pixel format and size")
            a = np.ascontiguousarray(in0image); b = np.ascontiguousarray(in1image)
            h, w = a.shape[:2]
            out = outimage if outimage is not None else np.empty_like(a)
            if not isinstance(out, np.ndarray) or out.shape != a.shape or out.dtype != a.dtype or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("outimage must be a writable contiguous array of the frames' dtype and shape")
            _check(self._L.rife_hip_process_px(self._h, _p(a), _p(b), w, h, float(timestep), _p(out), px), "process_px", self._L)
            return out
        a = np.ascontiguousarray(in0image, dtype=np.uint8)
        b = np.ascontiguousarray(in1image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
            raise ValueError("frames must be (h, w, 3) uint8 arrays of equal size")
        h, w, _ = a.shape
        out = outimage if outimage is not None else np.empty_like(a)
        if not isinstance(out, np.ndarray) or out.shape != a.shape or out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("outimage must be a writable contiguous (h, w, 3) uint8 array of the frames' size")
        _check(self._L.rife_hip_process(self._h, _p(a), _p(b), w, h, float(timestep), _p(out)), "process", self._L)
        return out

    def _strided(self, in0image, in1image, outimage, px):
        """process() without a copy: some frame of the call is not contiguous, and every one of them is an array whose rows are strided but whose pixels are
        contiguous (image_of) of one format and size.  Returns the call to make, or None: today's path (contiguous copies)."""
        arrs = [in0image, in1image] + ([outimage] if outimage is not None else [])
        if not all(isinstance(x, np.ndarray) for x in arrs) or all(x.flags.c_contiguous for x in arrs):
            return None
        if any(x.shape != in0image.shape or x.dtype != in0image.dtype for x in arrs) or (outimage is not None and not outimage.flags.writeable):
            return None
        imgs = [image_of(x, px) for x in arrs]
        if any(im is None for im in imgs):
            return None
        out = outimage if outimage is not None else np.empty(in0image.shape, in0image.dtype)
        if outimage is None:
            imgs.append(image_of(out, px))

        def call(timestep):
            rc = self._L.rife_hip_process_image(self._h, ctypes.byref(imgs[0]), ctypes.byref(imgs[1]), timestep, ctypes.byref(imgs[2]))
            if rc == -ENOSYS:      # refused before anything was written (include/rife_hip.h): the caller falls back
                return None
            _check(rc, "process_image", self._L)
            return out
        return call

    def process_planes(self, planes0, planes1, timestep, pixfmt, out=None):
        """YUV or planar RGB frames as tuples of 2-D plane arrays, each with its own base and row stride (what VapourSynth's plane views or an AVFrame's data /
        linesize are; shapes: planes_image()).  Nothing is repacked on the host.  out: a tuple of writable plane arrays to fill, or None; returns the output planes.
        A planar RGB frame may also be one (3, h, w) array (it is passed as tuple(a))."""
        planes0, planes1 = _plane_tuple(planes0), _plane_tuple(planes1)
        if out is not None:
            out = _plane_tuple(out)
        h, w = planes0[0].shape if len(planes0) and isinstance(planes0[0], np.ndarray) and planes0[0].ndim == 2 else (0, 0)
        a = planes_image(planes0, w, h, pixfmt, "planes0"); b = planes_image(planes1, w, h, pixfmt, "planes1")
        if out is None:
            out = tuple(np.empty(p.shape, p.dtype) for p in planes0)
        o = planes_image(out, w, h, pixfmt, "out", writable=True)
        _check(self._L.rife_hip_process_image(self._h, ctypes.byref(a), ctypes.byref(b), float(timestep), ctypes.byref(o)), "process_image", self._L)
        return tuple(out)

    def upload_planes(self, planes, pixfmt):
        """Stream mode for a YUV or planar RGB frame given as plane arrays (process_planes); the resident frame is that of the _px upload of the packed frame.
        process_frames() on planar RGB frames returns a (3, h, w) array."""
        planes = _plane_tuple(planes)
        h, w = planes[0].shape if len(planes) and isinstance(planes[0], np.ndarray) and planes[0].ndim == 2 else (0, 0)
        a = planes_image(planes, w, h, pixfmt, "planes")
        f = ctypes.c_void_p()
        _check(self._L.rife_hip_frame_upload_image(self._h, ctypes.byref(a), ctypes.byref(f)), "frame_upload_image", self._L)
        return Frame(f, int(w), int(h), self._L, int(pixfmt))

    def process_frames_image(self, frame0, frame1, timestep, out):
        """process_frames() into a strided result: `out` is a rife_hip_image (image_of / planes_image / device_image on HOST memory) of the frames' size and format."""
        if frame0._f is None or frame1._f is None:
            raise ValueError("frame was released")
        _check(self._L.rife_hip_process_frames_image(self._h, frame0._f, frame1._f, float(timestep), ctypes.byref(out)), "process_frames_image", self._L)

    def process_device_image(self, img0, img1, timestep, out, stream=None):
        """rife_hip_process_device_image: three rife_hip_image descriptors of DEVICE planes (device_image(w, h, pixfmt, [(ptr, pitch), ...])), read and written in
        place by the pitched kernels; enqueues on `stream` (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        _check(self._L.rife_hip_process_device_image(self._h, ctypes.byref(img0), ctypes.byref(img1), float(timestep), ctypes.byref(out), stream), "process_device_image", self._L)

    def process_yuv(self, buf0, buf1, w, h, timestep, pixfmt, out=None):
        """YUV frames in and out (rife-v4.6, plain mode): flat uint8 (NV12, I420, I422, I444) or uint16 (P010, I420P10, I422P10, I444P10) arrays of
        yuv_frame_bytes(w, h, pixfmt) bytes; pixfmt = PIX_NV12 .. PIX_I444P10, OR-ed with CSP_BT709 / CSP_BT601 / CSP_BT2020NCL and CSP_FULL.  The result has the inputs' format."""
        a = _yuv_buf(buf0, w, h, pixfmt, "buf0"); b = _yuv_buf(buf1, w, h, pixfmt, "buf1")
        o = _yuv_buf(out if out is not None else np.empty_like(a), w, h, pixfmt, "out")
        if not o.flags.writeable:
            raise ValueError("out must be writable")
        _check(self._L.rife_hip_process_px(self._h, _p(a), _p(b), int(w), int(h), float(timestep), _p(o), int(pixfmt)), "process_px", self._L)
        return o

    def upload_yuv(self, buf, w, h, pixfmt):
        """Stream mode for YUV frames: the frame stays in device memory in its own format and is converted at each use; process_frames() returns a flat array."""
        a = _yuv_buf(buf, w, h, pixfmt, "buf")
        f = ctypes.c_void_p()
        _check(self._L.rife_hip_frame_upload_px(self._h, _p(a), int(w), int(h), int(pixfmt), ctypes.byref(f)), "frame_upload_px", self._L)
        return Frame(f, int(w), int(h), self._L, int(pixfmt))

    def upload(self, image, pixfmt=None):
        """Stream mode: copy one (h, w, 3) uint8 frame to the device and keep it there (deep colour: a uint16 (h, w, 3) or uint32 (h, w)
        array, see process())."""
        px = _pix_of(image, pixfmt)
        im = image_of(image, px) if isinstance(image, np.ndarray) and not image.flags.c_contiguous else None
        if im is not None:      # rows strided, pixels contiguous: uploaded from where it lies
            f = ctypes.c_void_p()
            rc = self._L.rife_hip_frame_upload_image(self._h, ctypes.byref(im), ctypes.byref(f))
            if rc != -ENOSYS:      # -ENOSYS: an engine that does not serve strided images - the contiguous copy below, as ever
                _check(rc, "frame_upload_image", self._L)
                return Frame(f, im.w, im.h, self._L, im.pixfmt)
        if px is not None:
            a = np.ascontiguousarray(image)
            f = ctypes.c_void_p()
            _check(self._L.rife_hip_frame_upload_px(self._h, _p(a), a.shape[1], a.shape[0], px, ctypes.byref(f)), "frame_upload_px", self._L)
            return Frame(f, a.shape[1], a.shape[0], self._L, px)
        a = np.ascontiguousarray(image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("frame must be an (h, w, 3) uint8 array")
        f = ctypes.c_void_p()
        _check(self._L.rife_hip_frame_upload(self._h, _p(a), a.shape[1], a.shape[0], ctypes.byref(f)), "frame_upload", self._L)
        return Frame(f, a.shape[1], a.shape[0], self._L)

    def process_frames(self, frame0, frame1, timestep, outimage=None):
        """process() between two resident frames; same pixels as process() on the host arrays they were uploaded from."""
        if frame0._f is None or frame1._f is None:
            raise ValueError("frame was released")
        if frame0.pixfmt != frame1.pixfmt:
            raise ValueError("the two frames differ in pixel format")
        if frame0.pixfmt != PIX_RGB8:      # the result has the format the frames were uploaded in
            if frame0.pixfmt in _RGBP_DTYPE:
                dt = planar_rgb_dtype(frame0.pixfmt)
                shape = (3, frame0.h, frame0.w)
            elif (frame0.pixfmt & 0xff) >= PIX_NV12:
                dt = yuv_dtype(frame0.pixfmt)
                shape = (yuv_frame_bytes(frame0.w, frame0.h, frame0.pixfmt) // np.dtype(dt).itemsize,)
            else:
                dt, nd = _PIX_LAYOUT[frame0.pixfmt]
                shape = _pix_shape(frame0.pixfmt, frame0.h, frame0.w)
            out = outimage if outimage is not None else np.empty(shape, dt)
            if not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dt or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("outimage must be a writable contiguous array of the frames' format and size")
            _check(self._L.rife_hip_process_frames(self._h, frame0._f, frame1._f, float(timestep), _p(out)), "process_frames", self._L)
            return out
        out = outimage if outimage is not None else np.empty((frame0.h, frame0.w, 3), np.uint8)
        if out.shape != (frame0.h, frame0.w, 3) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("outimage must be a contiguous (h, w, 3) uint8 array of the frames' size")
        _check(self._L.rife_hip_process_frames(self._h, frame0._f, frame1._f, float(timestep), _p(out)), "process_frames", self._L)
        return out

    def process_motion(self, in0image, in1image, timestep, dtype=np.float32, outimage=None, pixfmt=None, flow=None, mask=None):
        """process() that also returns the motion the frame was made from (rife-v4.6, plain mode; include/rife_hip.h "motion export"): (frame, flow, mask) with
        flow (h, w, 4) = dx0, dy0, dx1, dy1 - output pixel (x, y) was sampled from frame 0 at (x + dx0, y + dy0) and from frame 1 at (x + dx1, y + dy1) - and
        mask (h, w) the weight of frame 0's warp.  dtype: np.float32 or np.float16 (the float32 value rounded to nearest even).  flow= / mask=: arrays to fill (row-padded
        arrays and views are written in place), or False for "not wanted" (None comes back in its place).  The frame is byte for byte process()'s."""
        px = _pix_of(in0image, pixfmt)
        if px is None:
            a = np.ascontiguousarray(in0image, dtype=np.uint8); b = np.ascontiguousarray(in1image, dtype=np.uint8)
            if a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
                raise ValueError("frames must be (h, w, 3) uint8 arrays of equal size")
            px = PIX_RGB8
        else:
            if _pix_of(in1image, px) != px or in1image.shape != in0image.shape:
                raise ValueError("both frames must have the same pixel format and size")
            a = np.ascontiguousarray(in0image); b = np.ascontiguousarray(in1image)
        h, w = a.shape[:2]
        out = outimage if outimage is not None else np.empty_like(a)
        if not isinstance(out, np.ndarray) or out.shape != a.shape or out.dtype != a.dtype or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("outimage must be a writable contiguous array of the frames' dtype and shape")
        d, f, m = _motion_host(w, h, dtype, flow, mask)
        _check(self._L.rife_hip_process_motion(self._h, _p(a), _p(b), w, h, float(timestep), _p(out), px, ctypes.byref(d)), "process_motion", self._L)
        return out, f, m

    def process_frames_motion(self, frame0, frame1, timestep, dtype=np.float32, outimage=None, flow=None, mask=None):
        """process_frames() with the motion: (frame, flow, mask) as process_motion() returns them, between two resident frames of a packed RGB format."""
        if frame0._f is None or frame1._f is None:
            raise ValueError("frame was released")
        if frame0.pixfmt != frame1.pixfmt or frame0.pixfmt not in _PIX_LAYOUT:
            raise ValueError("two frames of one packed RGB format")
        dt, _ = _PIX_LAYOUT[frame0.pixfmt]
        shape = _pix_shape(frame0.pixfmt, frame0.h, frame0.w)
        out = outimage if outimage is not None else np.empty(shape, dt)
        if not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dt or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("outimage must be a writable contiguous array of the frames' format and size")
        d, f, m = _motion_host(frame0.w, frame0.h, dtype, flow, mask)
        _check(self._L.rife_hip_process_frames_motion(self._h, frame0._f, frame1._f, float(timestep), _p(out), ctypes.byref(d)), "process_frames_motion", self._L)
        return out, f, m

    def process_device_motion(self, d_in0, d_in1, w, h, timestep, d_out, motion, stream=None, pixfmt=PIX_RGB8):
        """rife_hip_process_device_motion: device pointers (ints) to tight frames of `pixfmt` and a motion_desc() of DEVICE buffers with their pitches, written in
        place by the kernel that finishes the frame; enqueues on `stream` (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        _check(self._L.rife_hip_process_device_motion(self._h, d_in0, d_in1, int(w), int(h), float(timestep), d_out, int(pixfmt), ctypes.byref(motion), stream),
               "process_device_motion", self._L)

    def padded_size(self, w, h):
        """(wp, hp): the engine's padded frame size for frames of w x h at the flow scale in force - the extent of apply_motion's frame semantics."""
        wp, hp = ctypes.c_int(), ctypes.c_int()
        _check(self._L.rife_hip_padded_size(self._h, int(w), int(h), ctypes.byref(wp), ctypes.byref(hp)), "padded_size", self._L)
        return wp.value, hp.value

    def apply_motion(self, planes0, planes1, flow, mask, maxval=None, extent=None, out=None):
        """rife_hip_apply_motion (include/rife_hip.h "apply motion"): warp(planes0, flow[..., 0:2]) * mask + warp(planes1, flow[..., 2:4]) * (1 - mask) at fp32 on
        the caller's planes - a tuple of 2-D arrays or one (n, h, w) array of uint8 / uint16 / float16 / float32 (the dtype selects the sample type; row-padded arrays
        and views are taken without a copy).  flow (h, w, 4) and mask (h, w): float32 or float16, as process_motion() returns them.  maxval: integer samples, default
        the dtype's maximum.  extent: None or (w, h) = edge clamping; padded_size(w, h) = the engine's frame semantics.  Returns the tuple of output planes (out=:
        planes to fill in place).  Needs no loaded model."""
        d0 = planes_of(planes0, maxval, "planes0"); d1 = planes_of(planes1, maxval, "planes1")
        do, res = _planes_out(d0, out)
        m = _motion_in(d0.w, d0.h, flow, mask)
        wp, hp = extent if extent is not None else (0, 0)
        _check(self._L.rife_hip_apply_motion(self._h, ctypes.byref(d0), ctypes.byref(d1), ctypes.byref(m), int(wp), int(hp), ctypes.byref(do)), "apply_motion", self._L)
        return res

    def apply_device_motion(self, planes0, planes1, motion, planes_out, extent=None, stream=None):
        """rife_hip_apply_device_motion: planes_desc() descriptors of DEVICE planes and a motion_desc() of DEVICE buffers; one launch on `stream` (hipStream_t as int;
        None = a stream of the engine's, synchronised before returning)."""
        wp, hp = extent if extent is not None else (0, 0)
        _check(self._L.rife_hip_apply_device_motion(self._h, ctypes.byref(planes0), ctypes.byref(planes1), ctypes.byref(motion), int(wp), int(hp), ctypes.byref(planes_out), stream),
               "apply_device_motion", self._L)

    def process_apply(self, in0image, in1image, timestep, planes0, planes1, maxval=None, extent=None, out=None, outimage=None, pixfmt=None, want_frame=True):
        """rife_hip_process_apply: estimate the motion on the frames in0image / in1image (any packed RGB format, as process_motion()) and apply it to planes0 / planes1
        in the same pass, the motion staying in device memory: (frame, planes).  want_frame=False: the frame is not downloaded and None comes back in its place.
        Byte for byte process_motion() followed by apply_motion()."""
        px = _pix_of(in0image, pixfmt)
        if px is None:
            a = np.ascontiguousarray(in0image, dtype=np.uint8); b = np.ascontiguousarray(in1image, dtype=np.uint8)
            if a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
                raise ValueError("frames must be (h, w, 3) uint8 arrays of equal size")
            px = PIX_RGB8
        else:
            if _pix_of(in1image, px) != px or in1image.shape != in0image.shape:
                raise ValueError("both frames must have the same pixel format and size")
            a = np.ascontiguousarray(in0image); b = np.ascontiguousarray(in1image)
        h, w = a.shape[:2]
        frame = None
        if want_frame:
            frame = outimage if outimage is not None else np.empty_like(a)
            if not isinstance(frame, np.ndarray) or frame.shape != a.shape or frame.dtype != a.dtype or not frame.flags.c_contiguous or not frame.flags.writeable:
                raise ValueError("outimage must be a writable contiguous array of the frames' dtype and shape")
        d0 = planes_of(planes0, maxval, "planes0"); d1 = planes_of(planes1, maxval, "planes1")
        do, res = _planes_out(d0, out)
        wp, hp = extent if extent is not None else (0, 0)
        _check(self._L.rife_hip_process_apply(self._h, _p(a), _p(b), w, h, float(timestep), _p(frame), px, ctypes.byref(d0), ctypes.byref(d1), int(wp), int(hp), ctypes.byref(do)),
               "process_apply", self._L)
        return frame, res

    def process_device_apply(self, d_in0, d_in1, w, h, timestep, d_out, planes0, planes1, planes_out, extent=None, stream=None, pixfmt=PIX_RGB8):
        """rife_hip_process_device_apply: device pointers (ints) to tight frames of `pixfmt` and planes_desc() descriptors of DEVICE planes; enqueues on `stream`
        (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        wp, hp = extent if extent is not None else (0, 0)
        _check(self._L.rife_hip_process_device_apply(self._h, d_in0, d_in1, int(w), int(h), float(timestep), d_out, int(pixfmt), ctypes.byref(planes0), ctypes.byref(planes1),
                                                     int(wp), int(hp), ctypes.byref(planes_out), stream), "process_device_apply", self._L)

    def apply_motion_sets(self, sets, flow, mask):
        """rife_hip_apply_motion_sets (include/rife_hip.h "apply motion at another resolution"): one motion field flow (mh, mw, 4), mask (mh, mw), float32 or float16,
        applied to 1..4 apply_set()s whose planes are the motion's size, half of it (4:2:0 / 4:2:2 chroma) or twice it (proxy upscaling).  Returns the list of the
        sets' output plane tuples.  Needs no loaded model."""
        if not isinstance(mask, np.ndarray) or mask.ndim != 2:
            raise ValueError("mask is a (mh, mw) array")
        mh, mw = mask.shape
        m = _motion_in(mw, mh, flow, mask)
        n, arr = _set_array(sets)
        _check(self._L.rife_hip_apply_motion_sets(self._h, n, arr, ctypes.byref(m), mw, mh), "apply_motion_sets", self._L)
        return [s.planes for s in arr._keep]

    def apply_device_motion_sets(self, sets, motion, mw, mh, stream=None):
        """rife_hip_apply_device_motion_sets: apply_set_desc() sets over DEVICE planes and a motion_desc() of DEVICE buffers of mw x mh; one launch per set on `stream`
        (hipStream_t as int; None = a stream of the engine's, synchronised before returning)."""
        n, arr = _set_array(sets)
        _check(self._L.rife_hip_apply_device_motion_sets(self._h, n, arr, ctypes.byref(motion), int(mw), int(mh), stream), "apply_device_motion_sets", self._L)

    def process_apply_sets(self, in0image, in1image, timestep, sets, outimage=None, pixfmt=None, want_frame=True):
        """rife_hip_process_apply_sets: estimate the motion on the frames in0image / in1image (any packed RGB format, as process_motion()) and apply it to every
        apply_set() of `sets` in the same pass, the motion staying in device memory: (frame, [planes of each set]).  want_frame=False: the frame is not downloaded and
        None comes back in its place.  Byte for byte process_motion() followed by apply_motion_sets()."""
        a, b, px = _packed_pair(in0image, in1image, pixfmt)
        h, w = a.shape[:2]
        frame = None
        if want_frame:
            frame = outimage if outimage is not None else np.empty_like(a)
            if not isinstance(frame, np.ndarray) or frame.shape != a.shape or frame.dtype != a.dtype or not frame.flags.c_contiguous or not frame.flags.writeable:
                raise ValueError("outimage must be a writable contiguous array of the frames' dtype and shape")
        n, arr = _set_array(sets)
        _check(self._L.rife_hip_process_apply_sets(self._h, _p(a), _p(b), w, h, float(timestep), _p(frame), px, n, arr), "process_apply_sets", self._L)
        return frame, [s.planes for s in arr._keep]

    def process_device_apply_sets(self, d_in0, d_in1, w, h, timestep, d_out, sets, stream=None, pixfmt=PIX_RGB8):
        """rife_hip_process_device_apply_sets: device pointers (ints) to tight frames of `pixfmt` and apply_set_desc() sets over DEVICE planes; enqueues on `stream`
        (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        n, arr = _set_array(sets)
        _check(self._L.rife_hip_process_device_apply_sets(self._h, d_in0, d_in1, int(w), int(h), float(timestep), d_out, int(pixfmt), n, arr, stream),
               "process_device_apply_sets", self._L)

    def process_hbd(self, planes0, planes1, timestep, depth, pixfmt, out=None):
        """rife_hip_process_hbd (include/rife_hip.h "high bit depth"): planes of `depth`-bit samples (10..16, codes in the low bits of uint16) in the layout of
        pixfmt = PIX_I420P10 / PIX_I422P10 / PIX_I444P10 (OR-ed with CSP_*) or PIX_RGBP10, as process_planes() takes them - (h, w) and chroma-shaped arrays, views and
        row-padded arrays without a copy.  The motion is estimated on a ten-bit proxy made on the device and applied to the planes themselves.  out: a tuple of writable
        plane arrays to fill, or None; returns the output planes."""
        planes0, planes1 = _plane_tuple(planes0), _plane_tuple(planes1)
        if out is not None:
            out = _plane_tuple(out)
        h, w = planes0[0].shape if len(planes0) and isinstance(planes0[0], np.ndarray) and planes0[0].ndim == 2 else (0, 0)
        a = planes_image(planes0, w, h, pixfmt, "planes0"); b = planes_image(planes1, w, h, pixfmt, "planes1")
        if out is None:
            out = tuple(np.empty(p.shape, p.dtype) for p in planes0)
        o = planes_image(out, w, h, pixfmt, "out", writable=True)
        _check(self._L.rife_hip_process_hbd(self._h, ctypes.byref(a), ctypes.byref(b), float(timestep), ctypes.byref(o), int(depth)), "process_hbd", self._L)
        return tuple(out)

    def process_device_hbd(self, img0, img1, timestep, out, depth, stream=None):
        """rife_hip_process_device_hbd: three rife_hip_image descriptors of DEVICE planes (device_image(w, h, pixfmt, [(ptr, pitch), ...])) of `depth`-bit samples, read and
        written in place; enqueues on `stream` (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        _check(self._L.rife_hip_process_device_hbd(self._h, ctypes.byref(img0), ctypes.byref(img1), float(timestep), ctypes.byref(out), int(depth), stream),
               "process_device_hbd", self._L)

    def process_hbd_packed(self, in0, in1, timestep, depth, out=None):
        """rife_hip_process_hbd_packed (include/rife_hip.h "16-bit packed RGB and RGBA"): two (h, w, 3) or (h, w, 4) uint16 frames of `depth`-bit samples (10..16, codes
        in the low bits), R G B (A) interleaved; views and row-padded arrays are taken without a copy (the last two axes contiguous).  The motion is estimated on a
        ten-bit proxy of the colour channels made on the device and applied to all channels of the frames themselves.  out: a writable array to fill, or None;
        returns the output frame."""
        a = packed_of(in0, depth, "in0"); b = packed_of(in1, depth, "in1")
        if out is None:
            out = np.empty(in0.shape, np.uint16)
        o = packed_of(out, depth, "out", writable=True)
        _check(self._L.rife_hip_process_hbd_packed(self._h, ctypes.byref(a), ctypes.byref(b), float(timestep), ctypes.byref(o)), "process_hbd_packed", self._L)
        return out

    def process_device_hbd_packed(self, img0, img1, timestep, out, stream=None):
        """rife_hip_process_device_hbd_packed: three rife_hip_packed descriptors of DEVICE frames (packed_desc(w, h, channels, depth, ptr, pitch)), read and written in
        place; enqueues on `stream` (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        _check(self._L.rife_hip_process_device_hbd_packed(self._h, ctypes.byref(img0), ctypes.byref(img1), float(timestep), ctypes.byref(out), stream),
               "process_device_hbd_packed", self._L)

    def process_hbd_semiplanar(self, in0, in1, timestep, depth, chroma, csp=0, out=None):
        """rife_hip_process_hbd_semiplanar (include/rife_hip.h "semi-planar high bit depth"): two decoder surfaces (y, cbcr) - an (h, w) uint16 luma array and a
        (ch, 2 * cw) uint16 array of interleaved Cb, Cr pairs, `depth`-bit codes (10..16) in the HIGH bits; chroma 1 = 4:2:0 (P010 / P012 / P016), 2 = 4:2:2 (P210 /
        P212 / P216); views and row-padded arrays are taken without a copy.  The motion is estimated on a ten-bit proxy made on the device and applied to the surfaces
        themselves.  out: a (y, cbcr) pair of writable arrays to fill, or None; returns the output pair."""
        for name, s in (("in0", in0), ("in1", in1)) + ((("out", out),) if out is not None else ()):
            if not isinstance(s, (tuple, list)) or len(s) != 2:
                raise ValueError("%s: a pair (y, cbcr) of uint16 arrays" % name)
        a = semiplanar_of(in0[0], in0[1], depth, chroma, csp, "in0"); b = semiplanar_of(in1[0], in1[1], depth, chroma, csp, "in1")
        if out is None:
            out = (np.empty(in0[0].shape, np.uint16), np.empty(in0[1].shape, np.uint16))
        o = semiplanar_of(out[0], out[1], depth, chroma, csp, "out", writable=True)
        _check(self._L.rife_hip_process_hbd_semiplanar(self._h, ctypes.byref(a), ctypes.byref(b), float(timestep), ctypes.byref(o)), "process_hbd_semiplanar", self._L)
        return tuple(out)

    def process_device_hbd_semiplanar(self, img0, img1, timestep, out, stream=None):
        """rife_hip_process_device_hbd_semiplanar: three rife_hip_semiplanar descriptors of DEVICE surfaces (semiplanar_desc(w, h, chroma, depth, y, pitch_y, cbcr,
        pitch_c, csp)), read and written in place; enqueues on `stream` (hipStream_t as int; None = the engine's own stream, synchronised before returning)."""
        _check(self._L.rife_hip_process_device_hbd_semiplanar(self._h, ctypes.byref(img0), ctypes.byref(img1), float(timestep), ctypes.byref(out), stream),
               "process_device_hbd_semiplanar", self._L)

    def process_device(self, d_in0, d_in1, w, h, timestep, d_out, stream=None, pixfmt=PIX_RGB8):
        """Device pointers (ints) to tightly packed u8 HWC RGB frames (or frames of `pixfmt`); enqueues on `stream` (hipStream_t as int)."""
        if pixfmt not in _PIX_LAYOUT and pixfmt not in _RGBP_DTYPE:
            _yuv_base(pixfmt)
        if pixfmt != PIX_RGB8:
            _check(self._L.rife_hip_process_device_px(self._h, d_in0, d_in1, w, h, float(timestep), d_out, pixfmt, stream), "process_device_px", self._L)
            return
        _check(self._L.rife_hip_process_device(self._h, d_in0, d_in1, w, h, float(timestep), d_out, stream), "process_device", self._L)

    def stream_create(self, part, nparts):
        """A hipStream_t (int) that owns the compute units i with i % nparts == part (rife_hip_stream_create); for process_device."""
        st = ctypes.c_void_p()
        _check(self._L.rife_hip_stream_create(self._h, int(part), int(nparts), ctypes.byref(st)), "stream_create", self._L)
        return st.value

    def stream_destroy(self, stream):
        _check(self._L.rife_hip_stream_destroy(self._h, stream), "stream_destroy", self._L)

    def process_device_batch(self, d_in0, d_in1, w, h, timesteps, d_out, stream=None, pixfmt=PIX_RGB8):
        """n resident pairs in one call (rife_hip_process_device_batch): lists of device pointers; enqueued relative to `stream`."""
        if pixfmt not in _PIX_LAYOUT and pixfmt not in _RGBP_DTYPE:
            _yuv_base(pixfmt)
        n = len(d_in0)
        if len(d_in1) != n or len(d_out) != n or len(timesteps) != n:
            raise ValueError("one in1 / out / timestep per pair")
        pa = (ctypes.c_void_p * n)(*[int(x) for x in d_in0])
        pb = (ctypes.c_void_p * n)(*[int(x) for x in d_in1])
        po = (ctypes.c_void_p * n)(*[int(x) for x in d_out])
        ts = (ctypes.c_float * n)(*[float(t) for t in timesteps])
        if pixfmt != PIX_RGB8:
            _check(self._L.rife_hip_process_device_batch_px(self._h, n, pa, pb, ts, po, w, h, pixfmt, stream), "process_device_batch_px", self._L)
            return
        _check(self._L.rife_hip_process_device_batch(self._h, n, pa, pb, ts, po, w, h, stream), "process_device_batch", self._L)

    # ---- measurement / parity taps ----
    def process_batch(self, in0images, in1images, timesteps, outimages=None):
        """n independent pairs in one call (rife_hip_process_batch); returns the list of interpolated frames
        (`outimages`: optional preallocated (h, w, 3) uint8 arrays to write into)."""
        a = [np.ascontiguousarray(x, dtype=np.uint8) for x in in0images]
        b = [np.ascontiguousarray(x, dtype=np.uint8) for x in in1images]
        n = len(a)
        if n == 0:
            return []
        h, w, _ = a[0].shape
        if any(x.shape != (h, w, 3) for x in a + b) or len(b) != n or len(timesteps) != n:
            raise ValueError("all frames of a batch must share one size, and there must be one timestep per pair")
        outs = list(outimages) if outimages is not None else [np.empty((h, w, 3), np.uint8) for _ in range(n)]
        if len(outs) != n or any(o.shape != (h, w, 3) or o.dtype != np.uint8 or not o.flags.c_contiguous for o in outs):
            raise ValueError("outimages must be n contiguous (h, w, 3) uint8 arrays")
        pa = (ctypes.c_void_p * n)(*[x.ctypes.data for x in a])
        pb = (ctypes.c_void_p * n)(*[x.ctypes.data for x in b])
        po = (ctypes.c_void_p * n)(*[x.ctypes.data for x in outs])
        ts = (ctypes.c_float * n)(*[float(t) for t in timesteps])
        _check(self._L.rife_hip_process_batch(self._h, n, pa, pb, ts, po, w, h), "process_batch", self._L)
        return outs

    def profile_enable(self, on=True):
        _check(self._L.rife_hip_profile_enable(self._h, int(on)), "profile_enable", self._L)

    def profile_read(self):
        names = ctypes.create_string_buffer(4096)
        ms = np.zeros(64, np.float64); n = np.zeros(64, np.int64); fl = np.zeros(64, np.float64)
        k = self._L.rife_hip_profile_read(self._h, names, 4096, _p(ms), _p(n), _p(fl), 64)
        nm = names.value.decode().split("\n")
        return {nm[i]: dict(ms=float(ms[i]), launches=int(n[i]), flops=float(fl[i])) for i in range(k)}

    def _need_taps(self):
        if not self._taps:
            raise RifeError("the parity taps (include/rife_hip_test.h) live in the test build: create the engine with amd.test_build().RIFE(...)")

    def pool_state(self):
        """(pooled, leased, high_water) of the workspace pool of the host-buffer entry points (test build; include/rife_hip_test.h)."""
        self._need_taps()
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self._L.rife_hip_pool_state(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "pool_state", self._L)
        return a.value, b.value, c.value

    def v4_extract_flow(self, in0image, in1image, timestep, fi, inject=(), pixfmt=None):
        self._need_taps()
        px = _pix_of(in0image, pixfmt)
        if px is not None and _pix_of(in1image, px) != px:
            raise ValueError("both frames must have the same pixel format")
        if px is not None:
            a = np.ascontiguousarray(in0image); b = np.ascontiguousarray(in1image)
        else:
            a = np.ascontiguousarray(in0image, dtype=np.uint8); b = np.ascontiguousarray(in1image, dtype=np.uint8)
        h, w = a.shape[:2]
        nc, fh, fw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self._L.rife_hip_v4_flow_dims(self._h, w, h, fi, ctypes.byref(nc), ctypes.byref(fh), ctypes.byref(fw)), "v4_flow_dims", self._L)
        out = np.empty((nc.value, fh.value, fw.value), np.float32)
        inj = [np.ascontiguousarray(f, dtype=np.float32) for f in inject]
        arr = (ctypes.c_void_p * max(1, len(inj)))(*[f.ctypes.data for f in inj])
        if px is not None:
            _check(self._L.rife_hip_v4_extract_flow_px(self._h, _p(a), _p(b), w, h, float(timestep), fi, arr, len(inj), _p(out), px), "v4_extract_flow_px", self._L)
            return out
        _check(self._L.rife_hip_v4_extract_flow(self._h, _p(a), _p(b), w, h, float(timestep), fi, arr, len(inj), _p(out)), "v4_extract_flow", self._L)
        return out


    def v4_tap(self, in0image, in1image, timestep, what, b, inject, pixfmt=None):
        """what 0 / 1: 12-channel input of IFBlock b (unfused kernel / through the fused stem kernel); 2: blob out0 before the postproc;
        4 / 3: F (4 channels) and M as block b's stem finds them, after k_flow_update / as written by the stem that applies the last update itself;
        5 (b = 3): the block input through the row-streaming stem kernel of the product;
        6 (b = 2, 3): F and M, (5, hp, wp), as k_flow_cascade<b> writes them from the b injected flows alone (4 is its sequential reference);
        7 (b = 0..3, RGB8): the first S16 trunk tensor of block b after the block's stems, raw: a uint8 array of op_s16_geom(C, hp / 4 s, wp / 4 s)[3] bytes.
        what = 0 with b = 0 and no blobs: the 7-channel input of block 0.  The buffers follow the flow scale in force (padded_size(), block scales 8, 4, 2, 1 times
        the divisor); at divisor 2 the library serves what = 0, 1, 4, 7 and refuses 2, 3, 5, 6 (kernels of the scale-1 schedule)."""
        self._need_taps()
        px = _pix_of(in0image, pixfmt)
        if px is not None and _pix_of(in1image, px) != px:
            raise ValueError("both frames must have the same pixel format")
        if px is not None:
            a = np.ascontiguousarray(in0image); bb = np.ascontiguousarray(in1image)
        else:
            a = np.ascontiguousarray(in0image, dtype=np.uint8); bb = np.ascontiguousarray(in1image, dtype=np.uint8)
        h, w = a.shape[:2]
        wp, hp = self.padded_size(w, h)                              # 32n, flow scale 2: 64n
        s = (8, 4, 2, 1)[b if 0 <= b <= 3 else 3] * self.flow_scale     # the block's scale at the divisor in force
        if what == 7:
            C = (192, 128, 96, 64)[b]
            out = np.empty(op_s16_geom(C, hp // (4 * s), wp // (4 * s))[3], np.uint8)
        else:
            out = np.empty((4 if px == PIX_RGBA8 else 3, hp, wp) if what == 2 else (5, hp, wp) if what in (3, 4, 6) else (7 if b == 0 else 12, hp // s, wp // s), np.float32)
        inj = [np.ascontiguousarray(f, dtype=np.float32) for f in inject]
        arr = (ctypes.c_void_p * max(1, len(inj)))(*[f.ctypes.data for f in inj])
        if px is not None:
            _check(self._L.rife_hip_v4_tap_px(self._h, _p(a), _p(bb), w, h, float(timestep), int(what), int(b), arr, len(inj), _p(out), px), "v4_tap_px", self._L)
            return out
        _check(self._L.rife_hip_v4_tap(self._h, _p(a), _p(bb), w, h, float(timestep), int(what), int(b), arr, len(inj), _p(out)), "v4_tap", self._L)
        return out

    def v4_process_injected(self, in0image, in1image, timestep, inject, pixfmt=None):
        """The plain pass with the first len(inject) flow blobs injected.  pixfmt (an RGB format) or four blobs (flow scale 2): the _px form, which writes the
        frames' format."""
        self._need_taps()
        px = _pix_of(in0image, pixfmt)
        if px is not None or len(inject) > 3:
            a = np.ascontiguousarray(in0image); bb = np.ascontiguousarray(in1image)
            if a.shape != bb.shape or a.dtype != bb.dtype:
                raise ValueError("both frames must have the same pixel format and size")
            h, w = a.shape[:2]
            out = np.empty_like(a)
            inj = [np.ascontiguousarray(f, dtype=np.float32) for f in inject]
            arr = (ctypes.c_void_p * max(1, len(inj)))(*[f.ctypes.data for f in inj])
            _check(self._L.rife_hip_v4_process_injected_px(self._h, _p(a), _p(bb), w, h, float(timestep), arr, len(inj), _p(out), px or PIX_RGB8),
                   "v4_process_injected_px", self._L)
            return out
        a = np.ascontiguousarray(in0image, dtype=np.uint8); bb = np.ascontiguousarray(in1image, dtype=np.uint8)
        h, w, _ = a.shape
        out = np.empty((h, w, 3), np.uint8)
        inj = [np.ascontiguousarray(f, dtype=np.float32) for f in inject]
        arr = (ctypes.c_void_p * max(1, len(inj)))(*[f.ctypes.data for f in inj])
        _check(self._L.rife_hip_v4_process_injected(self._h, _p(a), _p(bb), w, h, float(timestep), arr, len(inj), _p(out)), "v4_process_injected", self._L)
        return out


# ---- single-kernel entry points (planar CHW float32 numpy arrays): include/rife_hip_test.h, test build ----
def op_conv3x3(x, weight, bias, stride=1, residual=None, slope=None, gpuid=0):
    x = np.ascontiguousarray(x, np.float32); weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    c, h, w = x.shape
    oc = weight.shape[0]
    out = np.empty((oc, (h - 1) // stride + 1, (w - 1) // stride + 1), np.float32)
    res = None if residual is None else np.ascontiguousarray(residual, np.float32)
    sl = None if slope is None else np.ascontiguousarray(slope, np.float32)
    _check(testlib().rife_hip_op_conv3x3(gpuid, _p(x), c, h, w, _p(weight), _p(bias), oc, stride, _p(res), _p(sl), _p(out)), "op_conv3x3", testlib())
    return out


def graph_plan(param_base):
    """rife_hip_graph_plan (host only): what the graph loader settled on for <param_base>.param, one dict per layer in file order -
    name, kind, fold (the layer that executes this one, or None), out (the blob its launch writes, or None), cls (a convolution's profile class, "direct", or None),
    padded (zero filters pad the output channels to a multiple of 4)."""
    buf = ctypes.create_string_buffer(1 << 20)
    _check(testlib().rife_hip_graph_plan(param_base.encode(), buf, len(buf)), "graph_plan", testlib())
    plan = []
    for line in buf.value.decode().splitlines():
        name, kind, *kv = line.split("\t")
        f = dict(x.split("=", 1) for x in kv)
        plan.append(dict(name=name, kind=kind, fold=None if f["fold"] == "-" else f["fold"], out=None if f["out"] == "-" else f["out"],
                         cls=None if f["class"] == "-" else f["class"], padded=f["padded"] == "1"))
    return plan


def graph_eval(param_base, inputs, wanted, keep=False, gpuid=0):
    """rife_hip_graph_eval: one graph_run of the generic executor on <param_base>.param / .bin.  inputs: {blob: (C, H, W) float32} (a (C, 1, 1) array becomes a
    vector blob); wanted: blob names.  Returns the wanted blobs as (C, H, W) float32 arrays.  keep: the net and its blob storage stay for the next call on the
    same files (include/rife_hip_test.h)."""
    names = list(inputs)
    arrs = [np.ascontiguousarray(inputs[n], np.float32) for n in names]
    if any(a.ndim != 3 for a in arrs):
        raise ValueError("bound blobs are (C, H, W) arrays")
    cn = (ctypes.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
    ca = (ctypes.c_void_p * max(1, len(names)))(*[a.ctypes.data for a in arrs])
    dims = np.array([a.shape for a in arrs], np.int32).reshape(-1)
    caps = [max([a.size for a in arrs] + [1 << 16]) * 64] * len(wanted)
    outs = [np.empty(c, np.float32) for c in caps]
    wn = (ctypes.c_char_p * len(wanted))(*[w.encode() for w in wanted])
    wa = (ctypes.c_void_p * len(wanted))(*[o.ctypes.data for o in outs])
    wc = (ctypes.c_size_t * len(wanted))(*caps)
    od = np.zeros(3 * len(wanted), np.int32)
    _check(testlib().rife_hip_graph_eval(gpuid, param_base.encode(), len(names), cn, ca, _p(dims), len(wanted), wn, wa, wc, _p(od), int(bool(keep))), "graph_eval", testlib())
    return [o[: c * h * w].reshape(c, h, w).copy() for o, (c, h, w) in zip(outs, od.reshape(-1, 3))]


def op_deconv4x4(x, weight, bias, slope=None, gpuid=0):
    x = np.ascontiguousarray(x, np.float32); weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    c, h, w = x.shape
    oc = weight.shape[0]
    out = np.empty((oc, 2 * h, 2 * w), np.float32)
    sl = None if slope is None else np.ascontiguousarray(slope, np.float32)
    _check(testlib().rife_hip_op_deconv4x4(gpuid, _p(x), c, h, w, _p(weight), _p(bias), oc, _p(sl), _p(out)), "op_deconv4x4", testlib())
    return out


def op_warp(image, flow, gpuid=0):
    image = np.ascontiguousarray(image, np.float32); flow = np.ascontiguousarray(flow, np.float32)
    c, h, w = image.shape
    out = np.empty_like(image)
    _check(testlib().rife_hip_op_warp(gpuid, _p(image), _p(flow), c, h, w, _p(out)), "op_warp", testlib())
    return out


def op_s16_geom(C, H, W):
    """(pitch, rows, plane_bytes, bytes) of the S16 tensor of a C x H x W trunk (csrc/engine_dispatch.h S16Geom); needs no device."""
    pitch, rows, plane, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint(), ctypes.c_size_t()
    _check(testlib().rife_hip_op_s16_geom(int(C), int(H), int(W), ctypes.byref(pitch), ctypes.byref(rows), ctypes.byref(plane), ctypes.byref(nbytes)), "op_s16_geom", testlib())
    return pitch.value, rows.value, plane.value, nbytes.value


def op_trunk(kernel, C, H, W, weight, bias, slope, in_s16, out_s16, flip=0, cus=0, gpuid=0, fast=False):
    """One (weight (C, C, 3, 3)) or two (weight (2, C, C, 3, 3)) residual trunk layers through ONE S16 kernel's own launcher (kernel = TRUNK_T64 .. TRUNK_KS) on
    raw S16 tensors: uint8 arrays of op_s16_geom(C, H, W)[3] bytes, or lists of up to four of them (the batched form of TRUNK_ROW / TRUNK_KS).  out_s16 goes to the
    device as given (what the kernel does not write comes back unchanged); returns the final tensor(s) as new arrays.  slope: one value per layer.
    fast: the launch goes through rife_hip_op_trunk_prec with PRECISION_FAST (the fast-precision instantiation of the kernel) or PRECISION_FULL (the bytes of
    rife_hip_op_trunk, which forwards to it)."""
    weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    n = 1 if weight.ndim == 4 else weight.shape[0]
    if weight.size != n * C * C * 9 or bias.size != n * C:
        raise ValueError("weight must be ([2,] C, C, 3, 3) and bias ([2,] C)")
    sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slope, np.float32), (n,)))
    single = isinstance(in_s16, np.ndarray)
    ins = [in_s16] if single else list(in_s16)
    outs = [out_s16] if single else list(out_s16)
    nbytes = op_s16_geom(C, H, W)[3]
    if len(ins) != len(outs) or not ins:
        raise ValueError("as many output tensors as input tensors, at least one")
    ins = [np.ascontiguousarray(a, np.uint8).reshape(-1) for a in ins]
    outs = [np.array(a, np.uint8).reshape(-1) for a in outs]      # copies: the call writes into them
    if any(a.size != nbytes for a in ins + outs):
        raise ValueError("an S16 tensor of this geometry has %d bytes" % nbytes)
    pi = (ctypes.c_void_p * len(ins))(*[a.ctypes.data for a in ins])
    po = (ctypes.c_void_p * len(outs))(*[a.ctypes.data for a in outs])
    _check(testlib().rife_hip_op_trunk_prec(gpuid, int(kernel), int(C), int(H), int(W), n, _p(weight), _p(bias), _p(sl), int(flip), int(cus), len(ins), pi, po,
                                            PRECISION_FAST if fast else PRECISION_FULL), "op_trunk", testlib())
    return outs[0] if single else outs


def op_stem1_s16(C, Ht, Wt, x, weight, bias, slope, out_s16, gpuid=0):
    """conv_h2s2_kernel<NS, true> alone: x (C / 2, 2 Ht, 2 Wt) fp32 -> the raw S16 tensor of a C x Ht x Wt trunk.  out_s16 (uint8, op_s16_geom(C, Ht, Wt)[3] bytes)
    goes to the device as given; returns the whole tensor after the launch as a new array."""
    x = np.ascontiguousarray(x, np.float32); weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    if x.shape != (C // 2, 2 * Ht, 2 * Wt) or weight.size != C * (C // 2) * 9 or bias.size != C:
        raise ValueError("x must be (C / 2, 2 Ht, 2 Wt), weight (C, C / 2, 3, 3) and bias (C)")
    out = np.array(out_s16, np.uint8).reshape(-1)      # a copy: the call writes into it
    if C % 16 == 0 and out.size != op_s16_geom(C, Ht, Wt)[3]:
        raise ValueError("an S16 tensor of this geometry has %d bytes" % op_s16_geom(C, Ht, Wt)[3])
    _check(testlib().rife_hip_op_stem1_s16(gpuid, int(C), int(Ht), int(Wt), _p(x), _p(weight), _p(bias), float(slope), _p(out)), "op_stem1_s16", testlib())
    return out


def op_head_ps(C, Ht, Wt, x, weight, bias, out8, gpuid=0):
    """head_h2_kernel<EPI_DECONV_PS, S16IN> alone.  x: a raw S16 tensor (uint8: S16IN = true) or (C, Ht, Wt) fp32 (S16IN = false).  out8 (8, 4 Ht, 4 Wt) fp32 is the
    flow tensor before the launch; returns all 8 planes after it as a new array."""
    s16 = isinstance(x, np.ndarray) and x.dtype == np.uint8
    x = np.ascontiguousarray(x) if s16 else np.ascontiguousarray(x, np.float32)
    weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    if weight.size != 24 * C * 16 or bias.size != 24 or (not s16 and x.shape != (C, Ht, Wt)):
        raise ValueError("x must be (C, Ht, Wt) or a raw S16 tensor, weight (24, C, 4, 4) and bias (24)")
    if s16 and C % 16 == 0 and x.size != op_s16_geom(C, Ht, Wt)[3]:
        raise ValueError("an S16 tensor of this geometry has %d bytes" % op_s16_geom(C, Ht, Wt)[3])
    out = np.array(out8, np.float32)                   # a copy: the call writes into it
    if out.shape != (8, 4 * Ht, 4 * Wt):
        raise ValueError("out8 must be (8, 4 Ht, 4 Wt)")
    _check(testlib().rife_hip_op_head_ps(gpuid, int(C), int(Ht), int(Wt), int(s16), _p(x), _p(weight), _p(bias), _p(out)), "op_head_ps", testlib())
    return out


def op_tail(kernel, pixfmt, w, h, trunk, weight, bias, F, M, img0, img1, out, cus=0, gpuid=0):
    """One of the kernels that write the quantised frame from block 3's last trunk tensor (kernel = TAIL_RS .. TAIL_UNFUSED), alone.  trunk: the raw S16 tensor
    (uint8) of a 64 x hp / 4 x wp / 4 trunk, for TAIL_HEAD_F32 (64, hp / 4, wp / 4) fp32; weight (24, 64, 4, 4), bias (24); F (hp, wp, 4), M (hp, wp) fp32; img0, img1
    (hp, wp) uint32 resident frames; out: uint8, TAIL_GUARD + frame bytes + TAIL_GUARD, goes to the device as given.  Returns the whole buffer after the launch as a
    new array."""
    wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32
    f32 = kernel == TAIL_HEAD_F32
    trunk = np.ascontiguousarray(trunk, np.float32) if f32 else np.ascontiguousarray(trunk, np.uint8).reshape(-1)
    weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    F = np.ascontiguousarray(F, np.float32); M = np.ascontiguousarray(M, np.float32)
    img0 = np.ascontiguousarray(img0, np.uint32); img1 = np.ascontiguousarray(img1, np.uint32)
    if weight.size != 24 * 64 * 16 or bias.size != 24 or F.shape != (hp, wp, 4) or M.shape != (hp, wp) or img0.shape != (hp, wp) or img1.shape != (hp, wp):
        raise ValueError("weight (24, 64, 4, 4), bias (24), F (hp, wp, 4), M (hp, wp) and two (hp, wp) uint32 frames")
    if trunk.size != (64 * (hp // 4) * (wp // 4) if f32 else op_s16_geom(64, hp // 4, wp // 4)[3]):
        raise ValueError("the trunk of this frame is 64 x %d x %d" % (hp // 4, wp // 4))
    bpp = {PIX_RGB8: 3, PIX_RGB10_U16: 6, PIX_A2B10G10R10: 4, PIX_RGBA8: 4}.get(pixfmt)
    buf = np.array(out, np.uint8).reshape(-1)          # a copy: the call writes into it
    if bpp is not None and buf.size != 2 * TAIL_GUARD + w * h * bpp:
        raise ValueError("out must hold %d bytes" % (2 * TAIL_GUARD + w * h * bpp))
    _check(testlib().rife_hip_op_tail(gpuid, int(kernel), int(pixfmt), int(w), int(h), _p(trunk), _p(weight), _p(bias), _p(F), _p(M), _p(img0), _p(img1), int(cus),
                                      _p(buf)), "op_tail", testlib())
    return buf


def op_tail_motion(kernel, pixfmt, w, h, trunk, weight, bias, F, M, img0, img1, out, fmt=MOTION_F32, flow=None, flow_pitch=0, mask=None, mask_pitch=0, cus=0, gpuid=0):
    """op_tail() through the motion form of the kernel under test (rife_hip_op_tail_motion).  flow / mask: uint8 buffers of TAIL_GUARD bytes, h rows
    of flow_pitch / mask_pitch bytes and TAIL_GUARD bytes, uploaded as given (None = not wanted).  Returns (frame buffer, flow buffer, mask buffer), whole, as new arrays."""
    wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32
    f32 = kernel == TAIL_HEAD_F32
    trunk = np.ascontiguousarray(trunk, np.float32) if f32 else np.ascontiguousarray(trunk, np.uint8).reshape(-1)
    weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
    F = np.ascontiguousarray(F, np.float32); M = np.ascontiguousarray(M, np.float32)
    img0 = np.ascontiguousarray(img0, np.uint32); img1 = np.ascontiguousarray(img1, np.uint32)
    if weight.size != 24 * 64 * 16 or bias.size != 24 or F.shape != (hp, wp, 4) or M.shape != (hp, wp) or img0.shape != (hp, wp) or img1.shape != (hp, wp):
        raise ValueError("weight (24, 64, 4, 4), bias (24), F (hp, wp, 4), M (hp, wp) and two (hp, wp) uint32 frames")
    if trunk.size != (64 * (hp // 4) * (wp // 4) if f32 else op_s16_geom(64, hp // 4, wp // 4)[3]):
        raise ValueError("the trunk of this frame is 64 x %d x %d" % (hp // 4, wp // 4))
    bpp = {PIX_RGB8: 3, PIX_RGB10_U16: 6, PIX_A2B10G10R10: 4, PIX_RGBA8: 4}.get(pixfmt)
    buf = np.array(out, np.uint8).reshape(-1)          # copies: the call writes into them
    if bpp is not None and buf.size != 2 * TAIL_GUARD + w * h * bpp:
        raise ValueError("out must hold %d bytes" % (2 * TAIL_GUARD + w * h * bpp))
    fb = None if flow is None else np.array(flow, np.uint8).reshape(-1)
    mb = None if mask is None else np.array(mask, np.uint8).reshape(-1)
    if (fb is not None and fb.size != 2 * TAIL_GUARD + h * flow_pitch) or (mb is not None and mb.size != 2 * TAIL_GUARD + h * mask_pitch):
        raise ValueError("a motion buffer holds TAIL_GUARD + h * pitch + TAIL_GUARD bytes")
    _check(testlib().rife_hip_op_tail_motion(gpuid, int(kernel), int(pixfmt), int(w), int(h), _p(trunk), _p(weight), _p(bias), _p(F), _p(M), _p(img0), _p(img1), int(cus),
                                             _p(buf), int(fmt), _p(fb), int(flow_pitch), _p(mb), int(mask_pitch)), "op_tail_motion", testlib())
    return buf, fb, mb


def op_apply(planes0, planes1, flow, mask, out, maxval=None, extent=None, force_scalar=0, gpuid=0):
    """rife_hip_op_apply (test build): ONE launch of the apply kernel on host planes (as planes_of takes them) and host motion; `out` planes are written in place - every
    byte the kernel did not write keeps its value.  force_scalar=1: the one-pixel-per-lane form."""
    d0 = planes_of(planes0, maxval, "planes0"); d1 = planes_of(planes1, maxval, "planes1")
    do = planes_of(out, d0.maxval, "out", writable=True)
    m = _motion_in(d0.w, d0.h, flow, mask)
    wp, hp = extent if extent is not None else (0, 0)
    _check(testlib().rife_hip_op_apply(int(gpuid), ctypes.byref(d0), ctypes.byref(d1), ctypes.byref(m), int(wp), int(hp), ctypes.byref(do), int(force_scalar)), "op_apply", testlib())
    return out


def op_apply_scaled(planes0, planes1, flow, mask, out, shift, maxval=None, extent=None, force_scalar=0, gpuid=0):
    """rife_hip_op_apply_scaled (test build): ONE launch of one set - host planes of the size `shift` demands of the motion flow (mh, mw, 4), mask (mh, mw); row-strided
    views of either are uploaded with their pitch.  `out` planes are written in place; every byte the kernel did not write keeps its value."""
    mh, mw = mask.shape
    s = apply_set(planes0, planes1, shift, maxval, extent, out)
    m = _motion_in(mw, mh, flow, mask)
    _check(testlib().rife_hip_op_apply_scaled(int(gpuid), ctypes.byref(s), ctypes.byref(m), mw, mh, int(force_scalar)), "op_apply_scaled", testlib())
    return out


def op_yuv_to_rgb10(buf, w, h, pixfmt, gpuid=0):
    """k_preproc_yuv / k_preproc_yuvc alone: one flat YUV frame -> the resident form, (hp, wp) uint32 R | G << 10 | B << 20 with zero padding (hp, wp = h, w rounded up to 32n)."""
    a = _yuv_buf(buf, w, h, pixfmt, "buf")
    out = np.empty(((h + 31) // 32 * 32, (w + 31) // 32 * 32), np.uint32)
    _check(testlib().rife_hip_op_yuv_to_rgb10(gpuid, _p(a), int(w), int(h), int(pixfmt), _p(out)), "op_yuv_to_rgb10", testlib())
    return out


def op_image_to_resident(img, force_scalar=0, gpuid=0):
    """The pitched pre-processing kernel alone (force_scalar = 2: the tight kernel of the _px path on a tight image) on a rife_hip_image of HOST planes ->
    the resident form, (hp, wp) uint32."""
    out = np.empty(((img.h + 31) // 32 * 32, (img.w + 31) // 32 * 32), np.uint32)
    _check(testlib().rife_hip_op_image_to_resident(gpuid, ctypes.byref(img), int(force_scalar), _p(out)), "op_image_to_resident", testlib())
    return out


def op_hbd_to_rgb10(img, depth, force_scalar=0, gpuid=0):
    """rife_hip_op_hbd_to_rgb10 (test build): the high-bit-depth pre-processing kernel alone on a rife_hip_image of HOST u16 planes of `depth`-bit samples -> the resident
    form, (hp, wp) uint32.  force_scalar=1: the scalar form."""
    out = np.empty(((img.h + 31) // 32 * 32, (img.w + 31) // 32 * 32), np.uint32)
    _check(testlib().rife_hip_op_hbd_to_rgb10(int(gpuid), ctypes.byref(img), int(depth), _p(out), int(force_scalar)), "op_hbd_to_rgb10", testlib())
    return out


def op_packed_to_rgb10(arr, depth, force_scalar=0, gpuid=0):
    """rife_hip_op_packed_to_rgb10 (test build): the packed pre-processing kernel alone on an (h, w, 3 | 4) uint16 HOST frame (as packed_of takes it, uploaded with its
    pitch and alignment) -> (the resident form, (hp, wp) uint32; True where the vector form ran).  force_scalar=1: the scalar form."""
    d = packed_of(arr, depth)
    out = np.empty(((d.h + 31) // 32 * 32, (d.w + 31) // 32 * 32), np.uint32)
    rc = testlib().rife_hip_op_packed_to_rgb10(int(gpuid), ctypes.byref(d), _p(out), int(force_scalar))
    if rc < 0:
        _check(rc, "op_packed_to_rgb10", testlib())
    return out, rc == 1


def op_apply_packed(in0, in1, flow, mask, out, depth, force_scalar=0, gpuid=0):
    """rife_hip_op_apply_packed (test build): ONE launch of the packed blend on (h, w, 3 | 4) uint16 HOST frames (as packed_of takes them) and host motion flow
    (h, w, 4), mask (h, w); `out` is written in place - every byte the kernel did not write keeps its value.  Returns True where the vector form ran."""
    d0 = packed_of(in0, depth, "in0"); d1 = packed_of(in1, depth, "in1"); do = packed_of(out, depth, "out", writable=True)
    m = _motion_in(d0.w, d0.h, flow, mask)
    rc = testlib().rife_hip_op_apply_packed(int(gpuid), ctypes.byref(d0), ctypes.byref(d1), ctypes.byref(do), ctypes.byref(m), int(force_scalar))
    if rc < 0:
        _check(rc, "op_apply_packed", testlib())
    return rc == 1


def op_sp_to_rgb10(y, cbcr, depth, chroma, csp=0, force_scalar=0, gpuid=0):
    """rife_hip_op_sp_to_rgb10 (test build): the semi-planar pre-processing kernel alone on a HOST surface (as semiplanar_of takes it, uploaded with its pitches and
    alignment) -> (the resident form, (hp, wp) uint32; True where the vector form ran).  force_scalar=1: the scalar form."""
    d = semiplanar_of(y, cbcr, depth, chroma, csp)
    out = np.empty(((d.h + 31) // 32 * 32, (d.w + 31) // 32 * 32), np.uint32)
    rc = testlib().rife_hip_op_sp_to_rgb10(int(gpuid), ctypes.byref(d), _p(out), int(force_scalar))
    if rc < 0:
        _check(rc, "op_sp_to_rgb10", testlib())
    return out, rc == 1


def op_apply_sp(in0, in1, flow, mask, out, depth, chroma, force_scalar=0, gpuid=0):
    """rife_hip_op_apply_sp (test build): ONE launch of the semi-planar blend on HOST surfaces (y, cbcr) (as semiplanar_of takes them) and host motion flow (h, w, 4),
    mask (h, w); the `out` pair is written in place - every byte the kernel did not write keeps its value.  Returns True where the vector form ran."""
    d0 = semiplanar_of(in0[0], in0[1], depth, chroma, 0, "in0"); d1 = semiplanar_of(in1[0], in1[1], depth, chroma, 0, "in1")
    do = semiplanar_of(out[0], out[1], depth, chroma, 0, "out", writable=True)
    m = _motion_in(d0.w, d0.h, flow, mask)
    rc = testlib().rife_hip_op_apply_sp(int(gpuid), ctypes.byref(d0), ctypes.byref(d1), ctypes.byref(do), ctypes.byref(m), d0.w, d0.h, int(force_scalar))
    if rc < 0:
        _check(rc, "op_apply_sp", testlib())
    return rc == 1


def op_apply_yuv(luma0, luma1, chroma0, chroma1, flow, mask, luma_out, chroma_out, shift, maxval=None, gpuid=0):
    """rife_hip_op_apply_yuv (test build): the apply launches of a subsampled high-bit-depth image alone - one luma plane and two chroma planes per frame (host
    arrays as planes_of takes them, uploaded with their pitch and alignment), shift = (-1, -1) 4:2:0 or (-1, 0) 4:2:2 for the chroma planes, a motion flow (mh, mw, 4),
    mask (mh, mw).  The output planes are written in place.  Returns True where this was ONE launch of k_apply_yuv, False where it was the two launches of the sets calls."""
    mh, mw = mask.shape
    sy = apply_set(luma0, luma1, (0, 0), maxval, None, luma_out)
    sc = apply_set(chroma0, chroma1, shift, maxval, None, chroma_out)
    m = _motion_in(mw, mh, flow, mask)
    rc = testlib().rife_hip_op_apply_yuv(int(gpuid), ctypes.byref(sy), ctypes.byref(sc), ctypes.byref(m), mw, mh)
    if rc < 0:
        _check(rc, "op_apply_yuv", testlib())
    return rc == 1


def op_resident_to_image(tight, img, force_scalar=0, gpuid=0):
    """The pitched output kernel alone: `tight` (4:2:0: (h, w) uint32 A2B10G10R10; RGB formats: the tight frame of the format) -> the HOST planes of `img`."""
    a = np.ascontiguousarray(tight)
    _check(testlib().rife_hip_op_resident_to_image(gpuid, _p(a), ctypes.byref(img), int(force_scalar)), "op_resident_to_image", testlib())


def op_rgb10_to_yuv(packed, pixfmt, gpuid=0):
    """k_postproc_yuv / k_postproc_yuvc alone: an (h, w) uint32 A2B10G10R10 frame -> one flat YUV frame of `pixfmt`."""
    a = np.ascontiguousarray(packed, np.uint32)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("packed must be an (h, w) uint32 array")
    h, w = a.shape
    out = np.empty(yuv_frame_bytes(w, h, pixfmt) // np.dtype(yuv_dtype(pixfmt)).itemsize, yuv_dtype(pixfmt))
    _check(testlib().rife_hip_op_rgb10_to_yuv(gpuid, _p(a), w, h, int(pixfmt), _p(out)), "op_rgb10_to_yuv", testlib())
    return out


# ---- the rife-v2.x / v3.x schedule's own kernels alone (include/rife_hip_test.h, csrc/engine_v2_ops.h): arrays in DEVICE layout (NHWC float32, resident uint32 frames);
# every `out` argument goes to the device as given and the whole buffer after the launch is returned as a new array ----
def _v2_frames(img0, img1):
    """Two frames of one form: (hp, wp) uint32 resident dwords (ImgU8) or (hp, wp, 4) float32 (ImgF4).  Returns (imgf4, img0, img1, wp, hp)."""
    f4 = np.asarray(img0).dtype != np.uint32
    a = np.ascontiguousarray(img0, np.float32 if f4 else np.uint32); b = np.ascontiguousarray(img1, np.float32 if f4 else np.uint32)
    if a.shape != b.shape or a.ndim != (3 if f4 else 2) or (f4 and a.shape[2] != 4):
        raise ValueError("two (hp, wp) uint32 frames or two (hp, wp, 4) float32 frames")
    return int(f4), a, b, a.shape[1], a.shape[0]


def _v2_out(out, shape, dtype=np.float32):
    o = np.array(out, dtype)                           # a copy: the call writes into it
    if o.shape != tuple(shape):
        raise ValueError("out must be %s" % (tuple(shape),))
    return o


def op_v2_assemble(S, img0, img1, acc, out, first=False, fscale=False, gpuid=0):
    """k2_assemble0<S> (first; acc unused) -> (hp / S, wp / S, 8), or k2_assemble<S, FSCALE> -> (hp / S, wp / S, 16), pad channels included."""
    f4, a, b, wp, hp = _v2_frames(img0, img1)
    acc = None if acc is None else np.ascontiguousarray(acc, np.float32)
    if acc is not None and acc.shape != (hp // 2, wp // 2, 4):
        raise ValueError("acc must be (hp / 2, wp / 2, 4)")
    o = _v2_out(out, (hp // S, wp // S, 8 if first else 16))
    _check(testlib().rife_hip_op_v2_assemble(gpuid, int(S), int(first), int(fscale), f4, _p(a), _p(b), wp, hp, _p(acc), _p(o)), "op_v2_assemble", testlib())
    return o


def op_v2_stem(route, S, img0, img1, acc, weight, bias, slope, out, fscale=False, gpuid=0):
    """The 10 -> cout stride-2 stem on the block input at scale S through `route` (V2_STEM_PRODUCT / _NO_R64 / _UNFUSED).  weight (cout, 10, 3, 3); out (hp / 2S, wp / 2S, out_ld)."""
    f4, a, b, wp, hp = _v2_frames(img0, img1)
    acc = np.ascontiguousarray(acc, np.float32); weight = np.ascontiguousarray(weight, np.float32)
    bias = np.ascontiguousarray(bias, np.float32); slope = np.ascontiguousarray(slope, np.float32)
    cout = weight.shape[0]
    if acc.shape != (hp // 2, wp // 2, 4) or weight.shape != (cout, 10, 3, 3) or bias.shape != (cout,) or slope.shape != (cout,):
        raise ValueError("acc (hp / 2, wp / 2, 4), weight (cout, 10, 3, 3), bias (cout) and slope (cout)")
    o = np.array(out, np.float32)
    if o.ndim != 3 or o.shape[:2] != (hp // S // 2, wp // S // 2):
        raise ValueError("out must be (hp / 2S, wp / 2S, out_ld)")
    _check(testlib().rife_hip_op_v2_stem(gpuid, int(route), int(S), int(fscale), f4, _p(a), _p(b), wp, hp, _p(acc), _p(weight), _p(bias), _p(slope), cout, o.shape[2], _p(o)),
           "op_v2_stem", testlib())
    return o


def op_v2_flow_accum(S, D, acc, first=False, mul=False, gpuid=0):
    """k2_flow_accum<S, FIRST, MUL>: D (hh / S, wh / S, 4) into acc (hh, wh, 4); returns acc after the launch."""
    D = np.ascontiguousarray(D, np.float32)
    a = np.array(acc, np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or D.shape != (a.shape[0] // S, a.shape[1] // S, 4):
        raise ValueError("acc (hh, wh, 4) and D (hh / S, wh / S, 4)")
    _check(testlib().rife_hip_op_v2_flow_accum(gpuid, int(S), int(first), int(mul), _p(D), a.shape[1], a.shape[0], _p(a)), "op_v2_flow_accum", testlib())
    return a


def op_v2_ctx_warps(acc, feats, fl, cat, batch=False, gpuid=0):
    """The ContextNet's flow pyramids and warps (batch: the one k2_warp_nhwc_batch launch).  feats / fl: eight arrays [4 frame + level], (h_l, w_l, 32 << level) /
    (h_l, w_l, 2); cat: B1..B4, (h_l, w_l, 128 << level).  Returns (fl, cat) after the launches."""
    acc = np.ascontiguousarray(acc, np.float32)
    hp, wp = 2 * acc.shape[0], 2 * acc.shape[1]
    dims = [(hp >> (l + 2), wp >> (l + 2)) for l in range(4)]
    feats = [np.ascontiguousarray(f, np.float32) for f in feats]
    fl = [_v2_out(f, dims[z & 3] + (2,)) for z, f in enumerate(fl)]
    cat = [_v2_out(c, dims[l] + (128 << l,)) for l, c in enumerate(cat)]
    if len(feats) != 8 or len(fl) != 8 or len(cat) != 4 or any(f.shape != dims[z & 3] + (32 << (z & 3),) for z, f in enumerate(feats)):
        raise ValueError("eight feature tensors (h_l, w_l, 32 << level), eight flow levels and four concat buffers")
    pf = (ctypes.c_void_p * 8)(*[f.ctypes.data for f in feats]); pl = (ctypes.c_void_p * 8)(*[f.ctypes.data for f in fl]); pc = (ctypes.c_void_p * 4)(*[c.ctypes.data for c in cat])
    _check(testlib().rife_hip_op_v2_ctx_warps(gpuid, int(batch), _p(acc), wp, hp, pf, pl, pc), "op_v2_ctx_warps", testlib())
    return fl, cat


def op_v2_final(img0, img1, w, h, acc, head, out, float_form=False, gpuid=0):
    """k2_final (uint8 buffer: TAIL_GUARD + w * h * 3 + TAIL_GUARD bytes) / k2_final_float (TAIL_GUARD + hp * wp * 16 + TAIL_GUARD bytes); returns the whole buffer."""
    _, a, b, wp, hp = _v2_frames(np.asarray(img0, np.uint32), np.asarray(img1, np.uint32))
    acc = np.ascontiguousarray(acc, np.float32); head = np.ascontiguousarray(head, np.float32)
    if (wp, hp) != ((w + 31) // 32 * 32, (h + 31) // 32 * 32) or acc.shape != (hp // 2, wp // 2, 4) or head.shape != (hp, wp, 4):
        raise ValueError("frames (hp, wp), acc (hp / 2, wp / 2, 4) and head (hp, wp, 4) of the frame padded to 32n")
    buf = _v2_out(np.asarray(out, np.uint8).reshape(-1), (2 * TAIL_GUARD + (hp * wp * 16 if float_form else w * h * 3),), np.uint8)
    _check(testlib().rife_hip_op_v2_final(gpuid, int(float_form), _p(a), _p(b), int(w), int(h), _p(acc), _p(head), _p(buf)), "op_v2_final", testlib())
    return buf


def op_v2_uhd(x, out, gpuid=0):
    """k2_image_half ((hp, wp) uint32 -> (hp / 2, wp / 2, 4)) or k2_flow_up2_double ((hp / 2, wp / 2, 4) float32 -> (hp, wp, 4)), by the input's type."""
    what = int(np.asarray(x).dtype != np.uint32)
    a = np.ascontiguousarray(x, np.float32 if what else np.uint32)
    hp, wp = (2 * a.shape[0], 2 * a.shape[1]) if what else a.shape
    o = _v2_out(out, (hp, wp, 4) if what else (hp // 2, wp // 2, 4))
    _check(testlib().rife_hip_op_v2_uhd(gpuid, what, _p(a), wp, hp, _p(o)), "op_v2_uhd", testlib())
    return o


def op_v2_conv_img(img0, img1, weight, bias, slope, out0, out1=None, cus=0, gpuid=0):
    """conv_img_s2_kernel on one frame (img1, out1 None: gridDim.y = 1) or on both (gridDim.y = 2).  weight (32, 3, 3, 3); out (hp / 2, wp / 2, 32).  Returns out0 or (out0, out1)."""
    two = img1 is not None
    a = np.ascontiguousarray(img0, np.uint32); b = np.ascontiguousarray(img1, np.uint32) if two else None
    hp, wp = a.shape
    weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32); slope = np.ascontiguousarray(slope, np.float32)
    if weight.shape != (32, 3, 3, 3) or bias.shape != (32,) or slope.shape != (32,) or (two and (b.shape != a.shape or out1 is None)):
        raise ValueError("weight (32, 3, 3, 3), bias (32), slope (32); two frames of one size need two outputs")
    o0 = _v2_out(out0, (hp // 2, wp // 2, 32)); o1 = _v2_out(out1, (hp // 2, wp // 2, 32)) if two else None
    _check(testlib().rife_hip_op_v2_conv_img(gpuid, int(two), int(cus), _p(a), _p(b), wp, hp, _p(weight), _p(bias), _p(slope), _p(o0), _p(o1)), "op_v2_conv_img", testlib())
    return (o0, o1) if two else o0


def op_conv_pair(weight, bias, slope, x0, y0, x1=None, y1=None, y_coff=0, y2=None, y2_coff=0, stride=1, deconv=False, gpuid=0):
    """launch_conv with a second tensor pair (x1, y1) or a second destination view (y2).  weight (cout, cin, 3, 3) or, deconv, (cout, cin, 4, 4); x (H, W, cin); y0 / y1
    (Ho, Wo, y_ld) with the layer's channels at y_coff; y2 (Ho, Wo, y2_ld) at y2_coff.  Returns the destinations that were given, in that order."""
    weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32); slope = np.ascontiguousarray(slope, np.float32)
    cout, cin = weight.shape[:2]
    x0 = np.ascontiguousarray(x0, np.float32); x1 = None if x1 is None else np.ascontiguousarray(x1, np.float32)
    H, W = x0.shape[:2]
    if x0.shape != (H, W, cin) or (x1 is not None and x1.shape != x0.shape) or bias.shape != (cout,) or slope.shape != (cout,):
        raise ValueError("x (H, W, cin), bias (cout) and slope (cout)")
    o0 = np.array(y0, np.float32); o1 = None if y1 is None else np.array(y1, np.float32); o2 = None if y2 is None else np.array(y2, np.float32)
    if o0.ndim != 3 or (o1 is not None and o1.shape != o0.shape) or (o2 is not None and (o2.ndim != 3 or o2.shape[:2] != o0.shape[:2])):
        raise ValueError("destinations are (Ho, Wo, ld) arrays of one pixel grid")
    _check(testlib().rife_hip_op_conv_pair(gpuid, cin, cout, int(stride), int(deconv), H, W, _p(weight), _p(bias), _p(slope), _p(x0), _p(x1), _p(o0), _p(o1), o0.shape[2], int(y_coff),
                                           _p(o2), 0 if o2 is None else o2.shape[2], int(y2_coff)), "op_conv_pair", testlib())
    return tuple(o for o in (o0, o1, o2) if o is not None)
