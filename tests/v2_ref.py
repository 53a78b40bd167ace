"""References of the rife-v2.x / v3.x schedule's own kernels (csrc/elementwise_v2.h, stem_fused_v2.h, conv_img.h) for tests/test_gpu_v2_ops.py.

elementwise_v2.h is compiled with -ffp-contract=off as "a literal restatement of the reference arithmetic": every product and every sum is rounded to float32 on its
own.  The functions here restate those kernels step by step in numpy float32 (one rounding per numpy operation, no fused multiply-add), in the kernels' operation
order, so their results are the kernels' results BIT FOR BIT; tests/test_v2_ref.py pins each of them bit for bit to the CPU oracle (OracleRIFE.net_extract on
injected blobs), without a GPU.  Tensors are in the kernels' layout: NHWC float32, frames as (hp, wp) uint32 resident dwords or (hp, wp, 3 | 4) float32.

Also here: the float64 3x3 stride-2 convolution the stems and conv_img are measured against, the injected flow fields of the tests, the share of sampling positions
they keep inside the frame, and a small reader of ncnn .param files that finds blobs by the graph's STRUCTURE (the synthetic models name their blobs differently
from the reference's)."""
import numpy as np

f32 = np.float32


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------------------
def pack_rgb(rgb8):
    """(hp, wp, 3) uint8 -> resident dwords R | G << 8 | B << 16."""
    a = rgb8.astype(np.uint32)
    return np.ascontiguousarray(a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16))


def unpack_rgb(img):
    """elementwise.h unpack_rgb<8>: code * (1 / 255.f) per channel.  A float frame ((hp, wp, 3 | 4): ImgF4) passes through with its first three channels."""
    img = np.asarray(img)
    if img.dtype != np.uint32:
        return np.ascontiguousarray(img[..., :3], f32)
    k = f32(1) / f32(255)
    return np.stack([((img >> s) & 0xFF).astype(f32) * k for s in (0, 8, 16)], axis=-1)


def padded_frames(w, h, seed, noise=True):
    """Two frames of w x h, zero-padded to 32n as the pre-processing kernel leaves them: ((hp, wp) uint32, (hp, wp) uint32)."""
    wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        px = np.zeros((hp, wp, 3), np.uint8)
        if noise:
            px[:h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            ph = rng.uniform(0, 6.28, 3)
            px[:h, :w] = np.stack([127.5 + 120 * np.sin(xx * 0.31 + ph[c]) * np.cos(yy * 0.23 + c) for c in range(3)], axis=-1).astype(np.uint8)
        out.append(pack_rgb(px))
    return out[0], out[1]


# ---- the pieces (elementwise.h) ----------------------------------------------------------------------------------------------------------------------------
def up_coeff(n_out, S, n_in):
    """up_coeff: ncnn linear_coeffs of an upscale by S for output indices 0 .. n_out - 1 -> (s0, a0, a1)."""
    d = np.arange(n_out, dtype=f32)
    f = (d + f32(0.5)) * (f32(1) / f32(S)) - f32(0.5)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(f32)
    lo, hi = s < 0, s >= n_in - 1
    s = np.where(lo, 0, np.where(hi, n_in - 2, s))
    f = np.where(lo, f32(0), np.where(hi, f32(1), f)).astype(f32)
    return s, (f32(1) - f).astype(f32), f


def interp_up(D, S):
    """Interp(x S) of an NHWC field, in the order of k2_flow_accum / flow_up2x2: (q00 a0 + q01 a1) b0 + (q10 a0 + q11 a1) b1."""
    D = np.asarray(D, f32)
    H, W = D.shape[:2]
    sy, b0, b1 = up_coeff(H * S, S, H)
    sx, a0, a1 = up_coeff(W * S, S, W)
    a0, a1 = a0[None, :, None], a1[None, :, None]
    b0, b1 = b0[:, None, None], b1[:, None, None]
    q00, q01 = D[sy][:, sx], D[sy][:, sx + 1]
    q10, q11 = D[sy + 1][:, sx], D[sy + 1][:, sx + 1]
    return (q00 * a0 + q01 * a1) * b0 + (q10 * a0 + q11 * a1) * b1


def flow_up2x2(acc):
    """2 * Interp(x2)(acc): the full-resolution flow of a running flow at half resolution (Resize, Mul 2)."""
    return interp_up(acc, 2) * f32(2)


def warp_taps(fx, fy):
    """warp_taps at every pixel of an (h, w) grid: clamped tap coordinates and the clamp-then-alpha weights (src/warp.cpp:126-146)."""
    h, w = fx.shape
    yy, xx = np.mgrid[0:h, 0:w]
    sx = xx.astype(f32) + np.asarray(fx, f32)
    sy = yy.astype(f32) + np.asarray(fy, f32)
    x0 = np.floor(sx).astype(np.int64); y0 = np.floor(sy).astype(np.int64)
    x1 = np.clip(x0 + 1, 0, w - 1); y1 = np.clip(y0 + 1, 0, h - 1)
    x0 = np.clip(x0, 0, w - 1); y0 = np.clip(y0, 0, h - 1)
    return x0, x1, y0, y1, sx - x0.astype(f32), sy - y0.astype(f32)


def warp(img, fx, fy):
    """rife.Warp of an (h, w, C) tensor by a flow given as two (h, w) planes: warp_lerp of the four taps."""
    img = np.asarray(img, f32)
    x0, x1, y0, y1, al, be = warp_taps(fx, fy)
    al, be = al[..., None], be[..., None]
    v4 = img[y0, x0] * (f32(1) - al) + img[y0, x1] * al
    v5 = img[y1, x0] * (f32(1) - al) + img[y1, x1] * al
    return v4 * (f32(1) - be) + v5 * be


def down4(v, S):
    """Interp(1 / S), S = 2^k: the source centre falls between pixels S i + S / 2 - 1 and S i + S / 2 with both weights 0.5 (elementwise.h down4)."""
    o = S // 2 - 1
    v00, v01 = v[o::S, o::S], v[o::S, o + 1::S]
    v10, v11 = v[o + 1::S, o::S], v[o + 1::S, o + 1::S]
    h = f32(0.5)
    return (v00 * h + v01 * h) * h + (v10 * h + v11 * h) * h


def inside_share(fx, fy):
    """Share of the sampling positions (x + fx, y + fy) whose four taps are four different pixels of the frame: no clamp on either axis."""
    h, w = fx.shape
    yy, xx = np.mgrid[0:h, 0:w]
    sx, sy = xx + fx.astype(np.float64), yy + fy.astype(np.float64)
    return float(((sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)).mean())


# ---- the kernels (elementwise_v2.h) ------------------------------------------------------------------------------------------------------------------------
def assemble0(img0, img1, S):
    """k2_assemble0<S>: Interp(1 / S)(Concat(img0, img1)) as NHWC8 {rgb0, rgb1, 0, 0}."""
    v = np.concatenate([unpack_rgb(img0), unpack_rgb(img1)], axis=-1)
    d = down4(v, S)
    return np.concatenate([d, np.zeros(d.shape[:2] + (2,), f32)], axis=-1)


def block_input_full(img0, img1, acc):
    """Concat(warp(img0, Ff.xy), warp(img1, Ff.zw), Ff), Ff = 2 * Interp(x2)(acc): the 10 channels at full resolution."""
    F = flow_up2x2(acc)
    w0 = warp(unpack_rgb(img0), F[..., 0], F[..., 1])
    w1 = warp(unpack_rgb(img1), F[..., 2], F[..., 3])
    return np.concatenate([w0, w1, F], axis=-1)


def assemble10(img0, img1, acc, S, fscale=False):
    """assemble2_pixel<S, IMG, FSCALE> at every pixel of the 1 / S grid: 10 channels."""
    v = block_input_full(img0, img1, acc)
    if S > 1:
        v = down4(v, S)
        if fscale:
            v[..., 6:] = v[..., 6:] * (f32(1) / f32(S))
    return np.ascontiguousarray(v, f32)


def assemble(img0, img1, acc, S, fscale=False):
    """k2_assemble<S, IMG, FSCALE>: NHWC16, ten channels and six zeros."""
    v = assemble10(img0, img1, acc, S, fscale)
    return np.concatenate([v, np.zeros(v.shape[:2] + (6,), f32)], axis=-1)


def flow_accum(D, acc, S, first=False, mul=False):
    """k2_flow_accum<S, FIRST, MUL>: acc = (FIRST ? 0 : acc) + Interp(x S)(D) (* S)."""
    u = np.asarray(D, f32) if S == 1 else interp_up(D, S)
    if mul and S > 1:
        u = u * f32(S)
    return np.ascontiguousarray(u if first else np.asarray(acc, f32) + u, f32)


def flow_pyramid(acc, c0):
    """The k2_flow_half chain: four levels, each Interp(1 / 2) * 0.5 of the one before; level 0 from channels c0, c0 + 1 of acc."""
    out, cur = [], np.asarray(acc, f32)[..., c0:c0 + 2]
    for _ in range(4):
        cur = np.ascontiguousarray(down4(cur, 2) * f32(0.5), f32)
        out.append(cur)
    return out


def warp_nhwc(feat, flow2):
    """k2_warp_nhwc / k2_warp_nhwc_batch: rife.Warp of (h, w, C) features by an (h, w, 2) flow."""
    return warp(feat, flow2[..., 0], flow2[..., 1])


def ctx_concat(acc, feats, cat):
    """The four concat buffers after the eight warps: level l of frame im lands in channels [64 << l + im (32 << l), + 32 << l) of cat[l]; the rest stays."""
    out = [np.array(c, f32) for c in cat]
    pyr = [flow_pyramid(acc, 0), flow_pyramid(acc, 2)]
    for im in range(2):
        for l in range(4):
            C = 32 << l
            o = (64 << l) + im * C
            out[l][..., o:o + C] = warp_nhwc(feats[4 * im + l], pyr[im][l])
    return pyr[0] + pyr[1], out


def final_float(img0, img1, acc, head):
    """k2_final_float: clip(warp(img0) m + warp(img1) (1 - m) + (o.rgb * 2 - 1), 0, 1) as float4 {r, g, b, 0} per padded pixel."""
    F = flow_up2x2(acc)
    w0 = warp(unpack_rgb(img0), F[..., 0], F[..., 1])
    w1 = warp(unpack_rgb(img1), F[..., 2], F[..., 3])
    head = np.asarray(head, f32)
    m = head[..., 3:4]
    rm = f32(1) - m
    v = (w0 * m + w1 * rm) + (head[..., :3] * f32(2) - f32(1))
    v = np.minimum(np.maximum(v, f32(0)), f32(1))
    return np.concatenate([v, np.zeros(v.shape[:2] + (1,), f32)], axis=-1)


def final_u8(img0, img1, acc, head, w, h):
    """k2_final: the same, quantised as the reference's postproc does - clamp((int)(v * 255 + 0.5)) - on the w x h frame."""
    v = final_float(img0, img1, acc, head)[:h, :w, :3]
    return np.clip((v * f32(255) + f32(0.5)).astype(np.int32), 0, 255).astype(np.uint8)


def image_half(img):
    """k2_image_half: Interp(0.5) of the frame's float samples as float4 {r, g, b, 0}."""
    d = down4(unpack_rgb(img), 2)
    return np.concatenate([d, np.zeros(d.shape[:2] + (1,), f32)], axis=-1)


flow_up2_double = flow_up2x2      # k2_flow_up2_double: (Interp x2) * 2.0, the arithmetic of the in-graph "Resize, Mul 2"


# ---- float64 convolution -----------------------------------------------------------------------------------------------------------------------------------
def conv3x3_s2_f64(x, weight, bias, slope):
    """3x3 stride-2 pad-1 convolution + bias + PReLU in float64.  x (H, W, C), weight (O, C, 3, 3) -> (Ho, Wo, O)."""
    x = np.asarray(x, np.float64); wt = np.asarray(weight, np.float64)
    H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((H + 2, W + 2, C))
    xp[1:-1, 1:-1] = x
    out = np.zeros((Ho, Wo, wt.shape[0]))
    for dy in range(3):
        for dx in range(3):
            out += xp[dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] @ wt[:, :, dy, dx].T
    out += np.asarray(bias, np.float64)
    return np.where(out < 0, out * np.asarray(slope, np.float64), out)


# ---- injected fields ---------------------------------------------------------------------------------------------------------------------------------------
FIELDS = ("zero", "shift", "smooth", "clamp")
SMOOTH = ("smooth",)                                  # the fields that must keep a quarter to nine tenths of the sampling positions inside


def injected_acc(wp, hp, kind, seed=0):
    """A running flow acc (hp / 2, wp / 2, 4) to inject.  The flow that samples the frames is 2 * Interp(x2)(acc), in full-resolution pixels.
    zero: no motion.  shift: an integer shift per channel (taps land on pixels, alpha = beta = 0, clamps along two edges).  smooth: a smooth field whose peak moves
    a sample by 0.3 of the frame's width / height, plus noise of a few pixels (fractional weights everywhere; roughly half of the positions leave the frame).
    clamp: thousands of pixels, signs by quadrant - every tap clamps, towards each of the four corners."""
    H, W = hp // 2, wp // 2
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.zeros((H, W, 4), f32)
    if kind == "shift":
        a[:] = np.array([1.5, -1.0, -2.5, 2.0], f32)          # x 2: 3, -2, -5, 4 pixels
    elif kind == "smooth":
        for c in range(4):
            dim = wp if c % 2 == 0 else hp
            ph = rng.uniform(0, 6.28, 2)
            a[..., c] = 0.15 * dim * np.sin(xx * (rng.uniform(0.7, 1.6) * 6.28 / W) + ph[0]) * np.cos(yy * (rng.uniform(0.7, 1.6) * 6.28 / H) + ph[1]) + rng.normal(0, 0.6, (H, W))
    elif kind == "clamp":
        sx = np.where(xx < W / 2, -1.0, 1.0); sy = np.where(yy < H / 2, 1.0, -1.0)
        a[..., 0] = 3000 * sx + rng.normal(0, 40, (H, W)); a[..., 1] = 2500 * sy + rng.normal(0, 40, (H, W))
        a[..., 2] = -2700 * sx + rng.normal(0, 40, (H, W)); a[..., 3] = -3100 * sy + rng.normal(0, 40, (H, W))
    elif kind != "zero":
        raise ValueError(kind)
    return np.ascontiguousarray(a, f32)


def inside_shares(acc):
    """The inside share of every warp the schedule runs from this acc: both frames at full resolution (assembly at every S, the stems, the final kernels) and the
    ContextNet levels of at least 8 x 8 pixels (a level of fewer rows or columns has no or hardly any position whose four taps are different pixels)."""
    F = flow_up2x2(acc)
    out = {"full0": inside_share(F[..., 0], F[..., 1]), "full1": inside_share(F[..., 2], F[..., 3])}
    for im in range(2):
        for l, fl in enumerate(flow_pyramid(acc, 2 * im)):
            if min(fl.shape[:2]) >= 8:
                out["ctx%d_l%d" % (im, l)] = inside_share(fl[..., 0], fl[..., 1])
    return out


# ---- ncnn .param files by structure --------------------------------------------------------------------------------------------------------------------------
class Param:
    """The layers of an ncnn .param file: (type, name, bottoms, tops, {id: value})."""

    def __init__(self, path):
        self.layers = []
        for line in list(open(path))[2:]:
            f = line.split()
            if len(f) < 4:
                continue
            nb, nt = int(f[2]), int(f[3])
            kv = dict(x.split("=", 1) for x in f[4 + nb + nt:])
            self.layers.append((f[0], f[1], f[4:4 + nb], f[4 + nb:4 + nb + nt], kv))

    def producer(self, blob):
        return next(l for l in self.layers if blob in l[3])

    def consumers(self, blob):
        return [l for l in self.layers if blob in l[2]]

    def of_type(self, t):
        return [l for l in self.layers if l[0] == t]

    def conv_inputs(self, cin):
        """Bottoms of the 3x3 Convolution layers with `cin` input channels (weight count / (9 cout)), in file order."""
        return [l[2][0] for l in self.of_type("Convolution") if int(l[4]["6"]) == 9 * cin * int(l[4]["0"])]

    def through(self, blob, types=("Interp", "BinaryOp")):
        """Follow `blob` through the single-input layers of `types` that consume it alone; returns the last top."""
        while True:
            c = self.consumers(blob)
            if len(c) != 1 or c[0][0] not in types or len(c[0][2]) != 1:
                return blob
            blob = c[0][3][0]

    def head_tops(self):
        """What each IFNet head adds to the running flow: the Deconvolution's top followed through its Interp (rife-v3.x: and Mul)."""
        return [self.through(l[3][0]) for l in self.of_type("Deconvolution")]
