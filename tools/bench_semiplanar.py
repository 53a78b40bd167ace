"""Semi-planar surfaces (include/rife_hip.h rife_hip_semiplanar_t) against the planar hbd call that defines them, in the same process.

    python tools/bench_semiplanar.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/semiplanar/bench.txt]

tools/bench_packed.py's layout: frames resident in HBM, four pairs in flight - four host threads, each driving one stream of rife_hip_stream_create that owns half of
the compute units - W untimed steps, K timed steps ended by a device synchronisation; legs alternating, R repeats each.  Three pairs of legs, the same samples in both
legs of a pair: 12-bit 4:2:0 (P012), 12-bit 4:2:2 (P212), 16-bit 4:2:0 (P016):
    (a) planar        rife_hip_process_device_hbd on the PRE-SPLIT planes Y >> s, Cb >> s, Cr >> s (I420P10 / I422P10 layout)      the yardstick; it does not pay for the split
    (b) semi-planar   rife_hip_process_device_hbd_semiplanar on the surface itself
Bar: (b) >= 0.97 of (a), the standing bar for a format variant.  Before the timing the contract must hold on the bench inputs: the surface (b) writes is byte for byte
join(planes << s) of what (a) writes.
Then the kernels alone, one pair at a time on the engine's own stream with the profiler's events around every launch, on the motion the engine estimates for these
frames: apply_sp against apply_yuv of leg (a) (bar: no longer than it plus 10 %), and the two preproc_sp launches of a call against the two launches of class preproc
(k_preproc_hbd_x8<1, SUBY>) of the planar call.
Last the blend alone on fields the tool supplies (rife_hip_bench_apply_sp of the bench build: the launch on surfaces, planes and motion in device memory, 200 launches
between two events, variants alternating, three repeats): a smooth field of a few pixels' amplitude and a rough one (independent uniform displacements of up to 8 pixels
per pixel), k_apply_sp against k_apply_yuv on the same samples and the same field, after their outputs agreed byte for byte; the same bar of 1.10.
The exit code says whether the bars held."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"4k": (3840, 2160), "1080p": (1920, 1080)}
PAIRS = [("P012 4:2:0", 1, 12), ("P212 4:2:2", 2, 12), ("P016 4:2:0", 1, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="timed steps per repeat (default: 240 at 4K, 600 at 1080p)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import benchlib, gen_frames, gen_models
    BL = benchlib.lib()
    BL.rife_hip_bench_apply_sp.argtypes = [ctypes.c_int] + [ctypes.POINTER(amd.rife_hip_semiplanar)] * 3 + [ctypes.POINTER(amd.rife_hip_image)] * 3 + [
        ctypes.POINTER(amd.rife_hip_motion), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    eng = amd.RIFE(0, rife_v4=True)
    eng.load(gen_models.ensure(None, "rife-v4.6"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        cw = w // 2
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        unit = []      # four frames as float planes in [0, 1]: BT.709 luma and chroma of the scene of bench_apply.py, limited range, full-resolution chroma
        for i in range(4):
            f = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))[:h, :w].astype(np.float32) / 255.0
            yv = 0.2126 * f[..., 0] + 0.7152 * f[..., 1] + 0.0722 * f[..., 2]
            unit.append(((16.0 + 219.0 * yv) / 256.0, (128.0 + 224.0 * (f[..., 2] - yv) / 1.8556) / 256.0, (128.0 + 224.0 * (f[..., 0] - yv) / 1.5748) / 256.0))
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
        fields = {}
        for kind in ("smooth", "rough"):
            if kind == "smooth":
                f = np.stack([3 * np.sin(xs / 97) * np.cos(ys / 61), 2.5 * np.cos(xs / 83) * np.sin(ys / 71), -3 * np.sin(xs / 89 + 1) * np.cos(ys / 67), 2 * np.cos(xs / 101) * np.cos(ys / 59)], axis=-1).astype(np.float32)
                m = (0.5 + 0.4 * np.sin(xs / 113) * np.sin(ys / 79)).astype(np.float32)
            else:
                f = rng.uniform(-8.0, 8.0, (h, w, 4)).astype(np.float32)
                m = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
            tf = torch.from_numpy(f.view(np.uint8).reshape(h, w * 16)).cuda(); tm = torch.from_numpy(m.view(np.uint8).reshape(h, w * 4)).cuda()
            fields[kind] = (tf, tm, amd.motion_desc(tf.data_ptr(), tm.data_ptr(), amd.MOTION_F32, w * 16, w * 4))
        del xs, ys
        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, steps, args.repeats))
        for label, chroma, depth in PAIRS:
            s, maxval = 16 - depth, (1 << depth) - 1
            ch = h // 2 if chroma == 1 else h
            pixfmt = amd.PIX_I420P10 if chroma == 1 else amd.PIX_I422P10
            pl, sp = [], []
            for yv, cb, cr in unit:
                sub = (lambda c: c.reshape(ch, h // ch, cw, 2).mean(axis=(1, 3)))
                code = lambda p: np.clip(p * (maxval + 1) + rng.uniform(-0.5, 0.5, p.shape), 0, maxval).astype(np.uint16)
                yy, bb, rr = code(yv), code(sub(cb)), code(sub(cr))
                pl.append((dev(yy), dev(bb), dev(rr)))
                low = lambda p: rng.integers(0, 1 << s, p.shape, dtype=np.uint32).astype(np.uint16) if s else np.uint16(0)
                cc = np.empty((ch, 2 * cw), np.uint16)
                cc[:, 0::2] = bb << s; cc[:, 1::2] = rr << s
                sp.append((dev((yy << s) | low(yy)), dev(cc | low(cc))))
            pl_out = [tuple(torch.empty_like(p) for p in pl[0]) for _ in range(4)]
            sp_out = [tuple(torch.empty_like(p) for p in sp[0]) for _ in range(4)]
            idesc = lambda t: amd.device_image(w, h, pixfmt, [(t[0].data_ptr(), w * 2), (t[1].data_ptr(), cw * 2), (t[2].data_ptr(), cw * 2)])
            sdesc = lambda t: amd.semiplanar_desc(w, h, chroma, depth, t[0].data_ptr(), w * 2, t[1].data_ptr(), cw * 4)
            LEGS = ["(a) planar", "(b) semi-planar"]

            def step(leg, i, stream="part"):
                k = i % 4
                st = streams[k] if stream == "part" else stream
                a, b, t = i % 4, (i + 1) % 4, timesteps[i % 5]
                if leg == LEGS[0]:
                    eng.process_device_hbd(idesc(pl[a]), idesc(pl[b]), t, idesc(pl_out[k]), depth, stream=st)
                else:
                    eng.process_device_hbd_semiplanar(sdesc(sp[a]), sdesc(sp[b]), t, sdesc(sp_out[k]), stream=st)

            def run_steps(leg, first, count):
                def worker(k):
                    torch.cuda.set_device(0)
                    for i in range(first, first + count):
                        if i % 4 == k:
                            step(leg, i)
                th = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
                [t.start() for t in th]
                [t.join() for t in th]

            def timed(leg):
                run_steps(leg, 0, 4)
                for i in range(args.warmup):
                    step(leg, i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(leg, args.warmup, steps)
                torch.cuda.synchronize()
                return steps / (time.perf_counter() - t0)

            # the contract first
            for p in pl_out[0] + sp_out[0]:
                p.zero_()
            step(LEGS[0], 0, None); step(LEGS[1], 0, None); torch.cuda.synchronize()
            wy = pl_out[0][0] << s
            wc = torch.stack((pl_out[0][1] << s, pl_out[0][2] << s), dim=2).reshape(ch, 2 * cw)
            same = bool(torch.equal(sp_out[0][0], wy)) and bool(torch.equal(sp_out[0][1], wc)) and bool((wy != ((sp[0][0] >> s) << s)).any())
            res = {leg: [] for leg in LEGS}
            for r in range(args.repeats):
                for leg in LEGS:
                    res[leg].append(timed(leg))
            med = {leg: float(np.median(res[leg])) for leg in LEGS}
            held = med[LEGS[1]] >= 0.97 * med[LEGS[0]]
            ok = ok and same and held
            say(" %s, depth %d:" % (label, depth))
            say("   %-16s frames/s %s  median %.1f" % (LEGS[0], " ".join("%.1f" % v for v in res[LEGS[0]]), med[LEGS[0]]))
            say("   %-16s frames/s %s  median %.1f | ratio to (a) %.4f (bar 0.97): %s | the contract holds on these inputs: %s" %
                (LEGS[1], " ".join("%.1f" % v for v in res[LEGS[1]]), med[LEGS[1]], med[LEGS[1]] / med[LEGS[0]], "held" if held else "MISSED", same))
            prof = {}
            for leg in LEGS:      # the kernels alone: one pair at a time, whole chip, profiler events around each launch, 16 pairs per leg
                for i in range(2):
                    step(leg, i, None)
                eng.profile_enable(True)
                for i in range(16):
                    step(leg, i, None)
                torch.cuda.synchronize()
                p = eng.profile_read()
                eng.profile_enable(False)
                prof[leg] = {k: v["ms"] / 16 for k, v in p.items() if v["launches"]}
            a_new, a_old = prof[LEGS[1]]["apply_sp"], prof[LEGS[0]]["apply_yuv"]
            kheld = a_new <= 1.10 * a_old
            ok = ok and kheld
            nbytes = 20.0 * w * h + 3 * 2 * (w * h + 2 * cw * ch)
            say("   kernels alone, ms per call: blend apply_sp %.4f (%.2f TB/s of the %d MB a call moves at least) | apply_yuv %.4f | ratio %.3f (bar 1.10): %s" %
                (a_new, nbytes / (a_new * 1e-3) / 1e12, int(nbytes / 1e6), a_old, a_new / a_old, "held" if kheld else "MISSED"))
            say("                               pre-processing, both inputs: preproc_sp %.4f | class preproc of the planar call %.4f | ratio %.3f" %
                (prof[LEGS[1]]["preproc_sp"], prof[LEGS[0]]["preproc"], prof[LEGS[1]]["preproc_sp"] / prof[LEGS[0]]["preproc"]))
            for leg in LEGS:
                tot = sum(prof[leg].values())
                top = sorted(prof[leg].items(), key=lambda kv: -kv[1])[:5]
                say("      %-16s all classes %.3f ms per call; largest: %s" % (leg, tot, ", ".join("%s %.3f" % kv for kv in top)))
            for kind, (tf, tm, md) in fields.items():      # the blend alone on a supplied field
                def blend(variant, iters):
                    ms = ctypes.c_float(0)
                    rc = BL.rife_hip_bench_apply_sp(0, ctypes.byref(sdesc(sp[0])), ctypes.byref(sdesc(sp[1])), ctypes.byref(sdesc(sp_out[0])), ctypes.byref(idesc(pl[0])),
                                                    ctypes.byref(idesc(pl[1])), ctypes.byref(idesc(pl_out[0])), ctypes.byref(md), variant, iters, ctypes.byref(ms))
                    if rc:
                        raise RuntimeError("rife_hip_bench_apply_sp failed (%d): %s" % (rc, BL.rife_hip_last_error().decode()))
                    return ms.value
                for p in pl_out[0] + sp_out[0]:
                    p.zero_()
                blend(0, 1); blend(1, 1); torch.cuda.synchronize()
                fsame = bool(torch.equal(sp_out[0][0], pl_out[0][0] << s)) and bool(torch.equal(sp_out[0][1], torch.stack((pl_out[0][1] << s, pl_out[0][2] << s), dim=2).reshape(ch, 2 * cw)))
                tt = {0: [], 1: []}
                for r in range(args.repeats):
                    for variant in (1, 0):
                        tt[variant].append(blend(variant, 200))
                b_new, b_old = float(np.median(tt[0])), float(np.median(tt[1]))
                fheld = b_new <= 1.10 * b_old
                ok = ok and fsame and fheld
                say("   blend alone, %-6s field, 200 launches between two events, ms per launch: k_apply_sp %s median %.4f | k_apply_yuv %s median %.4f | ratio %.3f (bar 1.10): %s | same bytes: %s" %
                    (kind, " ".join("%.4f" % v for v in tt[0]), b_new, " ".join("%.4f" % v for v in tt[1]), b_old, b_new / b_old, "held" if fheld else "MISSED", fsame))
            del pl, sp, pl_out, sp_out
            torch.cuda.empty_cache()
    say(json.dumps({"metric": "semi-planar call >= 0.97 of the planar hbd call on pre-split planes, the contract holds, apply_sp within 1.10 of apply_yuv", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
