"""Apply motion (include/rife_hip.h rife_hip_planes_t) against the motion call in the same process: what applying the motion to the caller's planes costs.

    python tools/bench_apply.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/apply/bench.txt]

tools/bench_motion.py's layout: frames, planes and motion resident in HBM, four pairs in flight - four host threads, each driving one stream of
rife_hip_stream_create that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  Legs on RGB8 frames of the same
scene, alternating, R repeats each: rife_hip_process_device_motion with F32 buffers (the yardstick) and rife_hip_process_device_apply with 3 x u8, 3 x u16 and 3 x
float planes.  The traffic model: on top of the ~5.6 GB a 4K pair moves (675 B per pixel) the apply adds 20 B of motion read plus n * es * 3 per pixel (two plane
reads, one write): ratios 0.959 (u8), 0.947 (u16), 0.923 (float); the bar of a leg is its ratio minus 0.03, the scatter same-process legs have shown here.
Before the timing, the contract must hold on the bench inputs: frame and planes of process_device_apply are byte for byte process_device_motion then
apply_device_motion.
Then the apply kernel alone: one pair at a time on the engine's own stream, the profiler's events around every launch - milliseconds per launch and bytes / s of the
class apply_motion, next to the byte model (20 + 3 n es per pixel) evaluated at the bandwidth the RGBPF post-processing kernel (16 B per pixel) reaches in the same
run; the apply kernel may take up to twice that time (every output sample gathers eight taps through the cache instead of streaming).
The exit code says whether the bars held."""
import argparse
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
PAIR_BYTES_PER_PIXEL = 675.0      # 5.6 GB per 4K pair
N = 3


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
    from tools import gen_frames, gen_models
    eng = amd.RIFE(0, rife_v4=True)
    eng.load(gen_models.ensure(None, "rife-v4.6"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    KIND = {"apply 3 x u8": (amd.SAMPLE_U8, np.uint8, 255), "apply 3 x u16": (amd.SAMPLE_U16, np.uint16, 65535), "apply 3 x float": (amd.SAMPLE_F32, np.float32, 0)}
    LEGS = ["motion F32"] + list(KIND)
    model = {leg: PAIR_BYTES_PER_PIXEL / (PAIR_BYTES_PER_PIXEL + 20 + 3 * N * np.dtype(k[1]).itemsize) for leg, k in KIND.items()}
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        f8 = [np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))[:h, :w] for i in range(4)]
        fr = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in f8]
        outs = [torch.empty_like(fr[0]) for _ in range(4)]
        mo = []
        for s in range(4):      # tight F32 motion buffers, one set per pair in flight (the yardstick's)
            f = torch.empty((h, w * 16), dtype=torch.uint8, device="cuda"); m = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda")
            mo.append((amd.motion_desc(f.data_ptr(), m.data_ptr(), amd.MOTION_F32, w * 16, w * 4), f, m))
        planes, pouts = {}, {}
        for leg, (sample, dt, maxval) in KIND.items():      # the frames' own R, G, B planes carried at the leg's sample type, plus sub-code noise where the type has room
            es = np.dtype(dt).itemsize
            src = []
            for f in f8:
                p = np.moveaxis(f, -1, 0).astype(np.float64)
                if dt == np.uint16:
                    p = p * 257 + rng.integers(-128, 129, p.shape)
                elif dt == np.float32:
                    p = (p + rng.random(p.shape) - 0.5) / 255.0
                src.append(torch.from_numpy(np.ascontiguousarray(np.clip(p, 0, maxval or 1).astype(dt)).view(np.uint8).reshape(N, h, w * es)).cuda())
            desc = lambda t, sample=sample, es=es, maxval=maxval: amd.planes_desc(w, h, sample, [(t[k].data_ptr(), w * es) for k in range(N)], maxval or None)
            planes[leg] = [(desc(t), t) for t in src]
            pouts[leg] = []
            for s in range(4):
                t = torch.empty((N, h, w * es), dtype=torch.uint8, device="cuda")
                pouts[leg].append((desc(t), t))
        ext = eng.padded_size(w, h)

        def step(leg, i, stream="part"):
            s = i % 4
            st = streams[s] if stream == "part" else stream
            a, b, t, o = fr[i % 4].data_ptr(), fr[(i + 1) % 4].data_ptr(), timesteps[i % 5], outs[s].data_ptr()
            if leg == "motion F32":
                eng.process_device_motion(a, b, w, h, t, o, mo[s][0], stream=st)
            else:
                eng.process_device_apply(a, b, w, h, t, o, planes[leg][i % 4][0], planes[leg][(i + 1) % 4][0], pouts[leg][s][0], extent=ext, stream=st)

        def run_steps(leg, first, count):
            def worker(s):
                torch.cuda.set_device(0)
                for i in range(first, first + count):
                    if i % 4 == s:
                        step(leg, i)
            th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
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

        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), RGB8 frames, planes and motion resident:" % (name, w, h, steps, args.repeats))
        same = {}
        for leg in LEGS[1:]:      # the contract first: process_device_apply == process_device_motion, then apply_device_motion
            step("motion F32", 0, None); torch.cuda.synchronize()
            want_frame = outs[0].cpu().numpy().copy()
            ref = torch.empty_like(pouts[leg][0][1])
            sample, dt, maxval = KIND[leg]
            es = np.dtype(dt).itemsize
            eng.apply_device_motion(planes[leg][0][0], planes[leg][1][0], mo[0][0], amd.planes_desc(w, h, sample, [(ref[k].data_ptr(), w * es) for k in range(N)], maxval or None), extent=ext)
            torch.cuda.synchronize()
            outs[0].zero_(); pouts[leg][0][1].zero_()
            step(leg, 0, None); torch.cuda.synchronize()
            same[leg] = bool(np.array_equal(outs[0].cpu().numpy(), want_frame)) and bool(torch.equal(pouts[leg][0][1], ref))
        res = {leg: [] for leg in LEGS}
        for r in range(args.repeats):
            for leg in LEGS:
                res[leg].append(timed(leg))
        med = {leg: float(np.median(res[leg])) for leg in LEGS}
        say("   %-16s frames/s %s  median %.1f" % (LEGS[0], " ".join("%.1f" % v for v in res[LEGS[0]]), med[LEGS[0]]))
        for leg in LEGS[1:]:
            bar = model[leg] - 0.03
            say("   %-16s frames/s %s  median %.1f | ratio to motion F32 %.4f (model %.3f, bar %.3f) | the contract holds on these inputs: %s" %
                (leg, " ".join("%.1f" % v for v in res[leg]), med[leg], med[leg] / med[LEGS[0]], model[leg], bar, same[leg]))
            ok = ok and same[leg] and med[leg] >= bar * med[LEGS[0]]
        say("   the apply kernel alone (one pair at a time, whole chip; profiler events around each launch), 16 pairs per leg:")
        fpl = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(f, -1, 0)).astype(np.float32) / np.float32(255)).cuda() for f in f8[:2]]      # RGBPF frames for the streaming yardstick
        fo = torch.empty_like(fpl[0])
        for i in range(2):
            eng.process_device(fpl[0].data_ptr(), fpl[1].data_ptr(), w, h, 0.5, fo.data_ptr(), None, pixfmt=amd.PIX_RGBPF)
        eng.profile_enable(True)
        for i in range(16):
            eng.process_device(fpl[0].data_ptr(), fpl[1].data_ptr(), w, h, timesteps[i % 5], fo.data_ptr(), None, pixfmt=amd.PIX_RGBPF)
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile_enable(False)
        post_ms = prof["postproc_rgbp"]["ms"] / 16
        bw = 16.0 * w * h / (post_ms * 1e-3)
        say("      %-16s %.4f ms per launch, %.2f TB/s (16 B per pixel, streaming)" % ("postproc RGBPF", post_ms, bw / 1e12))
        for leg in LEGS[1:]:
            for i in range(2):
                step(leg, i, None)
            eng.profile_enable(True)
            for i in range(16):
                step(leg, i, None)
            torch.cuda.synchronize()
            prof = eng.profile_read()
            eng.profile_enable(False)
            ms = prof["apply_motion"]["ms"] / 16
            nbytes = (20.0 + 3 * N * np.dtype(KIND[leg][1]).itemsize) * w * h
            model_ms = nbytes / bw * 1e3
            say("      %-16s %.4f ms per launch, %.2f TB/s of the byte model (%.0f B per pixel) | model at the streaming rate %.4f ms, ratio %.2f (bar 2.0)" %
                (leg, ms, nbytes / (ms * 1e-3) / 1e12, nbytes / (w * h), model_ms, ms / model_ms))
            ok = ok and ms <= 2.0 * model_ms
        del fr, outs, mo, planes, pouts, fpl, fo
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "process_device_apply >= (traffic model - 0.03) of the process_device_motion rate of the same run, the contract holds, the apply kernel within 2x its byte model", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
