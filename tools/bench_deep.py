"""Depth 8 against depth 10 in the same process: frames/s of rife-v4.6 at 3840x2160 and 1920x1080 for RGB8 and A2B10G10R10, alternating, three repeats each.

    python tools/bench_deep.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/.../deep_bench.txt]

Layout and timed region of bench.py's headline leg: frames resident in HBM at native resolution (the reference's real pair tiled; the 10-bit frames are the same
pictures with two random low bits under every sample, so that they are truly 10-bit), four pairs in flight - four host threads, each driving one stream that owns
half of the compute units (rife_hip_stream_create(i % 2, 2)) through rife_hip_process_device / rife_hip_process_device_px - W untimed warm-up steps, then K timed
steps ended by a device synchronisation.  A second leg times rife_hip_process_device_batch / _batch_px with four pairs per call (its lockstep groups run on the
engine's own whole-chip streams).  Then one profiled pass per depth: the kernel-class table of rife_hip_profile_read.
The bar: fps10 >= 0.97 * fps8 (0.97 = the +-3 % spread between boxes and runs the README states); the exit code says whether it held."""
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
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    bstream = torch.cuda.Stream()
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        fr = {8: [], 10: []}
        for i in range(4):
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))
            codes = (f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16)
            fr[8].append(torch.from_numpy(f8).cuda())
            fr[10].append(torch.from_numpy(amd.pack_a2b10g10r10(codes).view(np.uint8).reshape(-1)).cuda())
        outs = {8: [torch.empty(w * h * 3, dtype=torch.uint8, device="cuda") for _ in range(4)], 10: [torch.empty(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(4)]}
        fmt = {8: amd.PIX_RGB8, 10: amd.PIX_A2B10G10R10}

        def step(depth, i):
            s = i % 4
            eng.process_device(fr[depth][i % 4].data_ptr(), fr[depth][(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[depth][s].data_ptr(), streams[s], pixfmt=fmt[depth])

        def run_steps(depth, first, count):
            def worker(s):
                torch.cuda.set_device(0)
                for i in range(first, first + count):
                    if i % 4 == s:
                        step(depth, i)
            th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
            [t.start() for t in th]
            [t.join() for t in th]

        def timed(depth):
            run_steps(depth, 0, 4)
            for i in range(args.warmup):
                step(depth, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(depth, args.warmup, steps)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)

        def timed_batch(depth):
            def call(i):
                k = [(i + j) % 4 for j in range(4)]
                eng.process_device_batch([fr[depth][q].data_ptr() for q in k], [fr[depth][(q + 1) % 4].data_ptr() for q in k], w, h, [timesteps[(i + j) % 5] for j in range(4)],
                                         [outs[depth][j].data_ptr() for j in range(4)], bstream.cuda_stream, pixfmt=fmt[depth])
            for i in range(2):
                call(i)
            torch.cuda.synchronize()
            n = max(1, steps // 4)
            t0 = time.perf_counter()
            for i in range(n):
                call(i)
            torch.cuda.synchronize()
            return 4 * n / (time.perf_counter() - t0)

        res = {8: [], 10: []}
        resb = {8: [], 10: []}
        for r in range(args.repeats):
            for depth in (8, 10):
                res[depth].append(timed(depth))
        for r in range(args.repeats):
            for depth in (8, 10):
                resb[depth].append(timed_batch(depth))
        med = {d: float(np.median(res[d])) for d in res}
        medb = {d: float(np.median(resb[d])) for d in resb}
        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, steps, args.repeats))
        say("   RGB8          frames/s %s   median %.1f" % (" ".join("%.1f" % v for v in res[8]), med[8]))
        say("   A2B10G10R10   frames/s %s   median %.1f   ratio %.4f (bar 0.97)" % (" ".join("%.1f" % v for v in res[10]), med[10], med[10] / med[8]))
        say("   process_device_batch, 4 pairs per call:  RGB8 %s median %.1f;  A2B10G10R10 %s median %.1f;  ratio %.4f" %
            (" ".join("%.1f" % v for v in resb[8]), medb[8], " ".join("%.1f" % v for v in resb[10]), medb[10], medb[10] / medb[8]))
        ok = ok and med[10] >= 0.97 * med[8]
        # kernel classes of one profiled stretch per depth (events around every launch: slower than the timed region, comparable between the depths)
        prof = {}
        for depth in (8, 10):
            eng.profile_enable(True)
            for i in range(32):
                step(depth, i)
            torch.cuda.synchronize()
            prof[depth] = eng.profile_read()
            eng.profile_enable(False)
        say("   kernel classes, ms per pair (32 profiled pairs):   class  depth 8  depth 10  ratio")
        for cls in sorted(prof[8], key=lambda c: -prof[8][c]["ms"]):
            a, b = prof[8][cls]["ms"] / 32, prof[10].get(cls, {"ms": 0.0})["ms"] / 32
            say("      %-14s %8.4f %8.4f  %6.3f" % (cls, a, b, b / a if a > 0 else 0.0))
        say("      %-14s %8.4f %8.4f  %6.3f" % ("total", sum(v["ms"] for v in prof[8].values()) / 32, sum(v["ms"] for v in prof[10].values()) / 32,
                                                 sum(v["ms"] for v in prof[10].values()) / max(1e-9, sum(v["ms"] for v in prof[8].values()))))
        del fr, outs
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "fps10 >= 0.97 * fps8 at every size", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
