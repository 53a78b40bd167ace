"""Fast precision against full precision in the same process: frames/s of rife-v4.6 at 3840x2160 and 1920x1080, and at 4K with flow scale 2, one engine per
precision, alternating, three rounds each.

    python tools/bench_fastprec.py [--steps K] [--warmup W] [--repeats R] [--configs 4k,1080p,4k-fs2] [--out profiles/fastprec/bench.txt]

Layout and timed region of bench.py's headline leg (as tools/bench_flowscale.py): RGB8 frames resident in HBM at native resolution (the reference's real pair tiled),
four pairs in flight - four host threads, each driving one stream that owns half of the compute units (rife_hip_stream_create(i % 2, 2)) through
rife_hip_process_device - W untimed warm-up steps, then K timed steps ended by a device synchronisation.  Every round is printed.  Then one profiled stretch per
precision on ONE stream (pairs one after the other, events around every launch): the kernel-class table of rife_hip_profile_read, ms per pair, with the four trunk
classes (trunk_b0 .. trunk_b3) first.
The bar: fast precision beats full precision of the same process by more than the +- 3 % by which the boxes of the pool differ, at 4K and at 1080p; 4K at flow scale
2 has no bar, only the number.  The exit code says whether the bar held.  The instruction-count model (38 of 74 matrix instructions per row of the block-3 trunk) puts
the ceiling at 1.38 x for a 4K pair; the loaders still move both planes."""
import argparse
import gc
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

CONFIGS = {"4k": (3840, 2160, 1), "1080p": (1920, 1080, 1), "4k-fs2": (3840, 2160, 2)}
BAR = 1.03
BARRED = ("4k", "1080p")
MODES = ("full", "fast")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="timed steps per round (default: 240 at 4K, 600 at 1080p and at 4K with flow scale 2)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="4k,1080p,4k-fs2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    modeldir = gen_models.ensure(None, "rife-v4.6")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    ratios, plain = {}, {}
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    for name in args.configs.split(","):
        w, h, fscale = CONFIGS[name]
        steps = args.steps or (240 if name == "4k" else 600)
        eng, streams = {}, {}
        for mode in MODES:
            eng[mode] = amd.RIFE(0, rife_v4=True)
            eng[mode].load(modeldir)
            eng[mode].set_flow_scale(fscale)
            eng[mode].set_precision(mode)
            streams[mode] = [eng[mode].stream_create(i % 2, 2) for i in range(4)]
        base = gen_frames.tiled_real_pair(w // 640)
        fr = [torch.from_numpy(np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))).cuda() for i in range(4)]
        outs = [torch.empty(w * h * 3, dtype=torch.uint8, device="cuda") for _ in range(4)]

        def step(mode, i, stream=None):
            s = i % 4
            eng[mode].process_device(fr[i % 4].data_ptr(), fr[(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[s].data_ptr(), stream if stream is not None else streams[mode][s])

        def run_steps(mode, first, count):
            def worker(s):
                torch.cuda.set_device(0)
                for i in range(first, first + count):
                    if i % 4 == s:
                        step(mode, i)
            th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
            [t.start() for t in th]
            [t.join() for t in th]

        def timed(mode):
            run_steps(mode, 0, 4)
            for i in range(args.warmup):
                step(mode, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(mode, args.warmup, steps)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)

        res = {m: [] for m in MODES}
        for r in range(args.repeats):
            for mode in MODES:
                res[mode].append(timed(mode))
                say("   %s round %d, %s precision: %.1f frames/s" % (name, r + 1, mode, res[mode][-1]))
        med = {m: float(np.median(res[m])) for m in MODES}
        ratios[name] = med["fast"] / med["full"]
        plain[name] = med["full"]
        say("%s %dx%d flow scale %d, %d steps x %d rounds, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, fscale, steps, args.repeats))
        say("   full precision   frames/s %s   median %.1f" % (" ".join("%.1f" % v for v in res["full"]), med["full"]))
        say("   fast precision   frames/s %s   median %.1f   ratio %.3f%s" % (" ".join("%.1f" % v for v in res["fast"]), med["fast"], ratios[name],
                                                                               " (bar > %.2f, model ceiling 1.38 at 4K)" % BAR if name in BARRED else " (no bar)"))
        if name in BARRED:
            ok = ok and ratios[name] > BAR
        prof = {}
        NP = 16
        for mode in MODES:
            for i in range(2):
                step(mode, i, streams[mode][0])
            torch.cuda.synchronize()
            eng[mode].profile_enable(True)
            for i in range(NP):
                step(mode, i, streams[mode][0])
            torch.cuda.synchronize()
            prof[mode] = eng[mode].profile_read()
            eng[mode].profile_enable(False)
        say("   kernel classes, ms per pair (%d profiled pairs, one stream on half of the compute units):   class  full  fast  ratio" % NP)
        ms = lambda m, c: prof[m].get(c, {"ms": 0.0})["ms"] / NP
        classes = sorted(set(prof["full"]) | set(prof["fast"]), key=lambda c: (not c.startswith("trunk_b"), c if c.startswith("trunk_b") else -ms("full", c)))
        for cls in classes:
            a, b = ms("full", cls), ms("fast", cls)
            say("      %-14s %8.4f %8.4f  %6.3f" % (cls, a, b, b / a if a > 0 else 0.0))
        ta, tb = (sum(v["ms"] for v in prof[m].values()) / NP for m in MODES)
        say("      %-14s %8.4f %8.4f  %6.3f" % ("total", ta, tb, tb / max(1e-9, ta)))
        for mode in MODES:
            for s in streams[mode]:
                eng[mode].stream_destroy(s)
        del fr, outs, eng, streams
        gc.collect()
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "fps(fast precision) > %.2f * fps(full precision), same process, at %s" % (BAR, " and ".join(BARRED)),
                    "ratios": {k: round(v, 3) for k, v in ratios.items()}, "full_precision_fps": {k: round(v, 1) for k, v in plain.items()}, "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
