"""Flow scale 2 against flow scale 1 in the same process: frames/s of rife-v4.6 at 3840x2160 and 1920x1080, one engine per scale, alternating, three rounds each.

    python tools/bench_flowscale.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/flowscale/bench_flowscale.txt]

Layout and timed region of bench.py's headline leg (as tools/bench_deep.py): RGB8 frames resident in HBM at native resolution (the reference's real pair tiled), four pairs
in flight - four host threads, each driving one stream that owns half of the compute units (rife_hip_stream_create(i % 2, 2)) through rife_hip_process_device - W
untimed warm-up steps, then K timed steps ended by a device synchronisation.  Every round is printed.  Then one profiled stretch per scale on ONE stream (pairs one
after the other, events around every launch): the kernel-class table of rife_hip_profile_read, ms per pair.
The bar: at 4K the scale-2 rate is at least 1.5 x the scale-1 rate of the same process (the work model - trunks, stems and heads at a quarter, the full-resolution
passes unchanged - predicts about 2.5 x); 1080p has no bar, only the number.  The exit code says whether the 4K bar held."""
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
BAR_4K = 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="timed steps per round (default: 240 at 4K, 600 at 1080p)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    modeldir = gen_models.ensure(None, "rife-v4.6")
    eng, streams = {}, {}
    for scale in (1, 2):
        eng[scale] = amd.RIFE(0, rife_v4=True)
        eng[scale].load(modeldir)
        eng[scale].set_flow_scale(scale)
        streams[scale] = [eng[scale].stream_create(i % 2, 2) for i in range(4)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    ratios = {}
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        fr = [torch.from_numpy(np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))).cuda() for i in range(4)]
        outs = [torch.empty(w * h * 3, dtype=torch.uint8, device="cuda") for _ in range(4)]

        def step(scale, i, stream=None):
            s = i % 4
            eng[scale].process_device(fr[i % 4].data_ptr(), fr[(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[s].data_ptr(), stream if stream is not None else streams[scale][s])

        def run_steps(scale, first, count):
            def worker(s):
                torch.cuda.set_device(0)
                for i in range(first, first + count):
                    if i % 4 == s:
                        step(scale, i)
            th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
            [t.start() for t in th]
            [t.join() for t in th]

        def timed(scale):
            run_steps(scale, 0, 4)
            for i in range(args.warmup):
                step(scale, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(scale, args.warmup, steps)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)

        res = {1: [], 2: []}
        for r in range(args.repeats):
            for scale in (1, 2):
                res[scale].append(timed(scale))
                say("   %s round %d, flow scale %d: %.1f frames/s" % (name, r + 1, scale, res[scale][-1]))
        med = {s: float(np.median(res[s])) for s in res}
        ratios[name] = med[2] / med[1]
        say("%s %dx%d, %d steps x %d rounds, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, steps, args.repeats))
        say("   flow scale 1   frames/s %s   median %.1f" % (" ".join("%.1f" % v for v in res[1]), med[1]))
        say("   flow scale 2   frames/s %s   median %.1f   ratio %.3f%s" % (" ".join("%.1f" % v for v in res[2]), med[2], ratios[name],
                                                                             " (bar %.1f, work model 2.5)" % BAR_4K if name == "4k" else " (no bar)"))
        if name == "4k":
            ok = ok and ratios[name] >= BAR_4K
        prof = {}
        NP = 16
        for scale in (1, 2):
            for i in range(2):
                step(scale, i, streams[scale][0])
            torch.cuda.synchronize()
            eng[scale].profile_enable(True)
            for i in range(NP):
                step(scale, i, streams[scale][0])
            torch.cuda.synchronize()
            prof[scale] = eng[scale].profile_read()
            eng[scale].profile_enable(False)
        say("   kernel classes, ms per pair (%d profiled pairs, one stream on half of the compute units):   class  scale 1  scale 2  ratio" % NP)
        for cls in sorted(set(prof[1]) | set(prof[2]), key=lambda c: -prof[1].get(c, {"ms": 0.0})["ms"]):
            a, b = prof[1].get(cls, {"ms": 0.0})["ms"] / NP, prof[2].get(cls, {"ms": 0.0})["ms"] / NP
            say("      %-14s %8.4f %8.4f  %6.3f" % (cls, a, b, b / a if a > 0 else 0.0))
        ta, tb = (sum(v["ms"] for v in prof[s].values()) / NP for s in (1, 2))
        say("      %-14s %8.4f %8.4f  %6.3f" % ("total", ta, tb, tb / max(1e-9, ta)))
        del fr, outs
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "4K: fps(flow scale 2) >= %.1f * fps(flow scale 1), same process" % BAR_4K, "ratios": {k: round(v, 3) for k, v in ratios.items()}, "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
