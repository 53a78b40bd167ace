"""RGB8 against RGBA8 in the same process: frames/s of rife-v4.6 at 3840x2160 and 1920x1080 for the two formats, alternating, three repeats each.

    python tools/bench_alpha.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/alpha/alpha_bench.txt]

Layout and timed region of bench.py's headline leg (and of tools/bench_deep.py): frames resident in HBM at native resolution (the reference's real pair tiled;
the RGBA frames are the same pictures with a smooth matte as their fourth byte), four pairs in flight - four host threads, each driving one stream that owns
half of the compute units (rife_hip_stream_create(i % 2, 2)) through rife_hip_process_device / rife_hip_process_device_px - W untimed warm-up steps, then K timed
steps ended by a device synchronisation.  A second leg times rife_hip_process_device_batch / _batch_px with four pairs per call (its lockstep groups run on the
engine's own whole-chip streams).  Then one profiled pass per format: the kernel-class table of rife_hip_profile_read.
The bar: fps_rgba >= 0.97 * fps_rgb8 (0.97 = the +-3 % spread between boxes and runs the README states); the exit code says whether it held."""
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
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        matte = np.rint(127.5 + 127.5 * np.sin(xx * 0.011) * np.cos(yy * 0.013)).astype(np.uint8)
        fr = {"rgb": [], "rgba": []}
        for i in range(4):
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))
            fr["rgb"].append(torch.from_numpy(f8).cuda())
            fr["rgba"].append(torch.from_numpy(np.ascontiguousarray(np.dstack([f8, np.roll(matte, 3 * i, axis=1)])).reshape(-1)).cuda())
        outs = {"rgb": [torch.empty(w * h * 3, dtype=torch.uint8, device="cuda") for _ in range(4)], "rgba": [torch.empty(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(4)]}
        fmt = {"rgb": amd.PIX_RGB8, "rgba": amd.PIX_RGBA8}

        def step(px, i):
            s = i % 4
            eng.process_device(fr[px][i % 4].data_ptr(), fr[px][(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[px][s].data_ptr(), streams[s], pixfmt=fmt[px])

        def run_steps(px, first, count):
            def worker(s):
                torch.cuda.set_device(0)
                for i in range(first, first + count):
                    if i % 4 == s:
                        step(px, i)
            th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
            [t.start() for t in th]
            [t.join() for t in th]

        def timed(px):
            run_steps(px, 0, 4)
            for i in range(args.warmup):
                step(px, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(px, args.warmup, steps)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)

        def timed_batch(px):
            def call(i):
                k = [(i + j) % 4 for j in range(4)]
                eng.process_device_batch([fr[px][q].data_ptr() for q in k], [fr[px][(q + 1) % 4].data_ptr() for q in k], w, h, [timesteps[(i + j) % 5] for j in range(4)],
                                         [outs[px][j].data_ptr() for j in range(4)], bstream.cuda_stream, pixfmt=fmt[px])
            for i in range(2):
                call(i)
            torch.cuda.synchronize()
            n = max(1, steps // 4)
            t0 = time.perf_counter()
            for i in range(n):
                call(i)
            torch.cuda.synchronize()
            return 4 * n / (time.perf_counter() - t0)

        res = {"rgb": [], "rgba": []}
        resb = {"rgb": [], "rgba": []}
        for r in range(args.repeats):
            for px in ("rgb", "rgba"):
                res[px].append(timed(px))
        for r in range(args.repeats):
            for px in ("rgb", "rgba"):
                resb[px].append(timed_batch(px))
        med = {d: float(np.median(res[d])) for d in res}
        medb = {d: float(np.median(resb[d])) for d in resb}
        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, steps, args.repeats))
        say("   RGB8          frames/s %s   median %.1f" % (" ".join("%.1f" % v for v in res["rgb"]), med["rgb"]))
        say("   RGBA8         frames/s %s   median %.1f   ratio %.4f (bar 0.97)" % (" ".join("%.1f" % v for v in res["rgba"]), med["rgba"], med["rgba"] / med["rgb"]))
        say("   process_device_batch, 4 pairs per call:  RGB8 %s median %.1f;  RGBA8 %s median %.1f;  ratio %.4f" %
            (" ".join("%.1f" % v for v in resb["rgb"]), medb["rgb"], " ".join("%.1f" % v for v in resb["rgba"]), medb["rgba"], medb["rgba"] / medb["rgb"]))
        ok = ok and med["rgba"] >= 0.97 * med["rgb"]
        # kernel classes of one profiled stretch per format (events around every launch: slower than the timed region, comparable between the formats)
        prof = {}
        for px in ("rgb", "rgba"):
            eng.profile_enable(True)
            for i in range(32):
                step(px, i)
            torch.cuda.synchronize()
            prof[px] = eng.profile_read()
            eng.profile_enable(False)
        say("   kernel classes, ms per pair (32 profiled pairs):   class     RGB8    RGBA8  ratio")
        for cls in sorted(prof["rgb"], key=lambda c: -prof["rgb"][c]["ms"]):
            a, b = prof["rgb"][cls]["ms"] / 32, prof["rgba"].get(cls, {"ms": 0.0})["ms"] / 32
            say("      %-14s %8.4f %8.4f  %6.3f" % (cls, a, b, b / a if a > 0 else 0.0))
        say("      %-14s %8.4f %8.4f  %6.3f" % ("total", sum(v["ms"] for v in prof["rgb"].values()) / 32, sum(v["ms"] for v in prof["rgba"].values()) / 32,
                                                 sum(v["ms"] for v in prof["rgba"].values()) / max(1e-9, sum(v["ms"] for v in prof["rgb"].values()))))
        del fr, outs
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "fps_rgba >= 0.97 * fps_rgb8 at every size", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
