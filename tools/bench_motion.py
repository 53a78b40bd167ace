"""Motion export (include/rife_hip.h rife_hip_motion_t) against the plain call in the same process: what storing the final flows and the blend mask costs.

    python tools/bench_motion.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/motion/bench.txt]

bench.py's headline layout (tools/bench_planar.py): frames and motion buffers resident in HBM, four pairs in flight - four host threads, each driving one stream of
rife_hip_stream_create that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  Three legs on A2B10G10R10 frames of
the same scene, alternating, R repeats each: rife_hip_process_device_px (the yardstick), rife_hip_process_device_motion with F32 buffers, and with F16 buffers.
The traffic model: F32 motion adds 20 bytes per pixel (166 MB at 4K) to the ~5.6 GB a 4K pair moves, ratio about 0.97; F16 half of that, about 0.985.  The bars
are the model minus 0.03 (the scatter same-process legs have shown here): F32 >= 0.94 and F16 >= 0.955 of the plain rate of the same run, at every size.  Before
the timing, the frame of a motion call must be the plain call's, byte for byte.
Then the kernels that finish the frame alone: one pair at a time on the engine's own stream, the profiler's events around every launch - milliseconds per pair of
the class that holds the final kernel (head_b3, or `final` where the tail is not fused), plain against the two motion formats.
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
BAR = {"motion F32": 0.94, "motion F16": 0.955}


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
    LEGS = ["plain", "motion F32", "motion F16"]
    FMT = {"motion F32": (amd.MOTION_F32, 4), "motion F16": (amd.MOTION_F16, 2)}
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        fr = []
        for i in range(4):      # four frames of the reference's real pair tiled, as ten-bit codes
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))[:h, :w]
            fr.append(torch.from_numpy(amd.pack_a2b10g10r10((f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16))).cuda())
        outs = [torch.empty_like(fr[0]) for _ in range(4)]
        mo = {}
        for leg, (fmt, es) in FMT.items():      # tight motion buffers, one set per pair in flight
            mo[leg] = []
            for s in range(4):
                f = torch.empty((h, w * 4 * es), dtype=torch.uint8, device="cuda"); m = torch.empty((h, w * es), dtype=torch.uint8, device="cuda")
                mo[leg].append((amd.motion_desc(f.data_ptr(), m.data_ptr(), fmt, w * 4 * es, w * es), f, m))

        def step(leg, i, stream="part"):
            s = i % 4
            st = streams[s] if stream == "part" else stream
            a, b, t, o = fr[i % 4].data_ptr(), fr[(i + 1) % 4].data_ptr(), timesteps[i % 5], outs[s].data_ptr()
            if leg == "plain":
                eng.process_device(a, b, w, h, t, o, st, pixfmt=amd.PIX_A2B10G10R10)
            else:
                eng.process_device_motion(a, b, w, h, t, o, mo[leg][s][0], stream=st, pixfmt=amd.PIX_A2B10G10R10)

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

        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), A2B10G10R10 frames and motion buffers resident:" % (name, w, h, steps, args.repeats))
        same = {}
        for leg in LEGS[1:]:      # same frame bytes first
            step("plain", 0, None); torch.cuda.synchronize(); want = outs[0].cpu().numpy().copy()
            outs[0].zero_()
            step(leg, 0, None); torch.cuda.synchronize()
            same[leg] = bool(np.array_equal(outs[0].cpu().numpy(), want))
        res = {leg: [] for leg in LEGS}
        for r in range(args.repeats):
            for leg in LEGS:
                res[leg].append(timed(leg))
        med = {leg: float(np.median(res[leg])) for leg in LEGS}
        say("   %-12s frames/s %s  median %.1f" % ("plain", " ".join("%.1f" % v for v in res["plain"]), med["plain"]))
        for leg in LEGS[1:]:
            say("   %-12s frames/s %s  median %.1f | ratio to plain %.4f (bar %.3f) | same frame bytes as the plain call: %s" %
                (leg, " ".join("%.1f" % v for v in res[leg]), med[leg], med[leg] / med["plain"], BAR[leg], same[leg]))
            ok = ok and same[leg] and med[leg] >= BAR[leg] * med["plain"]
        say("   the kernel that finishes the frame alone (one pair at a time, whole chip; profiler events around each launch), 16 pairs per leg, ms per pair:")
        for leg in LEGS:
            for i in range(2):
                step(leg, i, None)
            eng.profile_enable(True)
            for i in range(16):
                step(leg, i, None)
            torch.cuda.synchronize()
            prof = eng.profile_read()
            eng.profile_enable(False)
            say("      %-12s %s" % (leg, "  ".join("%s %.4f" % (k, prof[k]["ms"] / 16) for k in sorted(prof) if "head" in k or "final" in k)))
        del fr, outs, mo
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "motion F32 >= 0.94 and F16 >= 0.955 of the plain A2B10G10R10 rate of the same run, at every size (resident frames)", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
