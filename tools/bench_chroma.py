"""4:2:2 / 4:4:4 frames against the packed 10-bit format in the same process: what the wider chroma planes cost at the boundary.

    python tools/bench_chroma.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/chroma/chroma_bench.txt]

bench.py's headline layout (tools/bench_yuv.py, tools/bench_planes.py): frames resident in HBM, four pairs in flight - four host threads, each driving one stream
of rife_hip_stream_create that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  For each of I422, I422P10,
I444 and I444P10: rife_hip_process_device_px on tight frames, and rife_hip_process_device_image on planes in SEPARATE allocations whose rows are aligned to 256
bytes (never tight) plus one row of slack; A2B10G10R10 on tight frames of the same scene is the yardstick.  The legs alternate, R repeats each.
The bar: every leg >= 0.97 of the A2B10G10R10 rate at every size.  Before the timing, the tight and the image call of a format must return the same bytes.
Then the kernel-class table of one profiled stretch per leg (postproc_yuv and preproc are the classes the formats differ in).
The exit code says whether the bar held."""
import argparse
import importlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

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
    import chroma_ref as cr
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    model = gen_models.ensure(None, "rife-v4.6")
    eng = amd.RIFE(0, rife_v4=True)
    eng.load(model)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    REF = "A2B10G10R10"
    FMTS = [("I422", amd.PIX_I422), ("I422P10", amd.PIX_I422P10), ("I444", amd.PIX_I444), ("I444P10", amd.PIX_I444P10)]
    fmt = dict(FMTS, **{REF: amd.PIX_A2B10G10R10})
    LEGS = [(REF, "tight")] + [(n, path) for n, _ in FMTS for path in ("tight", "image")]

    def frames_of(w, h):
        """Four frames of the reference's real pair tiled, as tight frames (uint8 bytes) of each format."""
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        out = {n: [] for n in fmt}
        for i in range(4):
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))
            codes = (f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16)
            for n in fmt:
                f = amd.pack_a2b10g10r10(codes) if n == REF else cr.rgb10_to_yuv(codes, fmt[n])
                out[n].append(np.ascontiguousarray(f).view(np.uint8).reshape(-1))
        return out

    def plane_table(w, h, px):
        """(rows, row bytes, byte offset in the tight frame) per plane."""
        rbs = [amd.image_row_bytes(w, px, p) for p in range(3)]
        offs = [0, rbs[0] * h, rbs[0] * h + rbs[1] * h]
        return [(h, rb, off) for rb, off in zip(rbs, offs)]

    class Planes:
        """One frame in device memory as separate allocations per plane, rows aligned to 256 bytes, one row of slack after the last."""

        def __init__(self, tight, w, h, px):
            self.t = []
            planes = []
            for (rows, rb, off) in plane_table(w, h, px):
                pitch = (rb + 255) // 256 * 256
                if pitch == rb:
                    pitch += 256                               # never tight: a tight image IS the _px call and would measure nothing
                host = np.zeros((rows + 1, pitch), np.uint8)
                if tight is not None:
                    host[:rows, :rb] = tight[off:off + rows * rb].reshape(rows, rb)
                t = torch.from_numpy(host).cuda()
                self.t.append(t)
                planes.append((t.data_ptr(), pitch))
            self.desc = amd.device_image(w, h, px, planes)

    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        host = frames_of(w, h)
        fr = {n: [torch.from_numpy(x).cuda() for x in host[n]] for n in fmt}
        outs = {n: [torch.empty_like(fr[n][0]) for _ in range(4)] for n in fmt}
        pl = {n: [Planes(x, w, h, fmt[n]) for x in host[n]] for n, _ in FMTS}
        plo = {n: [Planes(None, w, h, fmt[n]) for _ in range(4)] for n, _ in FMTS}

        def step(leg, i):
            n, path = leg
            s = i % 4
            if path == "image":
                eng.process_device_image(pl[n][i % 4].desc, pl[n][(i + 1) % 4].desc, timesteps[i % 5], plo[n][s].desc, streams[s])
            else:
                eng.process_device(fr[n][i % 4].data_ptr(), fr[n][(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[n][s].data_ptr(), streams[s], pixfmt=fmt[n])

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

        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident; tight = the _px call, image = separate"
            " allocations per plane, rows aligned to 256 bytes:" % (name, w, h, steps, args.repeats))
        same = {}
        for n, _ in FMTS:      # same bytes first: the last outputs of a short stretch through both paths
            for i in range(4):
                step((n, "image"), i); step((n, "tight"), i)
            torch.cuda.synchronize()
            same[n] = True
            for s in range(4):
                tight = outs[n][s].cpu().numpy()
                for t, (rows, rb, off) in zip(plo[n][s].t, plane_table(w, h, fmt[n])):
                    same[n] = same[n] and np.array_equal(t.cpu().numpy()[:rows, :rb].reshape(-1), tight[off:off + rows * rb])
        res = {leg: [] for leg in LEGS}
        for r in range(args.repeats):
            for leg in LEGS:
                res[leg].append(timed(leg))
        med = {leg: float(np.median(res[leg])) for leg in LEGS}
        ref = med[(REF, "tight")]
        say("   %-20s frames/s %s  median %.1f" % (REF + " tight", " ".join("%.1f" % v for v in res[(REF, "tight")]), ref))
        for leg in LEGS[1:]:
            say("   %-20s frames/s %s  median %.1f | ratio to %s %.4f (bar 0.97) | tight and image return the same bytes: %s" %
                ("%s %s" % leg, " ".join("%.1f" % v for v in res[leg]), med[leg], REF, med[leg] / ref, same[leg[0]]))
            ok = ok and same[leg[0]] and med[leg] >= 0.97 * ref
        prof = {}
        for leg in LEGS:
            eng.profile_enable(True)
            for i in range(32):
                step(leg, i)
            torch.cuda.synchronize()
            prof[leg] = eng.profile_read()
            eng.profile_enable(False)
        say("   kernel classes, ms per pair (32 profiled pairs):   class  " + "  ".join("%s/%s" % c for c in LEGS))
        classes = sorted(set().union(*[set(p) for p in prof.values()]), key=lambda c: -max(p.get(c, {"ms": 0.0})["ms"] for p in prof.values()))
        for cls in classes:
            if max(prof[c].get(cls, {"ms": 0.0})["ms"] for c in LEGS) / 32 >= 0.002 or cls in ("preproc", "postproc_yuv"):
                say("      %-14s %s" % (cls, " ".join("%8.4f" % (prof[c].get(cls, {"ms": 0.0})["ms"] / 32) for c in LEGS)))
        say("      %-14s %s" % ("total", " ".join("%8.4f" % (sum(v["ms"] for v in prof[c].values()) / 32) for c in LEGS)))
        del fr, outs, pl, plo
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "I422 / I422P10 / I444 / I444P10, tight frames and pitched planes, >= 0.97 * A2B10G10R10 at every size (resident frames)", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
