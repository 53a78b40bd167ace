"""Strided planes against tight frames in the same process: what reading and writing the caller's pitched planes in place costs.

    python tools/bench_planes.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--legs resident,host] [--out profiles/planes/planes_bench.txt]

resident  bench.py's headline layout (tools/bench_yuv.py): frames resident in HBM, four pairs in flight - four host threads, each driving one stream of
          rife_hip_stream_create that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  For each of RGB8,
          A2B10G10R10, NV12 and I420P10: rife_hip_process_device_image on planes in SEPARATE allocations whose rows are aligned to 256 bytes (and never tight: + 256 where the row bytes are a
          multiple already) plus one row of slack, against rife_hip_process_device_px on the tight frames of the same samples, alternating, R repeats each.
          The bar: image >= 0.97 of the tight rate for every format at every size.  Then the kernel-class table of one profiled stretch per format and path
          (the RGB formats' store_rows class is the price of the tight workspace frame + store kernel variant).
host      4K I420 frames in pageable host memory, one caller thread: rife_hip_process_image on planes padded to 64-byte rows against "repack with numpy, then
          rife_hip_process_px, then unpack".  Both figures, no bar.
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
    ap.add_argument("--legs", default="resident,host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import planes_ref as pr
    import yuv_ref as yr
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    model = gen_models.ensure(None, "rife-v4.6")
    eng = amd.RIFE(0, rife_v4=True)
    eng.load(model)
    lines = []
    legs = args.legs.split(",")

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    FMTS = [("RGB8", amd.PIX_RGB8), ("A2B10G10R10", amd.PIX_A2B10G10R10), ("NV12", amd.PIX_NV12), ("I420P10", amd.PIX_I420P10)]

    def frames_of(w, h, names):
        """Four frames of the reference's real pair tiled, as tight frames (uint8 bytes) of each format."""
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        out = {n: [] for n in names}
        for i in range(4):
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))
            codes = (f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16)
            for n in names:
                f = f8 if n == "RGB8" else amd.pack_a2b10g10r10(codes) if n == "A2B10G10R10" else yr.rgb10_to_yuv(codes, getattr(amd, "PIX_" + n))
                out[n].append(np.ascontiguousarray(f).view(np.uint8).reshape(-1))
        return out

    class Planes:
        """One frame in device memory as separate allocations per plane, rows aligned to 256 bytes, one row of slack after the last."""

        def __init__(self, tight, w, h, px):
            self.t = []
            planes = []
            for (rows, rb, off, _) in pr.plane_table(w, h, px):
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

    if "resident" in legs:
        streams = [eng.stream_create(i % 2, 2) for i in range(4)]
        for name in args.sizes.split(","):
            w, h = SIZES[name]
            steps = args.steps or (240 if name == "4k" else 600)
            host = frames_of(w, h, [n for n, _ in FMTS])
            fmt = dict(FMTS)
            fr = {n: [torch.from_numpy(x).cuda() for x in host[n]] for n, _ in FMTS}
            outs = {n: [torch.empty_like(fr[n][0]) for _ in range(4)] for n, _ in FMTS}
            pl = {n: [Planes(x, w, h, fmt[n]) for x in host[n]] for n, _ in FMTS}
            plo = {n: [Planes(None, w, h, fmt[n]) for _ in range(4)] for n, _ in FMTS}

            def step(n, path, i):
                s = i % 4
                if path == "image":
                    eng.process_device_image(pl[n][i % 4].desc, pl[n][(i + 1) % 4].desc, timesteps[i % 5], plo[n][s].desc, streams[s])
                else:
                    eng.process_device(fr[n][i % 4].data_ptr(), fr[n][(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[n][s].data_ptr(), streams[s], pixfmt=fmt[n])

            def run_steps(n, path, first, count):
                def worker(s):
                    torch.cuda.set_device(0)
                    for i in range(first, first + count):
                        if i % 4 == s:
                            step(n, path, i)
                th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
                [t.start() for t in th]
                [t.join() for t in th]

            def timed(n, path):
                run_steps(n, path, 0, 4)
                for i in range(args.warmup):
                    step(n, path, i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(n, path, args.warmup, steps)
                torch.cuda.synchronize()
                return steps / (time.perf_counter() - t0)

            say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident; image = separate allocations per plane,"
                " rows aligned to 256 bytes:" % (name, w, h, steps, args.repeats))
            for n, _ in FMTS:
                # same bytes first: the last output of a short stretch through both paths
                for i in range(4):
                    step(n, "image", i); step(n, "tight", i)
                torch.cuda.synchronize()
                same = True
                for s in range(4):
                    tight = outs[n][s].cpu().numpy()
                    for t, (rows, rb, off, _) in zip(plo[n][s].t, pr.plane_table(w, h, fmt[n])):
                        same = same and np.array_equal(t.cpu().numpy()[:rows, :rb].reshape(-1), tight[off:off + rows * rb])
                res = {"tight": [], "image": []}
                for r in range(args.repeats):
                    for path in ("tight", "image"):
                        res[path].append(timed(n, path))
                med = {p: float(np.median(res[p])) for p in res}
                say("   %-12s tight frames/s %s  median %.1f | image %s  median %.1f | ratio %.4f (bar 0.97) | same bytes: %s" %
                    (n, " ".join("%.1f" % v for v in res["tight"]), med["tight"], " ".join("%.1f" % v for v in res["image"]), med["image"], med["image"] / med["tight"], same))
                ok = ok and same and med["image"] >= 0.97 * med["tight"]
            prof = {}
            for n, _ in FMTS:
                for path in ("tight", "image"):
                    eng.profile_enable(True)
                    for i in range(32):
                        step(n, path, i)
                    torch.cuda.synchronize()
                    prof[(n, path)] = eng.profile_read()
                    eng.profile_enable(False)
            cols = [(n, p) for n, _ in FMTS for p in ("tight", "image")]
            say("   kernel classes, ms per pair (32 profiled pairs):   class  " + "  ".join("%s/%s" % c for c in cols))
            classes = sorted(set().union(*[set(p) for p in prof.values()]), key=lambda c: -max(p.get(c, {"ms": 0.0})["ms"] for p in prof.values()))
            for cls in classes:
                if max(prof[c].get(cls, {"ms": 0.0})["ms"] for c in cols) / 32 >= 0.002 or cls in ("preproc", "postproc_yuv", "store_rows"):
                    say("      %-14s %s" % (cls, " ".join("%8.4f" % (prof[c].get(cls, {"ms": 0.0})["ms"] / 32) for c in cols)))
            say("      %-14s %s" % ("total", " ".join("%8.4f" % (sum(v["ms"] for v in prof[c].values()) / 32) for c in cols)))
            del fr, outs, pl, plo
            torch.cuda.empty_cache()

    if "host" in legs:
        w, h = SIZES["4k"]
        px = amd.PIX_I420
        tight = frames_of(w, h, ["I420"])["I420"]
        table = pr.plane_table(w, h, px)
        pairs = 24

        def padded(flat):
            out = []
            for (rows, rb, off, _) in table:
                p = np.zeros((rows, (rb + 63) // 64 * 64), np.uint8)[:, :rb]
                if flat is not None:
                    p[:] = flat[off:off + rows * rb].reshape(rows, rb)
                out.append(p)
            return tuple(out)
        planes = [padded(f) for f in tight]
        outp = padded(None)

        def image_call(i):
            eng.process_planes(planes[i % 4], planes[(i + 1) % 4], timesteps[i % 5], px, out=outp)

        def repack_call(i):
            a = np.concatenate([p.reshape(-1) for p in planes[i % 4]])                 # what a caller does today: three full-frame host copies per pair
            b = np.concatenate([p.reshape(-1) for p in planes[(i + 1) % 4]])
            o = eng.process_yuv(a, b, w, h, timesteps[i % 5], px)
            for p, (rows, rb, off, _) in zip(outp, table):
                p[:] = o[off:off + rows * rb].reshape(rows, rb)

        say("4k I420 host frames (pageable), planes padded to 64-byte rows, ONE caller thread, %d pairs per run, %d repeats:" % (pairs, args.repeats))
        res = {"process_image": [], "numpy repack + process_px": []}
        for fn in (image_call, repack_call):
            fn(0); fn(1)
        for r in range(args.repeats):
            for label, fn in (("process_image", image_call), ("numpy repack + process_px", repack_call)):
                t0 = time.perf_counter()
                for i in range(pairs):
                    fn(i)
                res[label].append(pairs / (time.perf_counter() - t0))
        for label in res:
            say("   %-26s frames/s %s   median %.1f" % (label, " ".join("%.1f" % v for v in res[label]), float(np.median(res[label]))))
    say(json.dumps({"metric": "device image call >= 0.97 * the _px call on tight frames, every format and size (resident frames)", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
