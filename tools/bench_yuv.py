"""4:2:0 frames against RGB frames in the same process: what taking NV12 / P010 at the boundary costs (one extra streaming pass) and saves (half the bytes).

    python tools/bench_yuv.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--legs resident,host,cli] [--out profiles/yuv/yuv_bench.txt]

resident  bench.py's headline layout (tools/bench_deep.py): frames resident in HBM, four pairs in flight - four host threads, each driving one stream that owns half
          of the compute units - W untimed steps, K timed steps ended by a device synchronisation; A2B10G10R10, NV12 and P010 alternating, R repeats each.
          The bar: NV12 and P010 >= 0.97 of the A2B10G10R10 rate (the path they ride).  Then the kernel-class table of one profiled stretch per format, with
          the postproc_yuv class.
host      rife_hip_process_px on pageable host frames at 4K, NV12 against RGB8, from 1 and 2 caller threads (the reference's default -j 1:2:2).  No bar.
cli       rife-hip, a 4K C420jpeg .y4m file to a .y4m file, -j 1:2:2: frames/s of the pipeline (RIFE_HIP_CLI_TIMING).  No bar.
The exit code says whether the bar held."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
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
    ap.add_argument("--legs", default="resident,host,cli")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
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
    FMTS = [("A2B10G10R10", amd.PIX_A2B10G10R10), ("NV12", amd.PIX_NV12), ("P010", amd.PIX_P010)]

    def frames_of(w, h):
        """Four frames of the reference's real pair tiled, as 8-bit RGB, 10-bit RGB codes and the two YUV formats (made from the 10-bit codes)."""
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        out = {"RGB8": [], "A2B10G10R10": [], "NV12": [], "P010": []}
        for i in range(4):
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))
            codes = (f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16)
            out["RGB8"].append(f8)
            out["A2B10G10R10"].append(amd.pack_a2b10g10r10(codes))
            out["NV12"].append(yr.rgb10_to_yuv(codes, yr.PIX_NV12))
            out["P010"].append(yr.rgb10_to_yuv(codes, yr.PIX_P010))
        return out

    if "resident" in legs:
        streams = [eng.stream_create(i % 2, 2) for i in range(4)]
        for name in args.sizes.split(","):
            w, h = SIZES[name]
            steps = args.steps or (240 if name == "4k" else 600)
            host = frames_of(w, h)
            fr = {n: [torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda() for x in host[n]] for n, _ in FMTS}
            outs = {n: [torch.empty_like(fr[n][0]) for _ in range(4)] for n, _ in FMTS}
            fmt = dict(FMTS)

            def step(n, i):
                s = i % 4
                eng.process_device(fr[n][i % 4].data_ptr(), fr[n][(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[n][s].data_ptr(), streams[s], pixfmt=fmt[n])

            def run_steps(n, first, count):
                def worker(s):
                    torch.cuda.set_device(0)
                    for i in range(first, first + count):
                        if i % 4 == s:
                            step(n, i)
                th = [threading.Thread(target=worker, args=(s,)) for s in range(4)]
                [t.start() for t in th]
                [t.join() for t in th]

            def timed(n):
                run_steps(n, 0, 4)
                for i in range(args.warmup):
                    step(n, i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(n, args.warmup, steps)
                torch.cuda.synchronize()
                return steps / (time.perf_counter() - t0)

            res = {n: [] for n, _ in FMTS}
            for r in range(args.repeats):
                for n, _ in FMTS:
                    res[n].append(timed(n))
            med = {n: float(np.median(res[n])) for n in res}
            say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, steps, args.repeats))
            for n, _ in FMTS:
                say("   %-12s  frames/s %s   median %.1f   ratio %.4f%s" % (n, " ".join("%.1f" % v for v in res[n]), med[n], med[n] / med["A2B10G10R10"],
                                                                         "" if n == "A2B10G10R10" else " (bar 0.97)"))
                ok = ok and med[n] >= 0.97 * med["A2B10G10R10"]
            prof = {}
            for n, _ in FMTS:
                eng.profile_enable(True)
                for i in range(32):
                    step(n, i)
                torch.cuda.synchronize()
                prof[n] = eng.profile_read()
                eng.profile_enable(False)
            say("   kernel classes, ms per pair (32 profiled pairs):   class  A2B10G10R10  NV12  P010")
            classes = sorted(set().union(*[set(p) for p in prof.values()]), key=lambda c: -max(p.get(c, {"ms": 0.0})["ms"] for p in prof.values()))
            for cls in classes:
                say("      %-14s %s" % (cls, " ".join("%8.4f" % (prof[n].get(cls, {"ms": 0.0})["ms"] / 32) for n, _ in FMTS)))
            say("      %-14s %s" % ("total", " ".join("%8.4f" % (sum(v["ms"] for v in prof[n].values()) / 32) for n, _ in FMTS)))
            del fr, outs
            torch.cuda.empty_cache()

    if "host" in legs:
        w, h = SIZES["4k"]
        host = frames_of(w, h)
        pairs = 48
        say("4k host frames (pageable), rife_hip_process_px, %d pairs per run, %d repeats:" % (pairs, args.repeats))
        for nthr in (1, 2):
            for n, px in (("RGB8", amd.PIX_RGB8), ("NV12", amd.PIX_NV12)):
                bufs = [np.empty_like(host[n][0]) for _ in range(nthr)]

                def call(i, s):
                    if px == amd.PIX_RGB8:
                        eng.process(host[n][i % 4], host[n][(i + 1) % 4], timesteps[i % 5], outimage=bufs[s])
                    else:
                        eng.process_yuv(host[n][i % 4], host[n][(i + 1) % 4], w, h, timesteps[i % 5], px, out=bufs[s])

                def run(count):
                    def worker(s):
                        torch.cuda.set_device(0)
                        for i in range(s, count, nthr):
                            call(i, s)
                    th = [threading.Thread(target=worker, args=(s,)) for s in range(nthr)]
                    [t.start() for t in th]
                    [t.join() for t in th]

                run(2 * nthr)
                rates = []
                for r in range(args.repeats):
                    t0 = time.perf_counter()
                    run(pairs)
                    rates.append(pairs / (time.perf_counter() - t0))
                say("   %d caller thread(s)  %-5s frames/s %s   median %.1f   (%.1f MB per frame)" % (nthr, n, " ".join("%.1f" % v for v in rates), float(np.median(rates)),
                                                                                                host[n][0].nbytes / 1e6))

    if "cli" in legs:
        exe = os.path.join(ROOT, "rife-ncnn-vulkan_amd", "rife-hip")
        w, h = SIZES["4k"]
        host = frames_of(w, h)
        count = 24
        with tempfile.TemporaryDirectory() as t:
            src, dst = os.path.join(t, "in.y4m"), os.path.join(t, "out.y4m")
            with open(src, "wb") as f:
                f.write(b"YUV4MPEG2 W%d H%d F24:1 Ip A1:1 C420jpeg\n" % (w, h))
                for i in range(count):
                    y, cb, cr = yr.split(host["NV12"][i % 4], w, h, yr.PIX_NV12)
                    f.write(b"FRAME\n" + yr.pack(y, cb, cr, yr.PIX_I420).tobytes())
            rates = []
            for r in range(args.repeats):
                p = subprocess.run([exe, "-i", src, "-o", dst, "-m", model, "-j", "1:2:2"], capture_output=True, text=True, env=dict(os.environ, RIFE_HIP_CLI_TIMING="1"), timeout=300)
                tl = [l for l in p.stderr.splitlines() if l.startswith("timing: devices")]
                if p.returncode != 0 or not tl:
                    say("   rife-hip failed (%d): %s" % (p.returncode, p.stderr[-300:]))
                    ok = False
                    break
                rates.append(float(tl[0].split("=")[-1].split()[0]))
            if rates:
                say("4k rife-hip, %d-frame C420jpeg .y4m file to .y4m file (%d output frames), -j 1:2:2:  pipeline frames/s %s   median %.1f" %
                    (count, 2 * count, " ".join("%.1f" % v for v in rates), float(np.median(rates))))
    say(json.dumps({"metric": "NV12 and P010 >= 0.97 * A2B10G10R10 at every size (resident frames)", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
