"""High bit depth (include/rife_hip.h "high bit depth") against the sets call it is defined by, in the same process: what making the ten-bit proxy on the device
costs or saves.

    python tools/bench_hbd.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--host-steps N] [--out profiles/hbd/bench.txt]

tools/bench_apply_scaled.py's layout: planes and frames resident in HBM, four pairs in flight - four host threads, each driving one stream of rife_hip_stream_create
that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  Legs, alternating, R repeats each, per format (12-bit 4:2:0,
12-bit 4:2:2, 16-bit 4:4:4):
  (a) sets on proxies    rife_hip_process_device_apply_sets on PRE-MADE resident ten-bit proxy frames (the host work of reducing and packing them is not in the leg) and
                         the planes: the yardstick, no new code in it
  (b) hbd, two launches  rife_hip_process_device_hbd on the planes alone with RIFE_HIP_APPLY_YUV=0: the same device work as (a) with the proxy's plane read folded into the
                         pre-processing and no post-processing launch of the proxy
  (c) hbd, fused launch  the same call as it ships: luma and chroma of a subsampled image in ONE launch of k_apply_yuv (csrc/apply_yuv.h); not run for 4:4:4, which has
                         no such launch
All three legs run on the TEST build of the library (the same sources and kernels; only it reads the switch, per call).
Checked, and decides the exit code: (b) >= 0.97 x (a) per format and size (the project's bar for a format; boxes differ by +- 3 %, legs of one process by less), and
before the timing the planes of (b) and (c) are byte for byte those of (a) on the bench inputs.  Reported for the decision whether the fused launch stays: (c) / (b)
next to the spread of the repeated (b) legs of the same run, and from the profiler's events the fused launch next to the sum of the two launches it replaces.
For the record only (no condition): one caller thread, 4K 12-bit 4:2:0 in pageable host memory - rife_hip_process_hbd against numpy reduce-and-pack around
rife_hip_process_apply_sets, which is what a caller had to do before."""
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


def planes_from_rgb8(f, depth, cls):
    """bench input, not a colour conversion anybody relies on: BT.709 limited-range Y'CbCr at `depth` bits from an RGB8 frame, chroma box-averaged to the layout"""
    r, g, b = (f[..., k].astype(np.float32) / 255 for k in range(3))
    y = 0.2126 * r + 0.7152 * g + 0.0722 * b
    s = float(1 << (depth - 8))
    cb, cr = (b - y) / 1.8556, (r - y) / 1.5748
    h, w = y.shape
    if cls in (1, 2):
        cb = cb.reshape(h, w // 2, 2).mean(2); cr = cr.reshape(h, w // 2, 2).mean(2)
    if cls == 1:
        cb = cb.reshape(h // 2, 2, w // 2).mean(1); cr = cr.reshape(h // 2, 2, w // 2).mean(1)
    q = lambda v: np.ascontiguousarray(np.clip(np.rint(v), 0, (1 << depth) - 1).astype(np.uint16))
    return [q((16 + 219 * y) * s), q((128 + 224 * cb) * s), q((128 + 224 * cr) * s)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="timed steps per repeat (default: 240 at 4K, 600 at 1080p)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--host-steps", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hbd_ref as hr
    eng = amd.test_build().RIFE(0, rife_v4=True)      # the test build: RIFE_HIP_APPLY_YUV is read there, per call
    eng.load(gen_models.ensure(None, "rife-v4.6"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    FORMATS = [("12-bit 4:2:0", amd.PIX_I420P10, 12, 1), ("12-bit 4:2:2", amd.PIX_I422P10, 12, 2), ("16-bit 4:4:4", amd.PIX_I444P10, 16, 3)]
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    up = lambda a: torch.from_numpy(a.view(np.int16)).cuda()
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        f8 = [np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))[:h, :w] for i in range(4)]
        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), planes and proxies resident:" % (name, w, h, steps, args.repeats))
        for fname, pixfmt, depth, cls in FORMATS:
            maxval = (1 << depth) - 1
            host = [planes_from_rgb8(f, depth, cls) for f in f8]
            src = [[up(p) for p in ps] for ps in host]                                           # four frames of three planes
            dst = [[torch.zeros_like(p) for p in src[0]] for _ in range(4)]                      # one output per pair in flight
            prox = [up(hr.proxy_frame(ps, depth)) for ps in host]
            pout = [torch.empty_like(prox[0]) for _ in range(4)]
            img = lambda ts: amd.device_image(w, h, pixfmt, [(t.data_ptr(), t.stride(0) * 2) for t in ts])
            simg, dimg = [img(ts) for ts in src], [img(ts) for ts in dst]

            def desc(ts, first, n):
                return amd.planes_desc(ts[first].shape[1], ts[first].shape[0], amd.SAMPLE_U16, [(ts[k].data_ptr(), ts[k].stride(0) * 2) for k in range(first, first + n)], maxval)

            def sets(i0, i1, s):
                if pixfmt in hr.SHIFT:
                    return [amd.apply_set_desc(desc(src[i0], 0, 1), desc(src[i1], 0, 1), desc(dst[s], 0, 1), (0, 0)),
                            amd.apply_set_desc(desc(src[i0], 1, 2), desc(src[i1], 1, 2), desc(dst[s], 1, 2), hr.SHIFT[pixfmt])]
                return [amd.apply_set_desc(desc(src[i0], 0, 3), desc(src[i1], 0, 3), desc(dst[s], 0, 3), (0, 0))]

            allsets = {(i % 4, (i + 1) % 4, i % 4): sets(i % 4, (i + 1) % 4, i % 4) for i in range(4)}
            LEGS = ["(a) sets on proxies", "(b) hbd, two launches"] + (["(c) hbd, fused launch"] if pixfmt in hr.SHIFT else [])

            def select(leg):      # between legs, with nothing in flight
                os.environ["RIFE_HIP_APPLY_YUV"] = "0" if leg == LEGS[1] else "1"

            def step(leg, i, stream="part"):
                s = i % 4
                st = streams[s] if stream == "part" else stream
                i0, i1, t = i % 4, (i + 1) % 4, timesteps[i % 5]
                if leg == LEGS[0]:
                    eng.process_device_apply_sets(prox[i0].data_ptr(), prox[i1].data_ptr(), w, h, t, pout[s].data_ptr(), allsets[(i0, i1, s)], stream=st, pixfmt=pixfmt)
                else:
                    eng.process_device_hbd(simg[i0], simg[i1], t, dimg[s], depth, stream=st)

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
                select(leg)
                run_steps(leg, 0, 4)
                for i in range(args.warmup):
                    step(leg, i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(leg, args.warmup, steps)
                torch.cuda.synchronize()
                return steps / (time.perf_counter() - t0)

            got = []
            for leg in LEGS:      # the contract first, on these inputs
                for t in dst[0]:
                    t.zero_()
                select(leg)
                step(leg, 0, None); torch.cuda.synchronize()
                got.append([t.clone() for t in dst[0]])
            same = all(bool(torch.equal(a, b)) for g in got[1:] for a, b in zip(got[0], g)) and any(bool(t.any()) for t in got[0])
            ok = ok and same
            res = {leg: [] for leg in LEGS}
            for r in range(args.repeats):
                for leg in LEGS:
                    res[leg].append(timed(leg))
            med = {leg: float(np.median(res[leg])) for leg in LEGS}
            ratio = med[LEGS[1]] / med[LEGS[0]]
            spread = (max(res[LEGS[0]]) - min(res[LEGS[0]])) / med[LEGS[0]]
            held = ratio >= 0.97
            ok = ok and held
            say("   %s" % fname)
            say("      %-22s frames/s %s  median %.1f (spread of the repeats %.2f %%)" % (LEGS[0], " ".join("%.1f" % v for v in res[LEGS[0]]), med[LEGS[0]], 100 * spread))
            say("      %-22s frames/s %s  median %.1f | ratio to (a) %.4f (bar 0.97): %s | planes of every hbd leg byte for byte those of (a): %s" % (
                LEGS[1], " ".join("%.1f" % v for v in res[LEGS[1]]), med[LEGS[1]], ratio, "holds" if held else "DOES NOT HOLD", same))
            if len(LEGS) == 3:
                bspread = (max(res[LEGS[1]]) - min(res[LEGS[1]])) / med[LEGS[1]]
                gain = med[LEGS[2]] / med[LEGS[1]] - 1.0
                say("      %-22s frames/s %s  median %.1f | against (b) %+.2f %%, spread of the repeated (b) legs %.2f %%: the fused launch %s" % (
                    LEGS[2], " ".join("%.1f" % v for v in res[LEGS[2]]), med[LEGS[2]], 100 * gain, 100 * bspread, "WINS" if gain > bspread else "DOES NOT WIN"))
            # the launches of one pair, from the profiler's events (the engine's own stream, whole chip)
            for leg in LEGS:
                select(leg)
                for i in range(2):
                    step(leg, i, None)
                eng.profile_enable(True)
                for i in range(8):
                    step(leg, i, None)
                torch.cuda.synchronize()
                prof = eng.profile_read()
                eng.profile_enable(False)
                keys = [k for k in ("preproc", "postproc_yuv", "apply_motion", "apply_motion_down", "apply_yuv") if k in prof and prof[k]["launches"]]
                say("      %-22s ms per pair: %s | apply launches together %.4f | all classes %.3f" % (
                    leg, ", ".join("%s %.4f" % (k, prof[k]["ms"] / 8) for k in keys), sum(prof[k]["ms"] for k in keys if k.startswith("apply")) / 8, sum(v["ms"] for v in prof.values()) / 8))
            os.environ.pop("RIFE_HIP_APPLY_YUV", None)
            del src, dst, prox, pout, got
            torch.cuda.empty_cache()
        if name == "4k" and args.host_steps > 0:      # for the record: the host path, one caller thread, pageable memory
            fname, pixfmt, depth, cls = FORMATS[0]
            host = [planes_from_rgb8(f, depth, cls) for f in f8[:2]]
            out = tuple(np.empty_like(p) for p in host[0])
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

            def old():
                f0, f1 = hr.proxy_frame(host[0], depth), hr.proxy_frame(host[1], depth)
                n, arr = amd._set_array(hr.make_sets(host[0], host[1], depth, pixfmt, out))
                assert eng._L.rife_hip_process_apply_sets(eng._h, p(f0), p(f1), w, h, 0.5, None, pixfmt, n, arr) == 0

            def new():
                eng.process_hbd(tuple(host[0]), tuple(host[1]), 0.5, depth, pixfmt, out=out)

            rates = {}
            for nm, fn in (("numpy reduce-and-pack + process_apply_sets", old), ("process_hbd", new)) * 2:
                fn()
                t0 = time.perf_counter()
                for i in range(args.host_steps):
                    fn()
                rates.setdefault(nm, []).append(args.host_steps / (time.perf_counter() - t0))
            say("   host path, for the record (one caller thread, %s in pageable memory, %d calls x 2):" % (fname, args.host_steps))
            for nm, v in rates.items():
                say("      %-44s frames/s %s" % (nm, " ".join("%.1f" % x for x in v)))
        del f8, base
    say(json.dumps({"metric": "process_device_hbd writes the planes of process_device_apply_sets on the bench inputs and runs at >= 0.97 of it, per format and size", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
