"""Planar RGB frames (RGBP8 / RGBP10 / RGBPH / RGBPF) against the packed 10-bit format in the same process: what three planes of u8 .. float cost at the boundary.

    python tools/bench_planar.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--host-pairs N] [--out profiles/planar/planar_bench.txt]

bench.py's headline layout (tools/bench_chroma.py): frames resident in HBM, four pairs in flight - four host threads, each driving one stream of
rife_hip_stream_create that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  For each of the four formats:
rife_hip_process_device_px on tight frames, and rife_hip_process_device_image on planes in SEPARATE allocations whose rows are aligned to 256 bytes (never tight)
plus one row of slack; A2B10G10R10 on tight frames of the same scene is the yardstick.  The legs alternate, R repeats each.
The bars: RGBP8, RGBP10, RGBPH >= 0.97 of the A2B10G10R10 rate at every size; RGBPF (12 bytes per pixel and frame instead of 4) >= 0.95.  Before the timing, the
tight and the image call of a format must return the same bytes.
Then the new kernels alone: one pair at a time on the engine's own stream (the whole chip, nothing else in flight), the profiler's events around every launch -
milliseconds per pair of preproc (its two launches together) and of postproc_rgbp, and the bandwidth that is (bytes the launches must move / time).
Last, host planes: process_planes on RGBPF planes in pageable host memory from one caller thread, against what a caller had to do before - quantise and interleave
in numpy, process_px(A2B10G10R10), and undo it.  Both rates are recorded; there is no bar (PCIe and the host set them).
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
    ap.add_argument("--host-pairs", type=int, default=6, help="pairs per leg of the host-planes comparison (4K RGBPF); 0 skips it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import planar_ref as pr
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
    FMTS = [("RGBP8", amd.PIX_RGBP8), ("RGBP10", amd.PIX_RGBP10), ("RGBPH", amd.PIX_RGBPH), ("RGBPF", amd.PIX_RGBPF)]
    BAR = {"RGBP8": 0.97, "RGBP10": 0.97, "RGBPH": 0.97, "RGBPF": 0.95}
    fmt = dict(FMTS, **{REF: amd.PIX_A2B10G10R10})
    LEGS = [(REF, "tight")] + [(n, path) for n, _ in FMTS for path in ("tight", "image")]

    def codes_of(w, h):
        """Four frames of the reference's real pair tiled, as (h, w, 3) ten-bit codes."""
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        out = []
        for i in range(4):
            f8 = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))
            out.append((f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16))
        return out

    def frames_of(codes):
        """The same frames as tight frames (uint8 bytes) of each format."""
        return {n: [np.ascontiguousarray(amd.pack_a2b10g10r10(c) if n == REF else pr.from_rgb10(c, fmt[n])).view(np.uint8).reshape(-1) for c in codes] for n in fmt}

    class Planes:
        """One frame in device memory as separate allocations per plane, rows aligned to 256 bytes, one row of slack after the last."""

        def __init__(self, tight, w, h, px):
            self.t = []
            planes = []
            rb = amd.image_row_bytes(w, px, 0)
            for p in range(3):
                pitch = (rb + 255) // 256 * 256
                if pitch == rb:
                    pitch += 256                               # never tight: a tight image IS the _px call and would measure nothing
                host = np.zeros((h + 1, pitch), np.uint8)
                if tight is not None:
                    host[:h, :rb] = tight[p * h * rb:(p + 1) * h * rb].reshape(h, rb)
                t = torch.from_numpy(host).cuda()
                self.t.append(t)
                planes.append((t.data_ptr(), pitch))
            self.desc = amd.device_image(w, h, px, planes)

    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        wp, hp = (w + 31) // 32 * 32, (h + 31) // 32 * 32
        steps = args.steps or (240 if name == "4k" else 600)
        codes = codes_of(w, h)
        host = frames_of(codes)
        fr = {n: [torch.from_numpy(x).cuda() for x in host[n]] for n in fmt}
        outs = {n: [torch.empty_like(fr[n][0]) for _ in range(4)] for n in fmt}
        pl = {n: [Planes(x, w, h, fmt[n]) for x in host[n]] for n, _ in FMTS}
        plo = {n: [Planes(None, w, h, fmt[n]) for _ in range(4)] for n, _ in FMTS}

        def step(leg, i, stream="part"):
            n, path = leg
            s = i % 4
            st = streams[s] if stream == "part" else stream
            if path == "image":
                eng.process_device_image(pl[n][i % 4].desc, pl[n][(i + 1) % 4].desc, timesteps[i % 5], plo[n][s].desc, st)
            else:
                eng.process_device(fr[n][i % 4].data_ptr(), fr[n][(i + 1) % 4].data_ptr(), w, h, timesteps[i % 5], outs[n][s].data_ptr(), st, pixfmt=fmt[n])

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
            rb = amd.image_row_bytes(w, fmt[n], 0)
            for s in range(4):
                tight = outs[n][s].cpu().numpy()
                for p, t in enumerate(plo[n][s].t):
                    same[n] = same[n] and np.array_equal(t.cpu().numpy()[:h, :rb].reshape(-1), tight[p * h * rb:(p + 1) * h * rb])
        res = {leg: [] for leg in LEGS}
        for r in range(args.repeats):
            for leg in LEGS:
                res[leg].append(timed(leg))
        med = {leg: float(np.median(res[leg])) for leg in LEGS}
        ref = med[(REF, "tight")]
        say("   %-20s frames/s %s  median %.1f" % (REF + " tight", " ".join("%.1f" % v for v in res[(REF, "tight")]), ref))
        for leg in LEGS[1:]:
            bar = BAR[leg[0]]
            say("   %-20s frames/s %s  median %.1f | ratio to %s %.4f (bar %.2f) | tight and image return the same bytes: %s" %
                ("%s %s" % leg, " ".join("%.1f" % v for v in res[leg]), med[leg], REF, med[leg] / ref, bar, same[leg[0]]))
            ok = ok and same[leg[0]] and med[leg] >= bar * ref
        # the kernels alone: one pair at a time on the engine's own stream, which synchronises before it returns
        say("   the boundary kernels alone (one pair at a time, whole chip; profiler events around each launch), 16 pairs per leg:")
        say("      %-16s %12s %10s %14s %10s" % ("leg", "preproc ms", "GB/s", "postproc ms", "GB/s"))
        for leg in LEGS:
            n = leg[0]
            for i in range(2):
                step(leg, i, None)
            eng.profile_enable(True)
            for i in range(16):
                step(leg, i, None)
            torch.cuda.synchronize()
            prof = eng.profile_read()
            eng.profile_enable(False)
            es = 4 if n == REF else amd.frame_bytes(1, 1, fmt[n]) // 3
            pre = prof.get("preproc", {"ms": 0.0})["ms"] / 16                      # two launches per pair: both frames
            pre_bytes = 2 * ((w * h * 4 if n == REF else 3 * w * h * es) + wp * hp * 4)
            post = prof.get("postproc_rgbp", {"ms": 0.0})["ms"] / 16
            post_bytes = w * h * 4 + 3 * w * h * es
            say("      %-16s %12.4f %10.0f %14s %10s" % ("%s %s" % leg, pre, pre_bytes / pre / 1e6 if pre else 0.0,
                                                        "%.4f" % post if post else "-", "%.0f" % (post_bytes / post / 1e6) if post else "-"))
        if name == "4k" and args.host_pairs > 0:
            # host planes: three float32 planes per frame in pageable memory, one caller thread
            n = args.host_pairs
            fa = [tuple(np.array(p) for p in pr.from_rgb10(c, amd.PIX_RGBPF)) for c in codes[:2]]      # three allocations per frame, as a VapourSynth RGBS frame has
            out = tuple(np.empty_like(p) for p in fa[0])
            eng.process_planes(fa[0], fa[1], 0.5, amd.PIX_RGBPF, out=out)
            t0 = time.perf_counter()
            for i in range(n):
                eng.process_planes(fa[i % 2], fa[(i + 1) % 2], timesteps[i % 5], amd.PIX_RGBPF, out=out)
            planes_rate = n / (time.perf_counter() - t0)

            def repack(f):      # what a caller of the packed format does per frame: quantise, interleave, pack
                c = [(np.clip(p, 0, 1) * np.float32(1023) + np.float32(0.5)).astype(np.uint32) for p in f]
                return c[0] | (c[1] << 10) | (c[2] << 20)
            packed_out = np.empty((h, w), np.uint32)
            t0 = time.perf_counter()
            for i in range(n):
                eng.process(repack(fa[i % 2]), repack(fa[(i + 1) % 2]), timesteps[i % 5], outimage=packed_out)
                back = np.stack([packed_out & 1023, (packed_out >> 10) & 1023, (packed_out >> 20) & 1023]).astype(np.float32) / np.float32(1023)
            repack_rate = n / (time.perf_counter() - t0)
            say("   host planes, 4K RGBPF, one caller thread, pageable memory, %d pairs: process_planes %.2f frames/s | numpy quantise + interleave around"
                " process_px(A2B10G10R10) %.2f frames/s | same bytes: %s (no bar: PCIe and the host set both)" % (n, planes_rate, repack_rate, all(np.array_equal(x, y) for x, y in zip(back, out))))
        del fr, outs, pl, plo
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "RGBP8 / RGBP10 / RGBPH >= 0.97 and RGBPF >= 0.95 of A2B10G10R10, tight frames and pitched planes, at every size (resident frames)", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
