"""Apply motion at another resolution (include/rife_hip.h rife_hip_apply_set_t) against the motion call in the same process: what applying one motion to 4:2:0 planes,
or a half-size estimate to full-size planes, costs.

    python tools/bench_apply_scaled.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/apply_scaled/bench.txt]

tools/bench_apply.py's layout: frames, planes and motion resident in HBM, four pairs in flight - four host threads, each driving one stream of rife_hip_stream_create
that owns half of the compute units - W untimed steps, K timed steps ended by a device synchronisation.  Legs on RGB8 frames, alternating, R repeats each:
  motion F32          rife_hip_process_device_motion with F32 buffers (the yardstick)
  apply 3 x T         rife_hip_process_device_apply with 3 full-size planes of u8 / u16 / float
  4:2:0 T             rife_hip_process_device_apply_sets with a luma set (n 1, shift 0, 0) and a chroma set (n 2, shift -1, -1): half the plane bytes of 3 full planes,
                      the motion read twice
  proxy -> 2x u8      (at 1080p only) the 1080p estimate applied to 3 u8 planes of 3840x2160 (shift +1, +1); its yardstick is the 4K motion call of the 4K section
Reported: the ratio of every leg to motion F32 of the same run.  Before the timing the contract must hold on the bench inputs: frame and planes of the sets call are
byte for byte process_device_motion then apply_device_motion_sets.
Then the kernels alone: apply_device_motion_sets on the engine's own stream, the profiler's events around every launch - milliseconds per launch of the classes
apply_motion (unscaled, n 2), apply_motion_down (4:2:0 chroma, n 2) and apply_motion_up (n 2, planes twice the motion) on the SAME motion and sample type, for the
engine's motion on the bench frames (the synthetic weights give a field that jumps several pixels between neighbours) and for a smooth field, next to the byte
model of each launch (motion 20 B per motion pixel, 3 n es per plane pixel) evaluated at the rate the RGBPF post-processing kernel (16 B per pixel) streams at in
the same run.
One expectation is checked and decides the exit code: the 4:2:0 chroma launch reads the same motion bytes as the unscaled launch and reads and writes a quarter of
the plane bytes, so it takes no longer than the unscaled launch of the same n, motion and sample type, with a 10 % margin (these are 0.1 - 0.4 ms launches)."""
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
N = 3


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
    TYPES = {"u8": (amd.SAMPLE_U8, np.uint8, 255), "u16": (amd.SAMPLE_U16, np.uint16, 65535), "float": (amd.SAMPLE_F32, np.float32, 0)}
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    rng = np.random.default_rng(7)

    def dev_planes(n, h, w, dt, maxval):
        """n random planes on the device: (descriptor factory over a (n, h, row bytes) uint8 tensor, the tensor)"""
        es = np.dtype(dt).itemsize
        a = rng.integers(0, maxval + 1, (n, h, w)).astype(dt) if maxval else rng.random((n, h, w)).astype(dt)
        return torch.from_numpy(a.view(np.uint8).reshape(n, h, w * es)).cuda()

    def desc(t, w, h, sample, maxval, first=0, n=None):
        n = n if n is not None else t.shape[0] - first
        return amd.planes_desc(w, h, sample, [(t[first + k].data_ptr(), t.stride(1)) for k in range(n)], maxval or None)

    for name in args.sizes.split(","):
        w, h = SIZES[name]
        cw, ch = (w + 1) // 2, (h + 1) // 2
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        f8 = [np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))[:h, :w] for i in range(4)]
        fr = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in f8]
        outs = [torch.empty_like(fr[0]) for _ in range(4)]
        mo = []
        for s in range(4):      # tight F32 motion buffers, one set per pair in flight (the yardstick's)
            f = torch.empty((h, w * 16), dtype=torch.uint8, device="cuda"); m = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda")
            mo.append((amd.motion_desc(f.data_ptr(), m.data_ptr(), amd.MOTION_F32, w * 16, w * 4), f, m))
        ext = eng.padded_size(w, h)
        cext = (ext[0] // 2, ext[1] // 2)
        full, yuv = {}, {}
        for tn, (sample, dt, maxval) in TYPES.items():
            src = [dev_planes(N, h, w, dt, maxval) for _ in range(2)]
            dst = [torch.empty_like(src[0]) for _ in range(4)]
            full[tn] = ([desc(t, w, h, sample, maxval) for t in src], [desc(t, w, h, sample, maxval) for t in dst], src, dst)
            csrc = [dev_planes(2, ch, cw, dt, maxval) for _ in range(2)]
            cdst = [torch.empty_like(csrc[0]) for _ in range(4)]
            sets = [[amd.apply_set_desc(desc(src[0], w, h, sample, maxval, 0, 1), desc(src[1], w, h, sample, maxval, 0, 1), desc(dst[s], w, h, sample, maxval, 0, 1), (0, 0), ext),
                     amd.apply_set_desc(desc(csrc[0], cw, ch, sample, maxval), desc(csrc[1], cw, ch, sample, maxval), desc(cdst[s], cw, ch, sample, maxval), (-1, -1), cext)]
                    for s in range(4)]
            yuv[tn] = (sets, csrc, cdst)
        LEGS = ["motion F32"] + ["apply 3 x " + tn for tn in TYPES] + ["4:2:0 " + tn for tn in TYPES]
        up = None
        if name == "1080p":      # the proxy leg: this size's estimate on planes of twice the size
            W2, H2 = 2 * w, 2 * h
            usrc = [dev_planes(N, H2, W2, np.uint8, 255) for _ in range(2)]
            udst = [torch.empty_like(usrc[0]) for _ in range(4)]
            up = [[amd.apply_set_desc(desc(usrc[0], W2, H2, amd.SAMPLE_U8, 255), desc(usrc[1], W2, H2, amd.SAMPLE_U8, 255), desc(udst[s], W2, H2, amd.SAMPLE_U8, 255), (1, 1),
                                      (2 * ext[0], 2 * ext[1]))] for s in range(4)]
            LEGS.append("proxy -> 2x u8")

        def step(leg, i, stream="part"):
            s = i % 4
            st = streams[s] if stream == "part" else stream
            a, b, t, o = fr[i % 4].data_ptr(), fr[(i + 1) % 4].data_ptr(), timesteps[i % 5], outs[s].data_ptr()
            if leg == "motion F32":
                eng.process_device_motion(a, b, w, h, t, o, mo[s][0], stream=st)
            elif leg.startswith("apply 3 x "):
                d = full[leg[10:]]
                eng.process_device_apply(a, b, w, h, t, o, d[0][0], d[0][1], d[1][s], extent=ext, stream=st)
            elif leg.startswith("4:2:0 "):
                eng.process_device_apply_sets(a, b, w, h, t, o, yuv[leg[6:]][0][s], stream=st)
            else:
                eng.process_device_apply_sets(a, b, w, h, t, o, up[s], stream=st)

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

        say("%s %dx%d, %d steps x %d repeats, four pairs in flight (two per half of the compute units), RGB8 frames, planes and motion resident:" % (name, w, h, steps, args.repeats))
        same = {}
        for leg in LEGS:      # the contract first: the sets call == process_device_motion, then apply_device_motion_sets
            if not (leg.startswith("4:2:0") or leg.startswith("proxy")):
                continue
            sets = yuv[leg[6:]][0][0] if leg.startswith("4:2:0") else up[0]
            touched = [full[leg[6:]][3][0], yuv[leg[6:]][2][0]] if leg.startswith("4:2:0") else [udst[0]]
            for t in touched:
                t.zero_()
            step("motion F32", 0, None); torch.cuda.synchronize()
            want_frame = outs[0].clone()
            eng.apply_device_motion_sets(sets, mo[0][0], w, h)
            torch.cuda.synchronize()
            want = [t.clone() for t in touched]
            outs[0].zero_()
            for t in touched:
                t.zero_()
            step(leg, 0, None); torch.cuda.synchronize()
            same[leg] = bool(torch.equal(outs[0], want_frame)) and all(bool(torch.equal(a, b)) for a, b in zip(touched, want))
            ok = ok and same[leg]
        res = {leg: [] for leg in LEGS}
        for r in range(args.repeats):
            for leg in LEGS:
                res[leg].append(timed(leg))
        med = {leg: float(np.median(res[leg])) for leg in LEGS}
        say("   %-16s frames/s %s  median %.1f" % (LEGS[0], " ".join("%.1f" % v for v in res[LEGS[0]]), med[LEGS[0]]))
        for leg in LEGS[1:]:
            say("   %-16s frames/s %s  median %.1f | ratio to motion F32 %.4f%s" % (leg, " ".join("%.1f" % v for v in res[leg]), med[leg], med[leg] / med[LEGS[0]],
                                                                                  " | the contract holds on these inputs: %s" % same[leg] if leg in same else ""))
        # ---- the kernels alone ----
        say("   the kernels alone (one launch at a time on the engine's stream, whole chip; profiler events around each launch), 16 launches each, n = 2:")
        fpl = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(f, -1, 0)).astype(np.float32) / np.float32(255)).cuda() for f in f8[:2]]      # RGBPF frames for the streaming yardstick
        fo = torch.empty_like(fpl[0])
        for i in range(2):
            eng.process_device(fpl[0].data_ptr(), fpl[1].data_ptr(), w, h, 0.5, fo.data_ptr(), None, pixfmt=amd.PIX_RGBPF)
        eng.profile_enable(True)
        for i in range(16):
            eng.process_device(fpl[0].data_ptr(), fpl[1].data_ptr(), w, h, timesteps[i % 5], fo.data_ptr(), None, pixfmt=amd.PIX_RGBPF)
        torch.cuda.synchronize()
        post_ms = eng.profile_read()["postproc_rgbp"]["ms"] / 16
        eng.profile_enable(False)
        bw = 16.0 * w * h / (post_ms * 1e-3)
        say("      %-34s %.4f ms per launch, %.2f TB/s (16 B per pixel, streaming)" % ("postproc RGBPF", post_ms, bw / 1e12))
        del fpl, fo
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
        smooth_f = np.stack([3 * np.sin(xs / 97) * np.cos(ys / 61), 2.5 * np.cos(xs / 83) * np.sin(ys / 71), -3 * np.sin(xs / 89 + 1) * np.cos(ys / 67), 2 * np.cos(xs / 101) * np.cos(ys / 59)], axis=-1).astype(np.float32)
        smooth_m = (0.5 + 0.4 * np.sin(xs / 113) * np.sin(ys / 79)).astype(np.float32)
        del ys, xs
        sf = torch.from_numpy(smooth_f.view(np.uint8).reshape(h, w * 16)).cuda(); sm = torch.from_numpy(smooth_m.view(np.uint8).reshape(h, w * 4)).cuda()
        del smooth_f, smooth_m
        step("motion F32", 0, None); torch.cuda.synchronize()
        fields = {"engine": mo[0][0], "smooth": amd.motion_desc(sf.data_ptr(), sm.data_ptr(), amd.MOTION_F32, w * 16, w * 4)}
        for tn, (sample, dt, maxval) in TYPES.items():
            es = np.dtype(dt).itemsize
            src, dst = full[tn][2], full[tn][3]
            csrc, cdst = yuv[tn][1], yuv[tn][2]
            W2, H2 = 2 * w, 2 * h
            big = name == "1080p"      # the up launch needs planes of twice the motion: at 1080p only
            if big:
                bsrc = [dev_planes(2, H2, W2, dt, maxval) for _ in range(2)]; bdst = torch.empty_like(bsrc[0])
            launches = {
                "apply_motion": ([amd.apply_set_desc(desc(src[0], w, h, sample, maxval, 0, 2), desc(src[1], w, h, sample, maxval, 0, 2), desc(dst[0], w, h, sample, maxval, 0, 2), (0, 0), ext)], w * h),
                "apply_motion_down": ([amd.apply_set_desc(desc(csrc[0], cw, ch, sample, maxval), desc(csrc[1], cw, ch, sample, maxval), desc(cdst[0], cw, ch, sample, maxval), (-1, -1), cext)], cw * ch),
            }
            if big:
                launches["apply_motion_up"] = ([amd.apply_set_desc(desc(bsrc[0], W2, H2, sample, maxval), desc(bsrc[1], W2, H2, sample, maxval), desc(bdst, W2, H2, sample, maxval), (1, 1),
                                                                   (2 * ext[0], 2 * ext[1]))], W2 * H2)
            for fname, field in fields.items():
                got = {}
                for cls, (sets, plane_px) in launches.items():
                    for i in range(2):
                        eng.apply_device_motion_sets(sets, field, w, h)
                    eng.profile_enable(True)
                    for i in range(16):
                        eng.apply_device_motion_sets(sets, field, w, h)
                    torch.cuda.synchronize()
                    ms = eng.profile_read()[cls]["ms"] / 16
                    eng.profile_enable(False)
                    nbytes = 20.0 * w * h + 3 * 2 * es * plane_px
                    model_ms = nbytes / bw * 1e3
                    got[cls] = ms
                    say("      %-6s %-7s %-18s %.4f ms per launch | byte model %.0f MB, at the streaming rate %.4f ms, ratio %.2f" % (tn, fname, cls, ms, nbytes / 1e6, model_ms, ms / model_ms))
                held = got["apply_motion_down"] <= 1.10 * got["apply_motion"]
                say("      %-6s %-7s 4:2:0 chroma launch / unscaled launch (n 2, same motion): %.3f (expected <= 1.10): %s" % (tn, fname, got["apply_motion_down"] / got["apply_motion"], "holds" if held else "DOES NOT HOLD"))
                ok = ok and held
            if big:
                del bsrc, bdst
        del fr, outs, mo, full, yuv, up, sf, sm
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "the contract of the sets calls holds on the bench inputs; the 4:2:0 chroma launch takes no longer than 1.10 x the unscaled launch of the same n, motion and sample type", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
