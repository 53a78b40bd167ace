"""Packed 16-bit frames (include/rife_hip.h rife_hip_packed_t) against the planar paths that existed before them, in the same process.

    python tools/bench_packed.py [--steps K] [--warmup W] [--repeats R] [--sizes 4k,1080p] [--out profiles/packed/bench.txt]

tools/bench_apply.py's layout: frames resident in HBM, four pairs in flight - four host threads, each driving one stream of rife_hip_stream_create that owns half of
the compute units - W untimed steps, K timed steps ended by a device synchronisation; legs alternating, R repeats each.  Depth 16, the same samples in every leg:
    hbd RGBP10 planes      rife_hip_process_device_hbd on the three de-interleaved planes                                (yardstick of packed RGB)
    packed RGB             rife_hip_process_device_hbd_packed, 3 channels
    sets 4 planes          rife_hip_process_device_apply_sets on pre-made RGBP10 proxies with one four-plane set         (yardstick of packed RGBA; it is GIVEN its proxies)
    packed RGBA            rife_hip_process_device_hbd_packed, 4 channels
Expectation: a packed leg is not slower than its yardstick by more than the spread (max - min) of the yardstick's repeats.
Before the timing the contract must hold on the bench inputs: the packed frame is byte for byte the interleaved planes of its yardstick.
Then the kernels alone, one pair at a time on the engine's own stream with the profiler's events around every launch, on the motion the engine estimates for these
frames: apply_packed against apply_motion (k_apply_motion<uint16_t>, n = 3 and n = 4; bar: no longer than the planar launch plus 10 %), and the two preproc_packed
launches of a call against the two k_preproc_hbd_rgb_x8 launches (class preproc) of the hbd call on the same samples.
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
LEGS = ["hbd RGBP10 planes", "packed RGB", "sets 4 planes", "packed RGBA"]
YARD = {"packed RGB": "hbd RGBP10 planes", "packed RGBA": "sets 4 planes"}


def reduce10(v, depth):
    c = (v.astype(np.uint32) + (1 << (depth - 11))) >> (depth - 10) if depth > 10 else v.astype(np.uint32)
    return np.minimum(c, 1023).astype(np.uint16)


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
    depth, maxval = 16, 65535
    timesteps = [0.5, 0.125, 0.25, 0.7, 0.9]
    streams = [eng.stream_create(i % 2, 2) for i in range(4)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        steps = args.steps or (240 if name == "4k" else 600)
        base = gen_frames.tiled_real_pair(w // 640)
        rng = np.random.default_rng(7)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        rgba = []
        for i in range(4):      # the scene of bench_apply.py at 16 bits with sub-code noise, plus a moving soft matte
            f = np.ascontiguousarray(np.roll(base[i % 2], (2 * (i // 2), 5 * (i // 2)), axis=(0, 1)))[:h, :w].astype(np.int32) * 257 + rng.integers(-128, 129, (h, w, 3))
            al = np.clip(0.5 + 0.7 * np.sin((xx + 3.0 * i) / 90.0) * np.cos((yy + 2.0 * i) / 70.0), 0, 1) * maxval
            rgba.append(np.concatenate([np.clip(f, 0, maxval), al[..., None]], axis=2).astype(np.uint16))
        pk = {3: [dev(f[..., :3]) for f in rgba], 4: [dev(f) for f in rgba]}                        # (h, w, ch)
        pl = [dev(np.moveaxis(f, -1, 0)) for f in rgba]                                              # (4, h, w)
        px = [dev(np.stack([reduce10(f[..., k], depth) for k in range(3)])) for f in rgba]          # tight RGBP10 proxies
        pk_out = {ch: [torch.empty_like(pk[ch][0]) for _ in range(4)] for ch in (3, 4)}
        pl_out = [torch.empty_like(pl[0]) for _ in range(4)]
        px_out = [torch.empty_like(px[0]) for _ in range(4)]
        pdesc = lambda t, ch: amd.packed_desc(w, h, ch, depth, t.data_ptr(), w * ch * 2)
        idesc = lambda t: amd.device_image(w, h, amd.PIX_RGBP10, [(t[k].data_ptr(), w * 2) for k in range(3)])
        sdesc = lambda t: amd.planes_desc(w, h, amd.SAMPLE_U16, [(t[k].data_ptr(), w * 2) for k in range(4)], maxval)

        def step(leg, i, stream="part"):
            s = i % 4
            st = streams[s] if stream == "part" else stream
            a, b, t = i % 4, (i + 1) % 4, timesteps[i % 5]
            if leg == "hbd RGBP10 planes":
                eng.process_device_hbd(idesc(pl[a]), idesc(pl[b]), t, idesc(pl_out[s]), depth, stream=st)
            elif leg == "sets 4 planes":
                sets = [amd.apply_set_desc(sdesc(pl[a]), sdesc(pl[b]), sdesc(pl_out[s]), (0, 0))]
                eng.process_device_apply_sets(px[a].data_ptr(), px[b].data_ptr(), w, h, t, px_out[s].data_ptr(), sets, stream=st, pixfmt=amd.PIX_RGBP10)
            else:
                ch = 3 if leg == "packed RGB" else 4
                eng.process_device_hbd_packed(pdesc(pk[ch][a], ch), pdesc(pk[ch][b], ch), t, pdesc(pk_out[ch][s], ch), stream=st)

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

        say("%s %dx%d, depth 16, %d steps x %d repeats, four pairs in flight (two per half of the compute units), frames resident:" % (name, w, h, steps, args.repeats))
        same = {}
        for leg, yard in YARD.items():      # the contract first
            ch = 3 if leg == "packed RGB" else 4
            pl_out[0].zero_(); pk_out[ch][0].zero_()
            step(yard, 0, None); step(leg, 0, None); torch.cuda.synchronize()
            want = pl_out[0][:ch].permute(1, 2, 0).contiguous()
            same[leg] = bool(torch.equal(pk_out[ch][0], want)) and bool((want != pk[ch][0]).any())
        res = {leg: [] for leg in LEGS}
        for r in range(args.repeats):
            for leg in LEGS:
                res[leg].append(timed(leg))
        med = {leg: float(np.median(res[leg])) for leg in LEGS}
        for leg in LEGS:
            line = "   %-18s frames/s %s  median %.1f" % (leg, " ".join("%.1f" % v for v in res[leg]), med[leg])
            if leg in YARD:
                y = YARD[leg]
                spread = max(res[y]) - min(res[y])
                held = med[leg] >= med[y] - spread
                line += " | ratio to '%s' %.4f, its spread %.1f frames/s: %s | the contract holds on these inputs: %s" % (y, med[leg] / med[y], spread, "not slower" if held else "SLOWER", same[leg])
                ok = ok and same[leg] and held
            say(line)
        say("   the kernels alone (one pair at a time, whole chip; profiler events around each launch), 16 pairs per leg, ms per call:")
        prof = {}
        for leg in LEGS:
            for i in range(2):
                step(leg, i, None)
            eng.profile_enable(True)
            for i in range(16):
                step(leg, i, None)
            torch.cuda.synchronize()
            p = eng.profile_read()
            eng.profile_enable(False)
            prof[leg] = {k: v["ms"] / 16 for k, v in p.items() if v["launches"]}
        for leg, yard in YARD.items():
            ch = 3 if leg == "packed RGB" else 4
            a_new, a_old = prof[leg]["apply_packed"], prof[yard]["apply_motion"]
            held = a_new <= 1.10 * a_old
            ok = ok and held
            nbytes = (20.0 + 3 * ch * 2) * w * h
            say("      blend, %d channels     apply_packed %.4f ms (%.2f TB/s of %d B per pixel) | k_apply_motion<u16> n = %d %.4f ms | ratio %.3f (bar 1.10): %s" %
                (ch, a_new, nbytes / (a_new * 1e-3) / 1e12, int(nbytes / (w * h)), ch, a_old, a_new / a_old, "held" if held else "MISSED"))
        say("      pre-processing, both inputs   preproc_packed RGB %.4f ms, RGBA %.4f ms | k_preproc_hbd_rgb_x8 (class preproc of the hbd call) %.4f ms" %
            (prof["packed RGB"]["preproc_packed"], prof["packed RGBA"]["preproc_packed"], prof["hbd RGBP10 planes"]["preproc"]))
        for leg in LEGS:
            tot = sum(prof[leg].values())
            top = sorted(prof[leg].items(), key=lambda kv: -kv[1])[:6]
            say("      %-18s all classes %.3f ms per call; largest: %s" % (leg, tot, ", ".join("%s %.3f" % kv for kv in top)))
        del pk, pl, px, pk_out, pl_out, px_out
        torch.cuda.empty_cache()
    say(json.dumps({"metric": "packed call not slower than its planar yardstick by more than the yardstick's spread, the contract holds, apply_packed within 1.10 of k_apply_motion<u16>", "ok": bool(ok)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
