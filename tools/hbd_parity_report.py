"""High bit depth against the ten-bit path on the SAME picture, reported and not asserted: what a caller gains and loses by handing 12- or 16-bit planes to
rife_hip_process_hbd instead of rounding them to ten bits for rife_hip_process_image.

    python tools/hbd_parity_report.py [--out profiles/hbd/parity.txt]

Frames are ten-bit Y'CbCr pairs (tools/gen_frames.py pairs, converted by tools/bench_hbd.py planes_from_rgb8) shifted up to the depth, c10 << 2 and c10 << 6, so both
paths estimate the SAME motion (the hbd proxy of c10 << k is c10 again).  Reported per layout, depth and plane: the distribution of
|hbd_out >> (depth - 10)  -  process_image(I4xxP10)_out| in ten-bit codes.  No bound is derived: the ten-bit path blends R, G, B of the converted frame with zero padding
at the frame's padded edge and converts back, the hbd path blends Y, Cb, Cr themselves at fp32 with edge clamping, chroma on the box-averaged motion."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    from tools.bench_hbd import planes_from_rgb8
    eng = amd.RIFE(0, rife_v4=True)
    eng.load(gen_models.ensure(None, "rife-v4.6"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("|hbd_out >> (depth - 10) - process_image(ten-bit)_out| in ten-bit codes, timestep 0.5, synthetic rife-v4.6 weights; share of the samples per bin:")
    say("   %-28s %8s %8s %8s %8s %8s %8s | %5s %7s" % ("", "0", "1", "2", "3-4", "5-8", ">8", "max", "mean"))
    for w, h, seed in ((256, 160, 77), (640, 352, 5)):
        a, b = gen_frames.smooth_pair(w, h, seed)
        for name, pixfmt, cls in (("4:2:0", amd.PIX_I420P10, 1), ("4:2:2", amd.PIX_I422P10, 2), ("4:4:4", amd.PIX_I444P10, 3)):
            t0, t1 = planes_from_rgb8(a, 10, cls), planes_from_rgb8(b, 10, cls)
            ref = eng.process_planes(tuple(t0), tuple(t1), 0.5, pixfmt)
            for depth in (12, 16):
                k = depth - 10
                up = lambda ps: tuple(np.ascontiguousarray((p.astype(np.uint32) << k).astype(np.uint16)) for p in ps)
                got = eng.process_hbd(up(t0), up(t1), 0.5, depth, pixfmt)
                for pl, pn in enumerate(("Y", "Cb", "Cr")):
                    d = np.abs((got[pl] >> k).astype(np.int32) - ref[pl].astype(np.int32))
                    n = float(d.size)
                    bins = [(d == 0).sum(), (d == 1).sum(), (d == 2).sum(), ((d >= 3) & (d <= 4)).sum(), ((d >= 5) & (d <= 8)).sum(), (d > 8).sum()]
                    say("   %dx%d %s %2d-bit %-3s      %s | %5d %7.3f" % (w, h, name, depth, pn, " ".join("%8.4f" % (v / n) for v in bins), int(d.max()), float(d.mean())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
