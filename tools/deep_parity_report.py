"""Depth-10 frame parity of rife-v4.6 against the oracle's network (tests/deep_ref.py), next to the 8-bit path on the same scene rounded to 8 bits:

    python tools/deep_parity_report.py [out.txt]

per case the largest difference in codes, the share of exact / off-by-one channels and the PSNR; at 1080p and 4K also p8 and the ratio p10 / max(p8, 1e-5)
(tests/test_gpu_deep.py asserts max <= 1 and ratio <= 8)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import deep_ref
    from oracle import pyoracle
    from tools import gen_models
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    d = gen_models.ensure(None, "rife-v4.6")
    g = amd.RIFE(0, rife_v4=True); g.load(d)
    o = pyoracle.OracleRIFE(rife_v4=True); o.set_gpu_crop(1); o.load(d)
    lines = ["case                      max  exact      off-by-one  PSNR dB | depth 8: max  off-by-one  PSNR dB | p10 / max(p8, 1e-5)"]
    cases = [(640, 360, 0.5, 1000), (256, 192, 0.125, 1001), (100, 60, 0.7, 1002), (33, 47, 0.9, 1003), (8, 300, 0.5, 77), (520, 16, 0.5, 77), (1920, 1080, 0.5, 2000), (3840, 2160, 0.5, 3000)]
    for (w, h, t, seed) in cases:
        a, b = deep_ref.deep_pair(w, h, seed)
        u = g.process(a, b, t)
        p = g.process(amd.pack_a2b10g10r10(a), amd.pack_a2b10g10r10(b), t)
        same = bool((amd.unpack_a2b10g10r10(p) == u).all())
        mx, f0, p10, psnr = deep_ref.report(u, deep_ref.expected_frame(o, a, b, t))
        a8, b8 = deep_ref.to_depth8(a), deep_ref.to_depth8(b)
        mx8, _, p8, psnr8 = deep_ref.report(g.process(a8, b8, t), o.process(a8, b8, t), 8)
        lines.append("%4dx%-4d t=%-5g %-6s %3d  %.6f   %.3e   %6.2f  |          %3d  %.3e   %6.2f  | %5.2f" %
                     (w, h, t, "u16=pk" if same else "DIFFER", mx, f0, p10, psnr, mx8, p8, psnr8, p10 / max(p8, 1e-5)))
        print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
