"""Where the apply kernel's time goes (csrc/apply_motion.h): one launch at a time at 3840x2160 on 3 planes, the profiler's events around each launch, for three motion
fields - all zero (every tap row is a streaming read), smooth (a few pixels, slowly varying) and the engine's own (rife_hip_process_device_motion on the bench frames).

    python tools/probes/apply_flow_probe.py [--pmc]      # --pmc: the engine's motion on float planes only, 8 launches, for a rocprofv3 --pmc counter pass around it
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import torch
    amd = importlib.import_module("rife-ncnn-vulkan_amd")
    from tools import gen_frames, gen_models
    pmc = "--pmc" in sys.argv
    w, h, n = 3840, 2160, 3
    eng = amd.RIFE(0, rife_v4=True)
    eng.load(gen_models.ensure(None, "rife-v4.6"))
    base = gen_frames.tiled_real_pair(w // 640)
    f8 = [np.ascontiguousarray(base[i])[:h, :w] for i in range(2)]
    fr = [torch.from_numpy(f).cuda() for f in f8]
    out = torch.empty_like(fr[0])
    dflow = torch.empty((h, w * 16), dtype=torch.uint8, device="cuda"); dmask = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda")
    mo = amd.motion_desc(dflow.data_ptr(), dmask.data_ptr(), amd.MOTION_F32, w * 16, w * 4)
    eng.process_device_motion(fr[0].data_ptr(), fr[1].data_ptr(), w, h, 0.5, out.data_ptr(), mo)
    torch.cuda.synchronize()
    flow = dflow.cpu().numpy().view(np.float32).reshape(h, w, 4)
    print("the engine's flow on the bench frames: mean |d| %.2f px, max %.1f px; mean |d(x+1) - d(x)| %.3f px, 99th percentile %.2f px" % (
        np.abs(flow).mean(), np.abs(flow).max(), np.abs(np.diff(flow, axis=1)).mean(), np.percentile(np.abs(np.diff(flow, axis=1)), 99)), flush=True)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    smooth = np.stack([3 * np.sin(xs / 97 + ys / 131), 3 * np.cos(xs / 113 - ys / 89), -3 * np.sin(xs / 101 + ys / 127), -3 * np.cos(xs / 109 - ys / 83)], axis=-1).astype(np.float32)
    fields = {"engine": None, "zero": np.zeros((h, w, 4), np.float32), "smooth": smooth}
    ext = eng.padded_size(w, h)
    for name, dt, sample, maxval in (("3 x float", np.float32, amd.SAMPLE_F32, None), ("3 x u8", np.uint8, amd.SAMPLE_U8, 255)):
        if pmc and dt != np.float32:
            continue
        es = np.dtype(dt).itemsize
        src = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(f, -1, 0).astype(dt)).view(np.uint8).reshape(n, h, w * es)).cuda() for f in f8]
        dst = torch.empty_like(src[0])
        desc = lambda t: amd.planes_desc(w, h, sample, [(t[k].data_ptr(), w * es) for k in range(n)], maxval)
        for fname, fld in fields.items():
            if pmc and fname != "engine":
                continue
            if fld is None:
                m = mo
            else:
                tf = torch.from_numpy(fld.view(np.uint8).reshape(h, w * 16)).cuda(); tm = torch.from_numpy(np.full((h, w), 0.5, np.float32).view(np.uint8).reshape(h, w * 4)).cuda()
                m = amd.motion_desc(tf.data_ptr(), tm.data_ptr(), amd.MOTION_F32, w * 16, w * 4)
            for _ in range(2):
                eng.apply_device_motion(desc(src[0]), desc(src[1]), m, desc(dst), extent=ext)
            eng.profile_enable(True)
            for _ in range(8):
                eng.apply_device_motion(desc(src[0]), desc(src[1]), m, desc(dst), extent=ext)
            torch.cuda.synchronize()
            prof = eng.profile_read()
            eng.profile_enable(False)
            ms = prof["apply_motion"]["ms"] / 8
            nbytes = (20.0 + 3 * n * es) * w * h
            print("   %-10s %-7s motion: %.4f ms per launch, %.2f TB/s of the byte model" % (name, fname, ms, nbytes / (ms * 1e-3) / 1e12), flush=True)


if __name__ == "__main__":
    main()
