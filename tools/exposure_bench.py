#!/usr/bin/env python3
"""Times the auto-exposure kernels on the device and writes profiles/auto_exposure.txt.

    python tools/exposure_bench.py [--out profiles/auto_exposure.txt] [--repeats 200]

At 1920 x 1080 and 3840 x 2160, on a rendered frame (the cornell golden, tests/golden/cornell.f32, upscaled by pixel
repetition and modulated by a fixed smooth ramp so that neighbouring pixels differ) and on a constant frame (every lane of every
wave in one bin: the contention worst case of the LDS histogram):

  k_ex_histogram   both forms (0: per-wave counting, 1: eight interleaved replicas): time, and the read bandwidth it amounts to
                   (16 bytes per pixel), next to the 6.29 TB/s a float4 copy reaches on this GPU. The kept form
                   (csrc/postprocess.inc: YART_EXPOSURE_HISTOGRAM) is the one that is faster on the rendered frame.
  k_ex_resolve     time
  k_ex_apply       with both outputs (16 + 19 bytes per pixel), against the kernels of yart_hip_tonemap_agx and
                   yart_hip_encode_rgb8 one after the other (16 + 16 + 16 + 3 bytes per pixel) on the same frame.

Every figure is device time between two events around `repeats` launches (yart_hip_debug_exposure_time), the median of 5 such
windows after one warm-up window; the variants alternate within a round. No GPU: the tool fails.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_TBS = 6.29
WHAT = {"histogram<0> per-wave counting": 0, "histogram<1> eight replicas": 1, "resolve": 2, "apply<ldr, rgb8>": 3, "tonemap_agx + encode_rgb8": 4}
BYTES = {0: 16, 1: 16, 3: 35, 4: 51}


def rendered(w, h):
    g = np.fromfile(os.path.join(ROOT, "tests", "golden", "cornell.f32"), np.float32).reshape(128, 128, 4)
    ys = (np.arange(h) * 128 // h)[:, None]
    xs = (np.arange(w) * 128 // w)[None, :]
    f = g[ys, xs].copy()
    ramp = (1.0 + 0.25 * np.sin(np.arange(w, dtype=np.float32) * 0.37)[None, :] * np.cos(np.arange(h, dtype=np.float32) * 0.23)[:, None]).astype(np.float32)
    f[..., :3] *= ramp[..., None]
    return np.ascontiguousarray(f, np.float32)


def constant(w, h):
    f = np.empty((h, w, 4), np.float32)
    f[...] = (0.5, 0.25, 0.125, 1.0)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_exposure.txt"))
    ap.add_argument("--repeats", type=int, default=200)
    a = ap.parse_args()
    import torch
    from yart_amd import api
    if not torch.cuda.is_available() or api.lib().yart_hip_device_count() <= 0:
        sys.exit("exposure_bench: no GPU")
    torch.cuda.set_device(0)
    L = api.lib()
    lines = ["# tools/exposure_bench.py: device time per launch (events around %d launches; median of 5 windows after a warm-up window)" % a.repeats,
             "# bandwidth: bytes the pass has to move (histogram 16, apply 16 + 19, the pair 16 + 16 + 16 + 3 per pixel) / time; a float4 copy reaches %.2f TB/s" % HBM_COPY_TBS,
             "# %-10s %-9s %-32s %10s %10s %8s" % ("size", "frame", "kernel", "us", "TB/s", "of copy")]
    verdict = []
    for w, h in ((1920, 1080), (3840, 2160)):
        for tag, make in (("rendered", rendered), ("constant", constant)):
            t = torch.from_numpy(make(w, h)).cuda()
            ldr = torch.empty_like(t)
            rgb8 = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
            ex = api.AutoExposure(device=0)
            ex.meter_into(t, 0.0)
            ep = api.make_exposure_params()
            ms = C.c_float()

            def window(what):
                api._check(L.yart_hip_debug_exposure_time(ex.handle, C.c_void_p(t.data_ptr()), w, h, C.byref(ep), what, a.repeats,
                                                          C.c_void_p(ldr.data_ptr()), C.c_void_p(rgb8.data_ptr()), C.byref(ms)), L)
                return ms.value
            times = {name: [] for name in WHAT}
            for rnd in range(6):                         # round 0 is the warm-up; the variants alternate within a round
                for name, what in WHAT.items():
                    v = window(what)
                    if rnd:
                        times[name].append(v)
            med = {name: statistics.median(v) for name, v in times.items()}
            for name, what in WHAT.items():
                us = med[name] * 1e3
                if what in BYTES:
                    tbs = BYTES[what] * w * h / (med[name] * 1e-3) / 1e12
                    lines.append("  %-10s %-9s %-32s %10.2f %10.2f %7.0f%%" % (f"{w}x{h}", tag, name, us, tbs, 100 * tbs / HBM_COPY_TBS))
                else:
                    lines.append("  %-10s %-9s %-32s %10.2f" % (f"{w}x{h}", tag, name, us))
            names = list(WHAT)
            verdict.append("# %dx%d %s: histogram<0> / histogram<1> = %.3f; apply / (tonemap + encode) = %.3f (spread of the windows: %s)" % (
                w, h, tag, med[names[0]] / med[names[1]], med[names[3]] / med[names[4]],
                ", ".join("%s %.1f%%" % (n.split()[0], 100 * (max(times[n]) - min(times[n])) / med[n]) for n in names)))
            ex.close()
    text = "\n".join(lines + verdict) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
