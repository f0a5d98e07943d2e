"""Measures the moments form of the temporal accumulator (include/yart_hip.h: yart_hip_temporal_accumulate_moments_*) against the
plain form on the CPU, and its one new parameter, min_moment_history. No GPU is involved.

  python tools/temporal_moments_sweep.py [--out profiles/temporal_moments_sweep.txt]

The orbits of tools/temporal_sweep.py (tests/golden/cornell.yscn at 96 x 96 and material.yscn at 96 x 64, 6 frames, 1.5 degrees per
frame, host path tracer with variance and feature buffers) at 1 spp — the sample count the moments form is for — and at 4 spp, and
the last camera's frame at 1024 spp (cornell: the fixture tests/golden/temporal/cornell_orbit_hi.f32). Both forms at the defaults
(demodulated), each followed by the variance-guided filter at its defaults: RMSE over the AgX-tonemapped frames against the
1024-spp frame, as ratios. Then the moments form over min_moment_history.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yart_amd import denoise, temporal  # noqa: E402
from tests import test_temporal as tt  # noqa: E402  (orbit_eyes, render_orbit_frame, host_tonemap, rmse: what the quality tests run)
from tests.paramfile import load_params  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim", "_build", "hostsim")
SCENES = {"cornell": (96, 96), "material": (96, 64)}
SPPS = (1, 4)
MIN_MOMENT_HISTORY = (2, 3, 4, 5, 6, 7)                   # 7: longer than the orbit, the spatial estimate everywhere


def accumulate(frames, moments, **kw):
    fn = temporal.temporal_moments_reference if moments else temporal.temporal_reference
    h, w = frames[0]["rgba"].shape[:2]
    hist = temporal.TemporalHistory(w, h)
    for fr in frames:
        r = fn(hist, fr["camera"], fr["rgba"], fr["variance"], fr["position"], fr["normal"], fr["depth"], fr["coverage"], fr["ids"],
               fr["albedo"], demodulate=True, **kw)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_moments_sweep.txt"))
    args = ap.parse_args()
    lines = [f"# tools/temporal_moments_sweep.py: host renders, {tt.ORBIT_FRAMES}-frame orbit ({tt.ORBIT_STEP_DEGREES} degrees per frame), both forms of the "
             f"temporal accumulator at the defaults (demodulated), then the variance-guided filter at its defaults;",
             f"# RMSE over AgX-tonemapped frames (look none) against {tt.ORBIT_HI_SPP} spp of the last camera",
             "# plain / moments: RMSE(form + filter) / RMSE(accumulated frame, unfiltered; over its finite pixels); moments/plain: the second "
             "chain over the first",
             "scene spp  rmse_accumulated  plain   moments  moments/plain"]
    with tempfile.TemporaryDirectory() as tmp:
        sim = os.path.join(tmp, "temporalsim")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", sim, os.path.join(ROOT, "tests", "temporalsim", "temporalsim.cpp"),
                        os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
        tm = lambda x: tt.host_tonemap(HOSTSIM, tmp, x)
        cases, hi = {}, {}
        for name, size in SCENES.items():
            eyes = tt.orbit_eyes(load_params(os.path.join(GOLDEN, name + ".txt")))
            if name == "cornell":
                high = np.fromfile(os.path.join(GOLDEN, "temporal", "cornell_orbit_hi.f32"), np.float32).reshape(size[1], size[0], 4)
            else:
                high = tt.render_orbit_frame(sim, tmp, name, size, tt.ORBIT_HI_SPP, eyes[-1])["rgba"]
            hi[name] = tm(high)
            for spp in SPPS:
                cases[(name, spp)] = [tt.render_orbit_frame(sim, tmp, name, size, spp, eye) for eye in eyes]

        def chain(key, moments, **kw):
            last = cases[key][-1]
            acc, var, _ = accumulate(cases[key], moments, **kw)
            out = denoise.atrous_var_reference(acc, var, last["albedo"], last["normal"], last["depth"])
            t = tm(acc)
            ok = np.isfinite(t).all(-1)                   # a pixel that is not usable passes through; the filter replaces it
            return tt.rmse(t[ok], hi[key[0]][ok]), tt.rmse(tm(out), hi[key[0]])
        plain = {}
        for key in cases:
            unfiltered, plain[key] = chain(key, False)
            _, m = chain(key, True)
            lines.append(f"{key[0]:<9} {key[1]}  {unfiltered:<16.5f}  {plain[key] / unfiltered:<6.4f}  {m / unfiltered:<7.4f}  {m / plain[key]:.4f}")
            print(lines[-1], flush=True)
        lines.append("# the moments form over min_moment_history (moments/plain per scene and sample count; 7 is longer than the orbit: the spatial "
                     "estimate everywhere)")
        lines.append("min_moment_history  " + "  ".join(f"{n}@{s}spp" for n, s in cases))
        for mmh in MIN_MOMENT_HISTORY:
            r = [chain(key, True, min_moment_history=mmh)[1] / plain[key] for key in cases]
            lines.append(f"{mmh:<18d}  " + "  ".join(f"{v:<12.4f}" for v in r))
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
