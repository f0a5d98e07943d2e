"""Chooses the defaults of the temporal accumulator (include/yart_hip.h: YART_TEMPORAL_DEFAULT_*) on the CPU and writes the
fixture of tests/test_temporal.py's quality test. No GPU is involved.

  python tools/temporal_sweep.py [--fixtures] [--out profiles/temporal_sweep.txt]

For tests/golden/cornell.yscn (96 x 96) and material.yscn (96 x 64): a 6-frame orbit about the vertical axis through the target,
1.5 degrees per frame, rendered by the host path tracer at 4 spp with its variance and feature buffers (tests/temporalsim
`render`), and the last camera's frame at 1024 spp. Then yart_amd.temporal.temporal_reference over a grid of alpha_min,
max_history, normal_cos_min and plane_tolerance, demodulated. The figure of merit is the RMSE over the AgX-tonemapped frames
(look "none", tests/hostsim `tonemap`) of the accumulated last frame against the 1024-spp frame, as a ratio to the RMSE of the
last 4-spp frame alone; the defaults minimise the worse of the two scenes. The same ratio after the variance-guided filter
(accumulated and filtered against filtered alone) is written for the defaults. --fixtures writes
tests/golden/temporal/cornell_orbit_hi.f32.
"""
import argparse
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yart_amd import denoise, temporal  # noqa: E402
from tests import test_temporal as tt  # noqa: E402  (orbit_eyes, render_orbit_frame, accumulate_orbit: what the quality test runs)
from tests.paramfile import load_params  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim", "_build", "hostsim")
SCENES = {"cornell": (96, 96), "material": (96, 64)}
GRID = dict(alpha_min=(0.0, 0.05, 0.1, 0.2, 0.4), max_history=(32, 8, 4, 2), normal_cos_min=(0.9, 0.8, 0.98),
            plane_tolerance=(0.01, 0.002, 0.05))


def tonemapped(frame, tmp):
    return tt.host_tonemap(HOSTSIM, tmp, frame)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixtures", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_sweep.txt"))
    args = ap.parse_args()
    lines = [f"# tools/temporal_sweep.py: host renders, {tt.ORBIT_FRAMES}-frame orbit ({tt.ORBIT_STEP_DEGREES} degrees per frame) at "
             f"{tt.ORBIT_SPP} spp, accumulated (demodulated) vs {tt.ORBIT_HI_SPP} spp of the last camera; RMSE over AgX-tonemapped frames (look none)",
             "# ratio = RMSE(accumulated last frame, high) / RMSE(last frame alone, high)"]
    with tempfile.TemporaryDirectory() as tmp:
        sim = os.path.join(tmp, "temporalsim")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", sim, os.path.join(ROOT, "tests", "temporalsim", "temporalsim.cpp"),
                        os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
        cases, hi, noisy = {}, {}, {}
        for name, size in SCENES.items():
            eyes = tt.orbit_eyes(load_params(os.path.join(GOLDEN, name + ".txt")))
            cases[name] = [tt.render_orbit_frame(sim, tmp, name, size, tt.ORBIT_SPP, eye) for eye in eyes]
            high = tt.render_orbit_frame(sim, tmp, name, size, tt.ORBIT_HI_SPP, eyes[-1])["rgba"]
            if args.fixtures and name == "cornell":
                os.makedirs(os.path.join(GOLDEN, "temporal"), exist_ok=True)
                high.tofile(os.path.join(GOLDEN, "temporal", "cornell_orbit_hi.f32"))
            hi[name] = tonemapped(high, tmp)
            noisy[name] = tt.rmse(tonemapped(cases[name][-1]["rgba"], tmp), hi[name])
            cov = np.mean([f["coverage"] == 1 for f in cases[name]])
            lines.append(f"# {name}: RMSE(last {tt.ORBIT_SPP}-spp frame, {tt.ORBIT_HI_SPP} spp) = {noisy[name]:.5f}; fully covered pixels {cov:.3f}")

        def ratios(**kw):
            r, reuse = {}, {}
            for name, frames in cases.items():
                acc, _, length = tt.accumulate_orbit(frames, **kw)
                r[name] = tt.rmse(tonemapped(acc, tmp), hi[name]) / noisy[name]
                reuse[name] = float((length > 1).mean())
            return r, reuse
        lines.append("alpha_min max_history normal_cos_min plane_tolerance  " + "  ".join(f"ratio_{n}" for n in cases) + "  worst")
        best = None
        keys = list(GRID)
        for combo in itertools.product(*(GRID[k] for k in keys)):
            kw = dict(zip(keys, combo))
            r, _ = ratios(**kw)
            worst = max(r.values())
            lines.append(f"{kw['alpha_min']:<9g} {kw['max_history']:<11d} {kw['normal_cos_min']:<14g} {kw['plane_tolerance']:<16g} "
                         + "  ".join(f"{r[n]:<13.4f}" for n in cases) + f"  {worst:.4f}")
            print(lines[-1], flush=True)
            # among equal worst cases the most cautious setting: the largest alpha_min, then the shortest history — an orbit of
            # a static scene under constant light cannot speak for a longer memory than it has frames
            key = (worst, -kw["alpha_min"], kw["max_history"])
            if best is None or key < best[3]:
                best = (worst, kw, r, key)
        lines.append("# smallest worst-case ratio (among equals: the largest alpha_min, then the smallest max_history): " + " ".join(f"{k} {v:g}" for k, v in best[1].items())
                     + ": " + ", ".join(f"{n} {v:.4f}" for n, v in best[2].items()))
        edge = [k for k, v in best[1].items() if v in (min(GRID[k]), max(GRID[k]))]
        lines.append("# on the edge of the grid in: " + (", ".join(edge) if edge else "nothing")
                     + f" (a history cannot grow past the {tt.ORBIT_FRAMES} frames of the orbit: every max_history >= {tt.ORBIT_FRAMES} is the same run)")
        r, reuse = ratios()
        lines.append(f"# the defaults (alpha_min {temporal.DEFAULT_ALPHA_MIN:g} max_history {temporal.DEFAULT_MAX_HISTORY} normal_cos_min "
                     f"{temporal.DEFAULT_NORMAL_COS_MIN:g} plane_tolerance {temporal.DEFAULT_PLANE_TOLERANCE:g}): "
                     + ", ".join(f"{n} {v:.4f}" for n, v in r.items()) + "; pixels with a history in the last frame: "
                     + ", ".join(f"{n} {v:.3f}" for n, v in reuse.items()))
        both = {}
        for name, frames in cases.items():
            last = frames[-1]
            guides = (last["albedo"], last["normal"], last["depth"])
            acc, acc_var, _ = tt.accumulate_orbit(frames)
            alone = tt.rmse(tonemapped(denoise.atrous_var_reference(last["rgba"], last["variance"], *guides), tmp), hi[name])
            chain = tt.rmse(tonemapped(denoise.atrous_var_reference(acc, acc_var, *guides), tmp), hi[name])
            both[name] = (alone / noisy[name], chain / noisy[name], chain / alone)
        lines.append("# followed by the variance-guided filter at its defaults (ratio to the unfiltered last frame: filtered alone, accumulated "
                     "and filtered; then the second over the first): " + ", ".join(f"{n} {a:.4f} {c:.4f} {q:.4f}" for n, (a, c, q) in both.items()))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-5:]))


if __name__ == "__main__":
    main()
