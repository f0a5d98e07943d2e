"""Chooses the defaults of the temporal accumulator's clip (include/yart_hip.h: YART_TEMPORAL_DEFAULT_CLIP_RADIUS / _GAMMA) on the
CPU. No GPU is involved.

  python tools/temporal_clip_sweep.py [--out profiles/temporal_clip_sweep.txt]

For tests/golden/cornell.yscn (96 x 96) and material.yscn (96 x 64): the 6-frame orbit of tools/temporal_sweep.py, rendered by the
host path tracer at 4 spp with its variance and feature buffers (tests/temporalsim `render`), accumulated demodulated at the
default parameters by yart_amd.temporal.temporal_reference with clip=(radius, gamma), and compared with the last camera's frame at
1024 spp (cornell: tests/golden/temporal/cornell_orbit_hi.f32; material: rendered here). Each orbit is used unchanged and with a
change of the lighting: frames 4 and 5 with rgba * 0.25 and variance * 0.0625 — radiance is linear in emission, so that is every
emitter dimmed to a quarter —, compared with 0.25 * the 1024-spp frame. The figure of merit is the RMSE over the AgX-tonemapped
frames (look "none", tests/hostsim `tonemap`) of the last accumulated frame. A candidate's score is the largest, over the four
(scene, sequence) pairs, of that RMSE divided by the better of two alternatives on the pair: accumulating without a clip, and not
accumulating (the last 4-spp frame alone). The defaults are the candidate with the smallest score; among equals the smaller
radius, then the larger gamma.
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
from yart_amd import temporal  # noqa: E402
from tests import test_temporal as tt  # noqa: E402  (orbit_eyes, render_orbit_frame, accumulate_orbit: what the quality tests run)
from tests.paramfile import load_params  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim", "_build", "hostsim")
SCENES = {"cornell": (96, 96), "material": (96, 64)}
RADII, GAMMAS = (1, 2, 3), (0.5, 1.0, 1.5, 2.0, 3.0)
DIM_FROM, DIM_FACTOR = 4, 0.25


def dimmed(frames):
    out = []
    for k, fr in enumerate(frames):
        if k >= DIM_FROM:
            fr = dict(fr, rgba=(fr["rgba"] * np.float32([DIM_FACTOR] * 3 + [1.0])).astype(np.float32),
                      variance=(fr["variance"] * np.float32(DIM_FACTOR * DIM_FACTOR)).astype(np.float32))
        out.append(fr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_clip_sweep.txt"))
    args = ap.parse_args()
    lines = [f"# tools/temporal_clip_sweep.py: host renders, {tt.ORBIT_FRAMES}-frame orbit ({tt.ORBIT_STEP_DEGREES} degrees per frame) at "
             f"{tt.ORBIT_SPP} spp, accumulated (demodulated, default parameters) vs {tt.ORBIT_HI_SPP} spp of the last camera; RMSE over "
             "AgX-tonemapped frames (look none)",
             f"# sequences: `orbit` unchanged; `dimmed`: frames {DIM_FROM} and {DIM_FROM + 1} with rgba * {DIM_FACTOR} and variance * "
             f"{DIM_FACTOR ** 2}, against {DIM_FACTOR} * the {tt.ORBIT_HI_SPP}-spp frame",
             "# ratio = RMSE(last accumulated frame with the clip) / min(RMSE(last accumulated frame without), RMSE(last frame alone))"]
    with tempfile.TemporaryDirectory() as tmp:
        sim = os.path.join(tmp, "temporalsim")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", sim, os.path.join(ROOT, "tests", "temporalsim", "temporalsim.cpp"),
                        os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
        tmap = lambda frame: tt.host_tonemap(HOSTSIM, tmp, frame)
        pairs = {}                                          # (scene, sequence) -> (frames, tonemapped target)
        for name, size in SCENES.items():
            eyes = tt.orbit_eyes(load_params(os.path.join(GOLDEN, name + ".txt")))
            frames = [tt.render_orbit_frame(sim, tmp, name, size, tt.ORBIT_SPP, eye) for eye in eyes]
            fixture = os.path.join(GOLDEN, "temporal", name + "_orbit_hi.f32")
            if os.path.exists(fixture):
                high = np.fromfile(fixture, np.float32).reshape(size[1], size[0], 4)
            else:
                high = tt.render_orbit_frame(sim, tmp, name, size, tt.ORBIT_HI_SPP, eyes[-1])["rgba"]
            pairs[(name, "orbit")] = (frames, tmap(high))
            pairs[(name, "dimmed")] = (dimmed(frames), tmap((high * np.float32([DIM_FACTOR] * 3 + [1.0])).astype(np.float32)))
        base = {}
        for key, (frames, ref) in pairs.items():
            alone = tt.rmse(tmap(frames[-1]["rgba"]), ref)
            unclipped = tt.rmse(tmap(tt.accumulate_orbit(frames)[0]), ref)
            base[key] = min(alone, unclipped)
            lines.append(f"# {key[0]} {key[1]}: RMSE last frame alone {alone:.5f}, accumulated without a clip {unclipped:.5f}")
        lines.append("radius gamma  " + "  ".join(f"{k[0]}_{k[1]:<8}" for k in pairs) + "  score")
        best = None
        for radius, gamma in itertools.product(RADII, GAMMAS):
            ratio = {key: tt.rmse(tmap(tt.accumulate_orbit(frames, clip=(radius, gamma))[0]), ref) / base[key]
                     for key, (frames, ref) in pairs.items()}
            score = max(ratio.values())
            lines.append(f"{radius:<6d} {gamma:<5g}  " + "  ".join(f"{ratio[k]:<{len(k[0]) + 9}.4f}" for k in pairs) + f"  {score:.4f}")
            print(lines[-1], flush=True)
            key = (round(score, 4), radius, -gamma)         # among equal scores: the smaller radius, then the larger gamma
            if best is None or key < best[0]:
                best = (key, radius, gamma, ratio)
        lines.append(f"# smallest score (among scores equal in the four digits above: the smaller radius, then the larger gamma): radius {best[1]} gamma {best[2]:g}: "
                     + ", ".join(f"{k[0]} {k[1]} {v:.4f}" for k, v in best[3].items()))
        lines.append(f"# the defaults in include/yart_hip.h and yart_amd/temporal.py: radius {temporal.DEFAULT_CLIP_RADIUS} gamma "
                     f"{temporal.DEFAULT_CLIP_GAMMA:g}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
