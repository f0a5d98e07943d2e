"""Chooses the defaults of the variance-guided à-trous filter (include/yart_hip.h: YART_DENOISE_VAR_DEFAULT_*) on the CPU and
writes the variance fixtures of tests/test_denoise_var.py's quality test. No GPU is involved.

  python tools/denoise_var_sweep.py [--fixtures] [--out profiles/denoise_var_sweep.txt]

For tests/golden/cornell.yscn (96 x 96) and material.yscn (96 x 64): the host path tracer at 16 spp again — tests/momentsim
`render`, which reduces every sample with csrc/moments.hpp as well — and the assertion that its frame IS the committed
tests/golden/denoise/<scene>_lo.f32, bit for bit: the variance belongs to those very samples. Then
yart_amd.denoise.atrous_var_reference over a grid of sigmas and iteration counts on the committed frames and guides. The
figure of merit is tools/denoise_sweep.py's: the RMSE over the AgX-tonemapped frames (look "none", tests/hostsim `tonemap`)
of the filtered 16-spp frame against the 1024-spp frame, as a ratio to the unfiltered 16-spp frame's. The plain filter's
ratios at its defaults, on the same inputs, are written next to them. --fixtures writes <scene>_var.f32.
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
from yart_amd import denoise  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim", "_build", "hostsim")
SCENES = {"cornell": (96, 96), "material": (96, 64)}
LOW, HIGH = 16, 1024


def tonemapped(frame, tmp):
    h, w = frame.shape[:2]
    src, dst = os.path.join(tmp, "t.in"), os.path.join(tmp, "t.out")
    np.ascontiguousarray(frame, np.float32).tofile(src)
    subprocess.run([HOSTSIM, "tonemap", src, str(w), str(h), "none", dst, os.path.join(tmp, "t.ppm")], check=True)
    return np.fromfile(dst, np.float32).reshape(h, w, 4)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def load_case(name, size):
    w, h = size
    d = os.path.join(GOLDEN, "denoise")
    c = {k: np.fromfile(os.path.join(d, f"{name}_{k}.f32"), np.float32) for k in ("lo", "hi", "albedo", "normal", "depth")}
    return dict(lo=c["lo"].reshape(h, w, 4), hi=c["hi"].reshape(h, w, 4), albedo=c["albedo"].reshape(h, w, 3),
                normal=c["normal"].reshape(h, w, 3), depth=c["depth"].reshape(h, w))


def render_variance(name, size, lo, momentsim, tmp):
    """The variance buffer of the 16-spp host render whose frame is `lo` (asserted on bits)."""
    w, h = size
    base = [ln for ln in open(os.path.join(GOLDEN, name + ".txt")).read().splitlines()
            if ln.split()[0] not in ("size", "spp", "threads", "probe_pixels")]
    pp, fp, mp = (os.path.join(tmp, f"{name}.{e}") for e in ("txt", "f32", "mom"))
    with open(pp, "w") as f:
        f.write("\n".join(base + [f"size {w} {h}", f"spp {LOW}", f"threads {min(16, os.cpu_count() or 1)}"]) + "\n")
    subprocess.run([momentsim, "render", os.path.join(GOLDEN, name + ".yscn"), pp, fp, mp], check=True)
    frame = np.fromfile(fp, np.float32).reshape(h, w, 4)
    assert np.array_equal(frame.view(np.uint32), lo.view(np.uint32)), \
        f"{name}: the frame of this render is not tests/golden/denoise/{name}_lo.f32: the variance would be of other samples"
    mom = np.fromfile(mp, np.uint32).reshape(h, w, 5)
    assert (mom[..., 4] == LOW).all() or name != "cornell"
    return np.ascontiguousarray(mom[..., 3]).view(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixtures", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_var_sweep.txt"))
    args = ap.parse_args()
    lines = [f"# tools/denoise_var_sweep.py: host renders, {LOW} spp filtered vs {HIGH} spp; RMSE over AgX-tonemapped frames (look none)",
             "# ratio = RMSE(filtered low, high) / RMSE(unfiltered low, high); variance-guided filter, all three guides, demodulated"]
    with tempfile.TemporaryDirectory() as tmp:
        momentsim = os.path.join(tmp, "momentsim")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", momentsim,
                        os.path.join(ROOT, "tests", "momentsim", "momentsim.cpp"),
                        os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
        cases = {name: load_case(name, size) for name, size in SCENES.items()}
        for name, size in SCENES.items():
            cases[name]["var"] = render_variance(name, size, cases[name]["lo"], momentsim, tmp)
            if args.fixtures:
                cases[name]["var"].tofile(os.path.join(GOLDEN, "denoise", f"{name}_var.f32"))
        hi = {name: tonemapped(c["hi"], tmp) for name, c in cases.items()}
        noisy = {name: rmse(tonemapped(c["lo"], tmp), hi[name]) for name, c in cases.items()}
        for name, c in cases.items():
            lines.append(f"# {name}: RMSE(unfiltered {LOW} spp, {HIGH} spp) = {noisy[name]:.5f}; variance of the mean luminance: "
                         f"median {np.median(c['var']):.3e}, max {c['var'].max():.3e}")

        def ratios(fn, **kw):
            r = {}
            for name, c in cases.items():
                out = fn(c, **kw)
                r[name] = rmse(tonemapped(out, tmp), hi[name]) / noisy[name]
            return r

        def var_filter(c, **kw):
            return denoise.atrous_var_reference(c["lo"], c["var"], c["albedo"], c["normal"], c["depth"], **kw)

        def plain_filter(c, **kw):
            return denoise.atrous_reference(c["lo"], c["albedo"], c["normal"], c["depth"], **kw)
        plain = ratios(plain_filter)
        lines.append(f"# the plain filter at its defaults (sigma_color {denoise.DEFAULT_SIGMA_COLOR:g} sigma_normal "
                     f"{denoise.DEFAULT_SIGMA_NORMAL:g} sigma_depth {denoise.DEFAULT_SIGMA_DEPTH:g}, {denoise.DEFAULT_ITERATIONS} "
                     "iterations) on the same inputs: " + ", ".join(f"{n} {v:.4f}" for n, v in plain.items()))
        lines.append("iterations sigma_luma sigma_normal sigma_depth  " + "  ".join(f"ratio_{n}" for n in cases) + "  worst")
        best = None
        for it, sl, sn, sd in itertools.product((3, 4, 5), (0.5, 1.0, 2.0, 4.0, 8.0, 16.0), (0.25, 0.5), (0.1, 0.3)):
            r = ratios(var_filter, iterations=it, sigma_luma=sl, sigma_normal=sn, sigma_depth=sd)
            worst = max(r.values())
            lines.append(f"{it:<10d} {sl:<10g} {sn:<12g} {sd:<12g} " + "  ".join(f"{r[n]:<13.4f}" for n in cases) + f"  {worst:.4f}")
            print(lines[-1], flush=True)
            if best is None or worst < best[0]:
                best = (worst, it, sl, sn, sd, r)
        lines.append(f"# smallest worst-case ratio: {best[1]} iterations, sigma_luma {best[2]:g} sigma_normal {best[3]:g} "
                     f"sigma_depth {best[4]:g}: " + ", ".join(f"{n} {v:.4f}" for n, v in best[5].items()))
        r = ratios(var_filter)
        lines.append(f"# the defaults ({denoise.DEFAULT_VAR_ITERATIONS} iterations, sigma_luma {denoise.DEFAULT_VAR_SIGMA_LUMA:g} "
                     f"sigma_normal {denoise.DEFAULT_VAR_SIGMA_NORMAL:g} sigma_depth {denoise.DEFAULT_VAR_SIGMA_DEPTH:g}): "
                     + ", ".join(f"{n} {v:.4f}" for n, v in r.items()))
        no_worse = all(r[n] <= plain[n] for n in cases)
        lines.append("# against the plain filter at its defaults: " + ("no worse on either scene" if no_worse else
                     "WORSE on " + ", ".join(f"{n} ({r[n]:.4f} vs {plain[n]:.4f})" for n in cases if r[n] > plain[n])))
        r = ratios(var_filter, demodulate=False)
        lines.append("# the defaults without demodulation: " + ", ".join(f"{n} {v:.4f}" for n, v in r.items()))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-6:]))


if __name__ == "__main__":
    main()
