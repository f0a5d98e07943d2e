"""Chooses the default sigmas of the à-trous filter (include/yart_hip.h: YART_DENOISE_DEFAULT_*) on the CPU and writes the
fixtures of tests/test_denoise.py's quality test. No GPU is involved.

  python tools/denoise_sweep.py [--fixtures] [--out profiles/denoise_sigma_sweep.txt]

For tests/golden/cornell.yscn (96 x 96) and material.yscn (96 x 64): the host path tracer of the tests (tests/hostsim `render`)
at 16 spp and at 1024 spp, the guides of the 16-spp frame from tests/aovsim `hits` reduced by api.reduce_aov_samples, then
yart_amd.denoise.atrous_reference over a grid of sigmas. The figure of merit is the RMSE over the AgX-tonemapped frames (look
"none", tests/hostsim `tonemap`) of the filtered 16-spp frame against the 1024-spp frame, as a ratio to the RMSE of the
unfiltered 16-spp frame. --fixtures writes the four frames and the guides to tests/golden/denoise/.
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
from yart_amd import api, denoise  # noqa: E402
from tests.paramfile import load_params  # noqa: E402

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


def render_case(name, size, tmp):
    """-> dict(lo, hi (H, W, 4), albedo, normal (H, W, 3), depth (H, W))"""
    w, h = size
    scene = os.path.join(GOLDEN, name + ".yscn")
    base = [ln for ln in open(os.path.join(GOLDEN, name + ".txt")).read().splitlines()
            if ln.split()[0] not in ("size", "spp", "threads", "probe_pixels")]
    out = {}
    for tag, spp in (("lo", LOW), ("hi", HIGH)):
        pp, fp = os.path.join(tmp, f"{name}_{tag}.txt"), os.path.join(tmp, f"{name}_{tag}.f32")
        with open(pp, "w") as f:
            f.write("\n".join(base + [f"size {w} {h}", f"spp {spp}", f"threads {min(16, os.cpu_count() or 1)}"]) + "\n")
        subprocess.run([HOSTSIM, "render", scene, pp, fp], check=True)
        out[tag] = np.fromfile(fp, np.float32).reshape(h, w, 4)
    aovsim = os.path.join(tmp, "aovsim")
    if not os.path.exists(aovsim):
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", aovsim, os.path.join(ROOT, "tests", "aovsim", "aovsim.cpp"),
                        os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(LOW), indexing="ij")
    fin, fout = os.path.join(tmp, "hits.in"), os.path.join(tmp, "hits.out")
    np.stack([xs, ys, ss], -1).reshape(-1, 3).astype(np.uint32).tofile(fin)
    subprocess.run([aovsim, "hits", scene, os.path.join(tmp, f"{name}_lo.txt"), fin, fout], check=True)
    words = np.fromfile(fout, np.uint32).reshape(h, w, LOW, 22)
    f, hit = words.view(np.float32), words[..., 6] == 1
    out["albedo"] = api.reduce_aov_samples(f[..., 14:17], hit)
    out["normal"] = api.reduce_aov_samples(f[..., 11:14], hit)
    out["depth"] = api.reduce_aov_samples(f[..., 7:8], hit)[..., 0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixtures", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_sigma_sweep.txt"))
    args = ap.parse_args()
    lines = [f"# tools/denoise_sweep.py: host renders, {LOW} spp filtered vs {HIGH} spp; RMSE over AgX-tonemapped frames (look none)",
             "# ratio = RMSE(filtered low, high) / RMSE(unfiltered low, high); 5 iterations, all three guides, demodulated unless noted"]
    with tempfile.TemporaryDirectory() as tmp:
        cases = {name: render_case(name, size, tmp) for name, size in SCENES.items()}
        hi = {name: tonemapped(c["hi"], tmp) for name, c in cases.items()}
        noisy = {name: rmse(tonemapped(c["lo"], tmp), hi[name]) for name, c in cases.items()}
        for name in cases:
            lines.append(f"# {name}: RMSE(unfiltered {LOW} spp, {HIGH} spp) = {noisy[name]:.5f}")
        if args.fixtures:
            d = os.path.join(GOLDEN, "denoise")
            os.makedirs(d, exist_ok=True)
            for name, c in cases.items():
                for key, a in c.items():
                    np.ascontiguousarray(a, np.float32).tofile(os.path.join(d, f"{name}_{key}.f32"))

        def ratios(**kw):
            r = {}
            for name, c in cases.items():
                out = denoise.atrous_reference(c["lo"], c["albedo"], c["normal"], c["depth"], **kw)
                r[name] = rmse(tonemapped(out, tmp), hi[name]) / noisy[name]
            return r
        lines.append("sigma_color sigma_normal sigma_depth  " + "  ".join(f"ratio_{n}" for n in cases) + "  worst")
        best = None
        for sc, sn, sd in itertools.product((0.25, 0.5, 1.0, 2.0, 4.0), (0.1, 0.25, 0.5), (0.05, 0.1, 0.3)):
            r = ratios(sigma_color=sc, sigma_normal=sn, sigma_depth=sd)
            worst = max(r.values())
            lines.append(f"{sc:<11g} {sn:<12g} {sd:<12g} " + "  ".join(f"{r[n]:<13.4f}" for n in cases) + f"  {worst:.4f}")
            print(lines[-1], flush=True)
            if best is None or worst < best[0]:
                best = (worst, sc, sn, sd, r)
        lines.append(f"# smallest worst-case ratio: sigma_color {best[1]:g} sigma_normal {best[2]:g} sigma_depth {best[3]:g}: "
                     + ", ".join(f"{n} {v:.4f}" for n, v in best[4].items()))
        r = ratios()
        lines.append(f"# the defaults (sigma_color {denoise.DEFAULT_SIGMA_COLOR:g} sigma_normal {denoise.DEFAULT_SIGMA_NORMAL:g} "
                     f"sigma_depth {denoise.DEFAULT_SIGMA_DEPTH:g}, {denoise.DEFAULT_ITERATIONS} iterations): "
                     + ", ".join(f"{n} {v:.4f}" for n, v in r.items()))
        r = ratios(demodulate=False)
        lines.append("# the defaults without demodulation: " + ", ".join(f"{n} {v:.4f}" for n, v in r.items()))
        for it in (3, 4, 6):
            r = ratios(iterations=it)
            lines.append(f"# the defaults with {it} iterations: " + ", ".join(f"{n} {v:.4f}" for n, v in r.items()))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-7:]))


if __name__ == "__main__":
    main()
