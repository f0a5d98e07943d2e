"""Shading suites: cases aimed on purpose at the places where texture fetches, GGX table lookups, the parametric BSDF and the
lights go wrong (the last texel column, a fractional weight of exactly 0, a table index at its cap, the smooth branches, total
internal reflection, a lobe threshold one float either side, a CDF entry hit exactly, the octahedral seams, the boundary between the
infinite and the area lights), with the scene each suite runs in.

`build(name)` returns (scene, params, cases) — deterministic, byte for byte. Operands are constructed in float64 or on dyadic
lattices and stored as float32. Two kinds of case need numbers only the code under test defines — `uc2` one float either side of a
material's lobe thresholds, and `u` exactly on an entry of a light's CDF or of the light sampler's power table: those are placed
by a second pass over what the oracle restatement prints for the scene (`yart_oracle shade` writes the thresholds of every BSDF
case and the tables next to its records), so build() needs oracle/_build/yart_oracle.

The committed fixtures (tests/golden/shading/, written by tests/golden/make_shade_goldens.py) are these scenes and cases plus the
records the compiled reference gives for them (oracle/shaderec.hpp holds the layout) and the oracle restatement's event masks;
tests/test_shade_suites.py compares the oracle, the host build of the device headers and the device probe with them.
"""
import json
import os
import subprocess
import tempfile

import numpy as np

from yart_amd import scenes
from yart_amd.scenes import MeshBuilder
from yart_amd.yscn import (LIGHT_IMAGE_INF, LIGHT_UNIFORM_INF, TEX_LINEAR, TEX_NONCOLOR, TEX_SRGB, Light, Material, Scene, Texture,
                           trs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle", "_build", "yart_oracle")

CASE = np.dtype([("kind", "<u4"), ("index", "<u4"), ("flags", "<u4"), ("pad", "<u4"), ("f", "<f4", 28)])
REC_WORDS = 32
assert CASE.itemsize == 128
LUT, TEX, MAT, BSDF, LIGHT, PICK = range(6)

# the oracle's event bits (oracle/oracle_main.cpp ShadeEvent), in bit order
EVENTS = ["tex_integer_uv", "tex_negative_uv", "tex_frac_one", "tex_last_cell", "tex_weight_zero",
          "lut_on_grid", "lut_index_cap", "lut_negative_cos", "lut_ior_below_1", "lut_ior_eq_1",
          "lobe_clearcoat", "lobe_metallic", "lobe_dielectric", "lobe_glossy", "absorbed", "specular", "shortcut", "uc2_at_threshold",
          "env_u_on_guide", "env_u_on_cdf", "env_zero_pdf", "octa_seam", "area_sample",
          "pick_infinite", "pick_area", "pick_on_cdf", "pick_near_pinf"]
SUITES = ["textures", "luts", "lobes", "lights", "picks"]
# the events each suite is aimed at: at least FLOOR cases of the suite meet each
TARGETS = {"textures": ["tex_integer_uv", "tex_negative_uv", "tex_frac_one", "tex_last_cell", "tex_weight_zero"],
           "luts": ["lut_on_grid", "lut_index_cap", "lut_negative_cos", "lut_ior_below_1", "lut_ior_eq_1"],
           "lobes": ["lobe_clearcoat", "lobe_metallic", "lobe_dielectric", "lobe_glossy", "absorbed", "specular", "shortcut", "uc2_at_threshold"],
           "lights": ["env_u_on_guide", "env_u_on_cdf", "env_zero_pdf", "octa_seam", "area_sample", "pick_infinite", "pick_area", "pick_near_pinf"],
           "picks": ["pick_on_cdf"]}
FLOOR = 64
MAX_CASES = 2299           # 128-byte records: the largest file stays below the largest fixture of tests/golden
MAX_CASES_ALL = 60000
PARAMS = dict(size=(64, 64), spp=4, depth=4, focal=35.0, fnumber=0.0, eye=(0.0, 5.0, 15.0), target=(0.0, 5.0, 0.0),
              up=(0.0, 1.0, 0.0), exposure=0.0, background=(0.0, 0.0, 0.0))

f32 = np.float32
ONE_MINUS = float(np.nextafter(f32(1), f32(0)))          # 1 - 2^-24, the largest sampler value


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def down(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def case(kind, index=0, flags=0, f=()):
    c = np.zeros(1, CASE)
    c["kind"], c["index"], c["flags"] = kind, index, flags
    v = np.asarray(f, np.float64).ravel()
    assert len(v) <= 28 and np.isfinite(v).all()
    c["f"][0, :len(v)] = v.astype(np.float32)
    return c


def finish(parts):
    c = np.concatenate(parts)
    assert 0 < len(c) <= MAX_CASES, len(c)
    assert np.isfinite(c["f"]).all()
    return c


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def run_oracle(scene, params, cases):
    """-> (lobe thresholds per case [n, 3], the scene's tables) from `yart_oracle shade`."""
    with tempfile.TemporaryDirectory() as d:
        scene.save(os.path.join(d, "s.yscn"))
        scenes.write_params(os.path.join(d, "p.txt"), params)
        cases.tofile(os.path.join(d, "c.bin"))
        subprocess.run([ORACLE, "shade", os.path.join(d, "s.yscn"), os.path.join(d, "p.txt"), os.path.join(d, "c.bin"),
                        os.path.join(d, "o.bin")], check=True, capture_output=True)
        probs = np.fromfile(os.path.join(d, "o.bin.probs"), np.float32).reshape(-1, 3)
        tables = json.load(open(os.path.join(d, "o.bin.tables.json")))
    return probs, tables


def bits_to_f32(v):
    return np.asarray(v, np.uint32).view(np.float32)


def floor_quad(s, material):
    b = MeshBuilder()
    b.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), material)
    s.add_node(s.add_mesh(b.build()))


# ---------------------------------------------------------------------------------------------------------- textures
def uv_axis(n):
    """Coordinates along an axis of n texels: the lattice k / (n - 1) (a fractional weight of exactly 0 where the product is
    exact), exact integers, just below an integer (uv - floor(uv) rounds to 1: the only way to the clamp at n - 2), the last cell
    and one float either side of its edge, negative values."""
    a = [0.0, 1.0, -1.0, 2.0, 0.5, -0.25, -1.75, -3.3, 0.3137, 1.62]
    a += [k / (n - 1.0) for k in range(n)] if n <= 9 else [k / (n - 1.0) for k in (0, 1, 2, 31, 32, n - 3, n - 2, n - 1)]
    a += [float(np.nextafter(f32(0), f32(-1))), -1e-9, -3e-10, down(1.0), down(2.0), down(-1.0)]
    edge = (n - 2.0) / (n - 1.0)
    a += [edge, up(edge), down(edge), (n - 1.5) / (n - 1.0), 1.0 + edge, edge - 2.0]
    return a


def tex_cases(index, w, h, kind=TEX):
    ax, ay = uv_axis(w), uv_axis(h)
    out = []
    for i, x in enumerate(ax):
        for shift in (0, 5, 11):
            out.append((x, ay[(i + shift) % len(ay)]))
    for j, y in enumerate(ay):
        out.append((ax[(j + 3) % len(ax)], y))
    return out


def textures():
    """Every channel count as u8 (linear, sRGB, non-colour) and float RGB, sizes 2 x 2, 2 x N, N x 2, odd, 64 x 64; every texture
    is sampled directly by something, so it has footprint records of its own on the device. One material carries base colour,
    normal and metal-rough maps of one size: the device lays those out as one shared 64-byte record per texel (MAT cases). Four
    image lights and no area light: LIGHT and PICK cases of a scene whose light sampler has no power table. The fourth light
    exists only so that its map — the one with a +inf texel — is sampled directly and gets footprint records; it gets no
    LIGHT case, because its sampling tables are built from that texel (inf and NaN entries: no defined search)."""
    rng = np.random.RandomState(21)
    s = Scene()

    def u8(h, w, c, typ):
        return s.add_texture(Texture(rng.randint(0, 256, (h, w, c)).astype(np.uint8), typ))

    def hdr(h, w):
        return s.add_texture(Texture((rng.randint(0, 64, (h, w, 3)) / 8.0).astype(np.float32), TEX_LINEAR))
    t1a, t1b = u8(2, 2, 1, TEX_NONCOLOR), u8(3, 5, 1, TEX_NONCOLOR)
    t2a, t2b = u8(7, 2, 2, TEX_NONCOLOR), u8(64, 64, 2, TEX_NONCOLOR)
    t3a, t3b = u8(5, 3, 3, TEX_SRGB), u8(2, 7, 3, TEX_NONCOLOR)
    t4a, t4b, t4c = u8(64, 64, 4, TEX_SRGB), u8(2, 2, 4, TEX_LINEAR), u8(6, 9, 4, TEX_SRGB)
    f3a, f3b, f3c = hdr(4, 4), hdr(3, 5), hdr(2, 2)
    b8, n8, m8 = u8(8, 8, 4, TEX_SRGB), u8(8, 8, 3, TEX_NONCOLOR), u8(8, 8, 2, TEX_NONCOLOR)
    s.add_material(Material(base=(0.8, 0.7, 0.6), roughness=0.5, transmission=0.5, tex_transmission=t1a))
    s.add_material(Material(roughness=0.5, clearcoat=1.0, clearcoat_roughness=0.4, tex_clearcoat=t1b))
    s.add_material(Material(roughness=1.0, metallic=1.0, tex_mr=t2a))
    s.add_material(Material(roughness=1.0, metallic=1.0, tex_mr=t2b))
    s.add_material(Material(roughness=0.6, emission=(2.0, 3.0, 4.0), tex_emission=t3a))
    s.add_material(Material(roughness=0.6, tex_normal=t3b))
    s.add_material(Material(roughness=0.6, tex_base=t4a))
    s.add_material(Material(roughness=0.6, tex_base=t4b))
    s.add_material(Material(roughness=0.6, tex_base=t4c))
    bundle = s.add_material(Material(base=(0.9, 0.8, 0.7), roughness=1.0, metallic=1.0, tex_base=b8, tex_normal=n8, tex_mr=m8))
    floor_quad(s, 0)
    # a float map whose texel (row 1, column 0) is +inf. A fetch that clamps the column at width - 1 instead of width - 2 gives the
    # same VALUE everywhere else (its extra tap, the next row's first texel, has weight exactly 0); here 0 * inf shows it.
    px = (rng.randint(1, 64, (3, 3, 3)) / 8.0).astype(np.float32)
    px[1, 0, :] = np.inf
    finf = s.add_texture(Texture(px, TEX_LINEAR))
    for t, r in ((f3a, 50.0), (f3b, 80.0), (f3c, 20.0), (finf, 30.0)):
        s.lights.append(Light(LIGHT_IMAGE_INF, texture=t, radius=r))
    parts = []
    for x in (float(np.nextafter(f32(0), f32(-1))), -1e-9, -3e-10):
        for y in (0.0, 0.25, 0.4):                                  # the column past the clamp, in the row above the +inf texel
            parts.append(case(TEX, finf, 0, (x, y)))
    for t in (t1a, t1b, t2a, t2b, t3a, t3b, t4a, t4b, t4c, f3a, f3b, f3c):
        tx = s.textures[t]
        for uv in tex_cases(t, tx.width, tx.height):
            parts.append(case(TEX, t, 0, uv))
    n, t4 = unit((0.2, 0.3, 0.9)), (*unit((0.9, 0.1, -0.2333333)), -1.0)
    for k, uv in enumerate(tex_cases(0, 8, 8)):
        parts.append(case(MAT, bundle, 0, (*uv, *n, *t4, 0.5)))
        if k % 3 == 0:                                              # the shared record through matEvaluate as well
            parts.append(case(BSDF, bundle, k & 1, (*unit((0.3, -0.2, 0.8)), *unit((-0.4, 0.1, 0.7)), 0, 0, 1, 1, 0, 0, *uv, 0.3, 0.6, 0.4, 0.2)))
    for li in range(3):
        for k in range(16):
            wi = unit(rng.randint(-4, 5, 3) + np.array([0.0, 0.0, 0.5]))
            parts.append(case(LIGHT, li, 0, (0, 0, 0, (k * 5 % 16) / 16.0, (k * 3 % 16 + 0.5) / 16.0, *wi)))
    for u in (0.0, ONE_MINUS, 0.25, down(0.25), 0.5, down(0.5), 0.75, down(0.75), 1.0 / 3.0, 0.999):
        parts.append(case(PICK, 0, 0, (u,)))
    return s, dict(PARAMS), finish(parts)


# -------------------------------------------------------------------------------------------------------------- luts
def luts():
    """kat::lutInputs()'s grid, refined: every operand at 0, at 1, exactly on the tables' lattices (k / 31, k / 15) and one float
    either side of the cap's lattice point, negative cosines, ior below, at and above 1."""
    s = Scene()
    floor_quad(s, s.add_material(Material(roughness=1.0)))
    lat = sorted(set([k / 31.0 for k in range(32)] + [k / 15.0 for k in range(16)]))
    edges = [up(30 / 31.0), down(30 / 31.0), up(14 / 15.0), down(14 / 15.0), down(1.0), 0.999, 0.013, up(0.0), 1e-20]
    cs = [-1.0, -0.73, -0.4, -0.01, -1e-30, -0.0] + lat + edges
    rs = lat + edges
    small = [0.0, 0.03, 0.2, 0.5, 14 / 15.0, 30 / 31.0, 1.0, 0.81, down(1.0), 1 / 15.0, 1 / 31.0, 0.97]
    fs = [0.0, 0.04, 0.35, 1.0, 1 / 15.0, 14 / 15.0, up(14 / 15.0), 0.5, down(1.0), 7 / 15.0]
    iors = [1.5, 1.0 / 1.5, 1.33, 2.4, 1.0, 0.5, down(1.0), up(1.0), 1.0, 5.0, 0.9, 1.0001, 30.0, 1.0]
    parts, k = [], 0
    for c in cs:
        for r in small:
            parts.append(case(LUT, 0, 0, (c, r, fs[k % len(fs)], iors[k % len(iors)]))); k += 1
    for r in rs:
        for c in small + [-0.5, -1.0]:
            parts.append(case(LUT, 0, 0, (c, r, fs[k % len(fs)], iors[k % len(iors)]))); k += 1
    for f0 in lat:
        for j in range(4):
            parts.append(case(LUT, 0, 0, (small[(k + j) % len(small)], small[(k + 2 * j + 1) % len(small)], f0, iors[k % len(iors)]))); k += 1
    return s, dict(PARAMS), finish(parts)


# ------------------------------------------------------------------------------------------------------------- lobes
R_SMOOTH = 1e-3 ** 0.5           # roughness^2 = the ggxSmooth threshold


def lobe_materials(s):
    rng = np.random.RandomState(33)

    def u8(h, w, c, typ):
        return s.add_texture(Texture(rng.randint(0, 256, (h, w, c)).astype(np.uint8), typ))
    em, nm, coat = u8(4, 4, 3, TEX_SRGB), u8(4, 6, 3, TEX_NONCOLOR), u8(3, 3, 1, TEX_NONCOLOR)
    M = Material
    mats = [
        M(base=(0.7, 0.6, 0.5), roughness=0.5),                                                    # 0 the all-zero material: the shortcut
        M(base=(0.7, 0.6, 0.5), roughness=0.0),                                                    # 1 ... smooth
        M(base=(0.7, 0.6, 0.5), roughness=1.0, emission=(3.0, 2.0, 1.0)),                          # 2 ... emissive
        M(base=(0.7, 0.6, 0.5), roughness=0.6, emission=(3.0, 2.0, 1.0), tex_emission=em),         # 3 ... emission map
        M(base=(0.9, 0.6, 0.3), roughness=0.4, metallic=1.0),                                      # 4 metal
        M(base=(0.9, 0.6, 0.3), roughness=0.0, metallic=1.0),                                      # 5 metal, smooth
        M(base=(0.9, 0.6, 0.3), roughness=0.5, metallic=1.0, anisotropic=1.0, aniso_rotation=0.7),   # 6 metal, anisotropic
        M(base=(0.8, 0.9, 0.95), roughness=0.3, transmission=1.0, ior=1.5),                        # 7 glass, refractive
        M(base=(0.8, 0.9, 0.95), roughness=0.0, transmission=1.0, ior=1.5),                        # 8 glass, smooth
        M(base=(0.8, 0.9, 0.95), roughness=0.3, transmission=1.0, ior=1.33, thin_transmission=True),   # 9 thin
        M(base=(0.8, 0.9, 0.95), roughness=0.0, transmission=1.0, ior=1.33, thin_transmission=True),   # 10 thin, smooth
        M(base=(0.8, 0.9, 0.95), roughness=0.4, transmission=1.0, ior=0.8, volume_color=(0.9, 0.5, 0.2), volume_density=0.7),   # 11 ior below 1
        M(base=(0.2, 0.3, 0.8), roughness=0.5, clearcoat=1.0, clearcoat_roughness=0.2),            # 12 clearcoat
        M(base=(0.2, 0.3, 0.8), roughness=0.5, clearcoat=1.0, clearcoat_roughness=0.0, ior=1.8),   # 13 clearcoat, smooth (reads m_ior)
        M(base=(0.2, 0.3, 0.8), roughness=0.5, clearcoat=0.5, clearcoat_roughness=0.3, tex_clearcoat=coat),   # 14 clearcoat map
        M(base=(0.6, 0.6, 0.6), roughness=0.45, metallic=0.5, transmission=0.5, clearcoat=0.3, clearcoat_roughness=0.25, anisotropic=0.6,
          aniso_rotation=-1.1),                                                                    # 15 every lobe
        M(base=(0.6, 0.6, 0.6), roughness=down(R_SMOOTH), metallic=0.4, transmission=0.6),         # 16 one float below the smooth threshold
        M(base=(0.6, 0.6, 0.6), roughness=up(R_SMOOTH), metallic=0.4, transmission=0.6),           # 17 ... and above
        M(base=(0.6, 0.6, 0.6), roughness=1.0, metallic=0.3, transmission=0.3, clearcoat=0.2, clearcoat_roughness=1.0),   # 18 roughness 1
        M(base=(0.5, 0.7, 0.5), roughness=0.5, tex_normal=nm),                                     # 19 normal map (c = m = t = 0)
        M(base=(0.5, 0.7, 0.5), roughness=0.2, clearcoat=1e-30),                                   # 20 c tiny but not 0: no shortcut
    ]
    return [s.add_material(m) for m in mats]


def lobes():
    """Materials that isolate each lobe and each mixture (lobe_materials). Directions in the frame n = z, t = x — so that wo.z is
    what the case says: +0 and -0, grazing, back side, wi the mirror of wo, wo + wi = 0 — and in a tilted frame with and without
    a tangent; total internal reflection from inside the refractive materials; `regularized` on and off; uc2 at 0, spread over
    [0, 1) and — second pass — one float either side of pClearcoat, pMetallic and pDielectric."""
    s = Scene()
    mats = lobe_materials(s)
    floor_quad(s, 0)
    z, x = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    nt, tt = unit((0.3, -0.2, 0.9)), unit((0.9, 0.2, -0.2555555))
    wos = [z, (0.0, 0.0, -1.0), unit((0.3, 0.4, 0.866)), unit((0.3, -0.4, -0.866)), unit((1.0, 0.2, 1e-4)), unit((-0.6, 0.8, -1e-4)),
           unit((0.9, 0.0, -0.4358899)), unit((-0.5, 0.5, 0.7071068)), unit((0.1, 0.95, 0.2958)), unit((0.7, -0.7, -0.14))]
    zero_z = [(0.6, 0.8, 0.0), (0.6, 0.8, -0.0)]                   # wo.z at +0 and -0: a few cases per material (they are mostly NaN)
    us = [(0.3, 0.6), (0.0, 0.0), (ONE_MINUS, ONE_MINUS), (0.75, 0.1), (0.5, 0.5), (0.1, 0.9)]
    ucs = [0.01, 0.5, 0.99, 0.0, ONE_MINUS, 0.25]
    uc2s = [0.0, 0.3, 0.7, ONE_MINUS]
    parts, cand = [], []
    k = 0
    for m in mats:
        for i, wo in enumerate(wos + zero_z[k % 2:k % 2 + 1]):
            wo = np.asarray(wo, np.float64)
            wis = [wo * (-1, -1, 1), -wo, unit((-0.2, 0.5, 0.84)), unit((0.4, 0.1, -0.9)), (0.8, -0.6, 0.0)]
            for j in range(3):
                wi = wis[(i + 2 * j + k) % len(wis)]
                plain = (i + j) % 4 != 0
                n, t = (z, x) if plain else ((nt, tt) if i % 2 else (nt, (0.0, 0.0, 0.0)))
                uv = ((k * 7 % 11) / 4.0 - 1.0, (k * 5 % 13) / 5.0 - 0.8)
                for q in range(2):
                    uc2 = uc2s[(2 * j + q + i) % 4]
                    f = (*wo, *wi, *n, *t, *uv, *us[k % len(us)], ucs[(k + q) % len(ucs)], uc2)
                    c = case(BSDF, m, (i + j + q) & 1, f)
                    parts.append(c)
                    if q == 0 and i < 8 and plain:
                        cand.append(c)
                    k += 1
        parts.append(case(MAT, m, 0, (0.3, 0.7, *nt, *tt, 1.0, 0.5 + m)))
        parts.append(case(MAT, m, 0, (-0.3, 1.0, *z, *x, -1.0, 0.0)))
    base = np.concatenate(parts)
    cand = np.concatenate(cand)
    probs, _ = run_oracle(s, PARAMS, cand)
    second = []
    for c, p in zip(cand, probs):
        for col in range(3):
            v = float(p[col])
            if not (0.0 < v < 1.0) or (col > 0 and v == float(p[col - 1])):
                continue
            for u2 in (down(v), v, up(v)):
                d = c.copy().reshape(1)
                d["f"][0, 17] = u2
                second.append(d)
    second = np.concatenate(second)
    room = MAX_CASES - len(base)
    step = max(1, -(-len(second) // room))
    return s, dict(PARAMS), finish([base, second[::step]])


# ------------------------------------------------------------------------------------------------------------ lights
def env_map(h, w, seed):
    """A float RGB map with a row of zero integral, a zero run inside a row, a zero first column from row 2 on (u.x = 0 picks
    a texel of pdf 0 there: the empty sample), a single bright texel and otherwise dyadic noise."""
    rng = np.random.RandomState(seed)
    d = (rng.randint(1, 64, (h, w, 3)) / 16.0).astype(np.float32)
    d[1, :, :] = 0.0
    d[2:, 0, :] = 0.0
    d[3, 2:max(3, w // 2), :] = 0.0
    d[h - 1, w - 1, :] = (40.0, 30.0, 20.0)
    return d


def lights_scene(state=0):
    """Two emissive quads (four area lights: one two-sided, one at emission 0 — two equal consecutive entries of the power table)
    under a rotated, non-uniformly scaled node; a uniform infinite light; two image lights whose maps are 6 x 5 and 12 x 7 (no
    power of two: the guide tables' K = 4 * pow2ge(n) differs from 4 n). state 1: other maps and emissions, the same structure
    (what yart_hip_scene_update_lighting moves the scene to). No emissive triangle of zero area: the loader makes a light of
    every emissive triangle, and such a light's 1 / area is no quantity to pin; the light of power 0 is the one at emission 0."""
    s = Scene()
    e0, e1 = ((10.0, 10.0, 10.0), (2.0, 5.0, 1.0)) if state == 0 else ((4.0, 6.0, 12.0), (7.0, 1.0, 3.0))
    ma = s.add_material(Material(base=(0.8, 0.8, 0.8), roughness=1.0, emission=e0))
    mb = s.add_material(Material(base=(0.8, 0.8, 0.8), roughness=1.0, emission=e1))
    ta = s.add_texture(Texture(env_map(5, 6, 3 + 10 * state), TEX_LINEAR))
    tb = s.add_texture(Texture(env_map(7, 12, 4 + 10 * state), TEX_LINEAR))
    b = MeshBuilder()
    b.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), ma)
    b.quad((2, 1, 0), (3, 1, 0), (3, 2, 0.5), (2, 2, 0.5), mb)
    s.add_node(s.add_mesh(b.build()), 0, *trs(translation=(0.5, 2.0, -1.0), axis=(1, 2, 3), angle=0.9, scale=(2.0, 0.5, 1.25)))
    s.create_area_lights()
    assert len(s.lights) == 4
    s.lights[1].two_sided = True
    s.lights[2].emission = (0.0, 0.0, 0.0)
    s.lights.append(Light(LIGHT_UNIFORM_INF, radius=100.0, emission=(0.6, 0.7, 1.0) if state == 0 else (0.2, 0.9, 0.4)))
    s.lights.append(Light(LIGHT_IMAGE_INF, texture=ta, radius=50.0, fwd=trs(axis=(0, 1, 0), angle=0.6)[0], inv=trs(axis=(0, 1, 0), angle=0.6)[1]))
    s.lights.append(Light(LIGHT_IMAGE_INF, texture=tb, radius=80.0))
    return s


SEAMS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0, 0.8), (0.6, 0, -0.8), (0, -0.6, 0.8), (0, 0.8, -0.6),
         (0.6, 0.8, 0.0), (-0.8, 0.6, -0.0), (1, 0, -0.0), (0.0, -0.0, 1)]


def light_cases(tables, n_lights=7):
    rng = np.random.RandomState(17)
    parts = []
    wis = [unit(v) for v in SEAMS] + [unit(rng.randint(-4, 5, 3) + np.array([0.25, 0.0, 0.0])) for _ in range(10)]
    k = 0

    def add(li, p, u):
        nonlocal k
        parts.append(case(LIGHT, li, 0, (*p, *u, *wis[k % len(wis)])))
        k += 1
    pts = [(0, 0, 0), (1.5, 4.0, -2.0), (-3.0, -1.0, 2.5), (0.5, 2.0, -1.0)]
    tri_u = [(0.0, 0.0), (ONE_MINUS, ONE_MINUS), (0.25, 0.75), (0.75, 0.25), (0.5, 0.5), (0.0, ONE_MINUS), (ONE_MINUS, 0.0), (0.3, up(0.3)), (up(0.3), 0.3)]
    for li in range(4):
        for i, u in enumerate(tri_u + [tuple(rng.randint(0, 64, 2) / 64.0) for _ in range(9)]):
            add(li, pts[i % len(pts)], u)
    for i in range(8):
        add(4, pts[i % 4], (i / 8.0, 0.5))
    for li in ("5", "6"):
        marg = bits_to_f32(tables["envs"][li]["marg"])
        cond = [bits_to_f32(c) for c in tables["envs"][li]["cond"]]
        h, w = len(marg) - 1, len(cond[0]) - 1
        Kh, Kw = 4 * (1 << (h - 1).bit_length()), 4 * (1 << (w - 1).bit_length())
        mid = [float((f32(marg[r]) + f32(marg[r + 1])) * f32(0.5)) for r in range(h)]
        for j in range(Kh + 1):                                     # u.y exactly j / K
            add(int(li), pts[0], ((j * 5 % Kw) / float(Kw) if j % 2 else 0.37, min(j / float(Kh), ONE_MINUS)))
        for j in range(Kw + 1):
            add(int(li), pts[0], (min(j / float(Kw), ONE_MINUS), mid[j % h]))
        for r in range(1, h):                                       # u.y on the marginal CDF's entries and one float either side
            for v in (down(marg[r]), float(marg[r]), up(marg[r])):
                add(int(li), pts[1], (0.61, v))
        for r in range(h):                                          # u.x on the conditional CDF's entries of the row u.y picks
            for c in range(1, w):
                for v in (down(cond[r][c]), float(cond[r][c]), up(cond[r][c])):
                    if 0.0 <= v < 1.0 and marg[r] < mid[r] < marg[r + 1]:
                        add(int(li), pts[2], (v, mid[r]))
        for u in ((0.0, 0.0), (ONE_MINUS, ONE_MINUS), (0.0, ONE_MINUS), (ONE_MINUS, 0.0)):
            add(int(li), pts[3], u)
        # u = 1, which no sampler draws: the reference's search is defined there (the last texel), the guided search only through
        # its clamp of the bracket index to K - 1
        for u in ((1.0, mid[0]), (0.37, 1.0), (1.0, 1.0), (1.0, mid[h - 1])):
            add(int(li), pts[0], u)
        for j in range(40):                                         # u.x = 0 over every row: the rows whose first texel is 0 give no sample
            add(int(li), pts[3], (0.0, (j + 0.5) / 40.0))
    return parts


def pick_cases(tables, boundary=True):
    p_inf = float(bits_to_f32([tables["p_inf"]])[0])
    total = f32(bits_to_f32([tables["total_power"]])[0])
    powers = bits_to_f32(tables["powers"])
    us = [0.0, ONE_MINUS, 0.25, 0.5, down(0.25), up(0.5)]
    us += [j / 128.0 for j in range(128)] + [p_inf + (1.0 - p_inf) * (j + 0.5) / 64.0 for j in range(64)]
    lo = hi = f32(p_inf)
    us.append(p_inf)
    for _ in range(32 if boundary else 0):                          # the boundary between the infinite and the area lights, 32 floats either side
        lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(1))
        us += [float(lo), float(hi)]
    pi, one = f32(p_inf), f32(1.0)
    for c in powers:                                                # u whose scaled value is exactly the table's entry, and its neighbours
        u0 = f32(pi + f32(c) / total * (one - pi))
        near = [u0]
        for _ in range(8):
            near = [np.nextafter(near[0], f32(0))] + near + [np.nextafter(near[-1], f32(1))]
        hit = [u for u in near if f32(f32(f32(u - pi) / f32(one - pi)) * total) == f32(c) and u < one]
        for u in hit[:6]:
            us += [float(u), down(u), up(u)] if u == hit[0] else [float(u)]
        us += [float(u0)]
    # every u of the area range whose scaled value lands on an entry repeats the hit: spread copies over the entries
    return [case(PICK, 0, 0, (min(max(u, 0.0), ONE_MINUS),)) for u in us]


def lights():
    s = lights_scene(0)
    _, tables = run_oracle(s, PARAMS, case(PICK, 0, 0, (0.5,)))
    parts = light_cases(tables) + pick_cases(tables)
    return s, dict(PARAMS), finish(parts)


# ------------------------------------------------------------------------------------------------------------- picks
def picks():
    """160 emissive triangles of different sizes and emissions under a sheared node, a third of them at emission 0 (runs of equal
    entries in the power table), and no infinite light: pInfinite is 0, so u reaches the power table at full float resolution
    and most entries have a u whose scaled value is the entry exactly — those u, and one float either side. More lights than the
    shade kernel's LDS slots hold: the light table stays in memory under every form."""
    s = Scene()
    rng = np.random.RandomState(8)
    b = MeshBuilder()
    n = 160
    for k in range(n):
        e = (0.0, 0.0, 0.0) if k % 3 == 1 else tuple(float(v) for v in rng.randint(1, 40, 3) / 4.0)
        m = s.add_material(Material(base=(0.5, 0.5, 0.5), roughness=1.0, emission=e if any(e) else (1.0, 1.0, 1.0)))
        p0 = np.array([(k % 16) * 1.5, (k // 16) * 1.5, 0.0])
        a, c = rng.randint(1, 9) / 8.0, rng.randint(1, 9) / 8.0
        b.add([p0, p0 + (a, 0, 0), p0 + (0, c, 0.25 * a)], unit((0.0, -0.25, 1.0)), None, None, [[0, 1, 2]], m)
    s.add_node(s.add_mesh(b.build()), 0, *trs(translation=(-3.0, 1.0, 0.5), axis=(3, 1, 2), angle=2.1, scale=(0.75, 1.5, 3.0)))
    s.create_area_lights()
    assert len(s.lights) == n
    for k, l in enumerate(s.lights):
        if k % 3 == 1:
            l.emission = (0.0, 0.0, 0.0)
        l.two_sided = k % 5 == 0
    _, tables = run_oracle(s, PARAMS, case(PICK, 0, 0, (0.5,)))
    parts = pick_cases(tables, boundary=False)
    for k in range(0, n, 2):
        parts.append(case(LIGHT, k, 0, ((k % 7) - 3.0, 2.0, (k % 5) - 2.0, (k * 7 % 32) / 32.0, (k * 11 % 32 + 0.5) / 32.0, *unit((1, k % 3, -1)))))
    return s, dict(PARAMS), finish(parts)


BUILDERS = {"textures": textures, "luts": luts, "lobes": lobes, "lights": lights, "picks": picks}


def build(name):
    return BUILDERS[name]()
