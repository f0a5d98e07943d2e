"""yart_hip_scene_update_lighting on the host: csrc/lighting_update.hpp — MaterialDev records and lobe classes from new descriptors,
the lights' power / power CDF / total power, and an image light's tables (function, row CDFs, row integrals, marginal CDF, guide
tables, interleaved records) from new texels, driven per element and per row in a scrambled order the way the kernels drive them —
against host_scene.hpp::buildHostImage byte for byte (tests/lightingsim/lightingsim.cpp); the properties the cases rely on; and the
argument checks that need no device.

The cases (build_case; frames of 48 x 32 at 4 spp), each a list of states of one scene that differ in material values, light emission /
radius and the texels of image lights' maps only:
  sky_WxH    cornell (open towards the camera) under an image light whose map is W x H — 2x2 (the smallest map a scene can have:
             creation refuses 1x1, test_a_1x1_map_cannot_exist), 8x4, 33x17, 64x64, 65x63, 130x40: non-square, no powers of two,
             w and w + 1 on both sides of a wave and of a 64-column tile — with scenes.sky_octahedral's sun at two directions
  contents   the 65 x 63 map through: two suns, some all-black rows (row integral 0: a uniform CDF), all black (marginal integral 0,
             power 0), negative texels, one texel of 2^64 among values near 1, denormal texels, rows that are zero but for every 16th
             column (runs of equal CDF entries: ties in the guide search)
  materials  scenes.material_test(tex=32): every numeric field changed on several materials — the floor (a bundled texture triple),
             materials with transmission, clearcoat and emission maps —, three that move to another lobe class; then every emission
             at exactly 0
  cornell    cornell's area lights (and their material) dimmed to a quarter and recoloured
  records    scenes.many_records: a third of its 12 light quads at emission 0 (equal consecutive entries of the power CDF)
  uniform    scenes.uniform_sky with a new emission and radius
  two_skies  scenes.two_skies with both infinite lights changed (the image light's radius, the uniform light's emission)
  combined   material_test: materials, lights and the sky's texels in one step"""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import updatesim
from tests.conftest import ROOT
from tests.test_scene_update_host import SIZE, SPP

SKY_SIZES = [(2, 2), (8, 4), (33, 17), (64, 64), (65, 63), (130, 40)]
CASES = [f"sky_{w}x{h}" for w, h in SKY_SIZES] + ["contents", "materials", "cornell", "records", "uniform", "two_skies", "combined"]
SUN_A, SUN_B = (0.35, 0.8, 0.25), (-0.6, 0.3, 0.5)
TWO_64 = np.float32(2.0 ** 64)


def sky_image(w, h, sun_dir, sun_power=20.0):
    """scenes.sky_octahedral's sky and sun, sampled on a w x h grid of the square map"""
    from yart_amd import scenes
    size = max(w, h, 2)
    full = scenes.sky_octahedral(size, sun_dir=sun_dir, sun_power=sun_power).data
    rows, cols = (np.arange(h) * size) // h, (np.arange(w) * size) // w
    return np.ascontiguousarray(full[np.ix_(rows, cols)], np.float32)


def env_scene(img):
    from yart_amd import scenes, yscn
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    t = s.add_texture(yscn.Texture(np.ascontiguousarray(img, np.float32), yscn.TEX_LINEAR))
    s.lights.append(yscn.Light(yscn.LIGHT_IMAGE_INF, texture=t, radius=100.0))
    return s, p


def with_image(s, tex, img):
    s1 = copy.deepcopy(s)
    img = np.ascontiguousarray(img, np.float32)
    assert img.shape == s.textures[tex].data.shape
    s1.textures[tex].data = img
    return s1


def content_images(w=65, h=63):
    rng = np.random.RandomState(5)
    a, b = sky_image(w, h, SUN_A), sky_image(w, h, SUN_B)
    rows = a.copy()
    rows[[0, 1, 2, 20] + list(range(40, h))] = 0.0
    sign = np.where((np.add.outer(np.arange(h), np.arange(w)) % 3 == 0)[..., None], -1.0, 1.0).astype(np.float32)
    big = (0.5 + rng.rand(h, w, 3)).astype(np.float32)
    big[h // 3, w // 2, 1] = TWO_64
    den = (rng.randint(1, 1 << 22, (h, w, 3)).astype(np.uint32)).view(np.float32).copy()
    assert (den > 0).all() and (den < np.finfo(np.float32).tiny).all()
    ties = np.zeros((h, w, 3), np.float32)
    ties[:, ::16] = rng.rand(h, len(range(0, w, 16)), 3).astype(np.float32) + np.float32(0.25)
    ties[5] = 0.0
    ties[5, w - 1] = 1.0                                      # a row whose only texel is its last
    return [a, b, rows, np.zeros_like(a), a * sign, big, den, ties]


def _edit(m, **kw):
    for k, v in kw.items():
        assert hasattr(m, k)
        setattr(m, k, v)


def material_states():
    from yart_amd import scenes
    s0, p = scenes.material_test(SIZE[0], SIZE[1], SPP, 6, tex=32)
    s1 = copy.deepcopy(s0)
    M = s1.materials
    floor, copper, mirror, gold, thin, glass, rough, coat, coat_map, plastic, tiled, leaf, glow, lamp = range(14)
    assert M[floor].tex_base >= 0 and M[floor].tex_mr >= 0 and M[floor].tex_normal >= 0 and M[rough].tex_transmission >= 0
    assert M[coat_map].tex_clearcoat >= 0 and M[glow].tex_emission >= 0 and M[thin].thin_transmission and M[lamp].emission[0] == 20.0
    _edit(M[floor], base=(0.6, 0.9, 0.7), roughness=0.55, metallic=0.25, normal_scale=0.5)
    _edit(M[copper], base=(0.3, 0.5, 0.9), metallic=0.0, roughness=0.6)                    # metallic -> plain: another lobe class
    _edit(M[gold], anisotropic=0.4, aniso_rotation=-1.1, roughness=0.25)
    _edit(M[thin], transmission=0.6, roughness=0.1, ior=1.3)                               # (stays > 0: the transparency bit stays)
    _edit(M[glass], transmission=0.0, base=(0.2, 0.7, 0.3), volume_color=(0.9, 0.4, 0.4), volume_density=2.5)   # glass -> opaque
    _edit(M[rough], transmission=0.5, ior=1.7, roughness=0.05)
    _edit(M[coat], clearcoat=0.35, clearcoat_roughness=0.4)
    _edit(M[coat_map], clearcoat=0.5, clearcoat_roughness=0.05, metallic=0.9)
    _edit(M[plastic], clearcoat=0.7, clearcoat_roughness=0.1, roughness=0.3)               # plain -> clearcoat
    _edit(M[glow], emission=(1.0, 5.0, 8.0), base=(0.2, 0.2, 0.2))
    _edit(M[lamp], emission=(30.0, 12.0, 6.0))
    s2 = copy.deepcopy(s1)
    for m in s2.materials:
        m.emission = (0.0, 0.0, 0.0)                                                        # exactly 0 (and back: the way to s0)
    return [s0, s1, s2], p


def scale_lights(s, pick, factor, tint=(1.0, 1.0, 1.0)):
    """a copy with the area lights `pick` selects — and the materials of their triangles — at emission * factor * tint"""
    s1 = copy.deepcopy(s)
    f32 = lambda e: tuple(float(np.float32(v) * np.float32(factor) * np.float32(t)) for v, t in zip(e, tint))
    mats = set()
    for i, l in enumerate(s1.lights):
        if l.type == 0 and pick(i, l):
            l.emission = f32(l.emission)
            mats.add(int(s1.meshes[l.mesh].faces[l.tri][3]))
    for m in mats:
        s1.materials[m].emission = f32(s1.materials[m].emission)
    return s1


def build_case(name):
    """-> (states, params)"""
    from yart_amd import scenes
    if name.startswith("sky_"):
        w, h = (int(v) for v in name[4:].split("x"))
        s0, p = env_scene(sky_image(w, h, SUN_A))
        tex = len(s0.textures) - 1
        return [s0, with_image(s0, tex, sky_image(w, h, SUN_B))], p
    if name == "contents":
        imgs = content_images()
        s0, p = env_scene(imgs[0])
        tex = len(s0.textures) - 1
        return [s0] + [with_image(s0, tex, im) for im in imgs[1:]], p
    if name == "materials":
        return material_states()
    if name == "cornell":
        s0, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
        assert len(s0.lights) >= 2
        return [s0, scale_lights(s0, lambda i, l: True, 0.25, (1.0, 0.5, 0.2))], p
    if name == "records":
        s0, p = scenes.many_records(SIZE[0], SIZE[1], SPP, 5)
        area = [i for i, l in enumerate(s0.lights) if l.type == 0]
        assert len(area) == 2 + 2 * 12                          # cornell's lamp and 12 quads of two triangles
        quad = {i: (k - 2) // 2 for k, i in enumerate(area) if k >= 2}
        return [s0, scale_lights(s0, lambda i, l: i in quad and quad[i] % 3 == 0, 0.0)], p
    if name == "uniform":
        s0, p = scenes.uniform_sky(SIZE[0], SIZE[1], SPP, 4)
        s1 = copy.deepcopy(s0)
        sky = next(l for l in s1.lights if l.type == 1)
        sky.emission, sky.radius = (1.4, 0.9, 0.3), 40.0
        return [s0, s1], p
    if name == "two_skies":
        s0, p = scenes.two_skies(SIZE[0], SIZE[1], SPP, 5, tex=32)
        s1 = copy.deepcopy(s0)
        for l in s1.lights:
            if l.type == 1:
                l.emission = (0.9, 0.1, 0.6)
            elif l.type == 2:
                l.radius = 55.0
        return [s0, s1], p
    if name == "combined":
        (s0, s1, _), p = material_states()
        s1 = scale_lights(s1, lambda i, l: True, 0.5, (1.0, 0.3, 0.3))
        s1.materials[13].emission = (30.0, 12.0, 6.0)           # (scale_lights scaled the lamp's: keep the state's own value)
        tex = next(l.texture for l in s1.lights if l.type == 2)
        size = s1.textures[tex].data.shape[0]
        s1.textures[tex].data = scenes.sky_octahedral(size, sun_dir=SUN_B, sun_power=35.0).data
        return [s0, s1], p
    raise KeyError(name)


def update_args(prev, new):
    """the arguments of DeviceScene.update_lighting that take a scene holding `prev` to `new`: only what differs is passed"""
    args = {}
    if [m.pack() for m in prev.materials] != [m.pack() for m in new.materials]:
        args["materials"] = new.materials
    if [l.pack() for l in prev.lights] != [l.pack() for l in new.lights]:
        args["lights"] = new.lights
    images = {}
    for t in sorted({l.texture for l in new.lights if l.type == 2}):
        a, b = prev.textures[t].data, new.textures[t].data
        if a.tobytes() != b.tobytes():
            images[t] = b
    if images:
        args["images"] = images
    return args


def steps_of(states):
    return list(zip(states[:-1], states[1:])) + [(states[-1], states[0])]


SIM_SOURCES = ["lightingsim/lightingsim.cpp"]


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    return updatesim.build_sim(str(tmp_path_factory.mktemp("lightingsim") / "lightingsim"), SIM_SOURCES)


TAGS = ("materials", "lobe classes", "texF32", "envs", "envData", "envGuide", "lights", "areaPowerCdf", "totalPower")


def run_sim(exe, tmp_path, s0, s1):
    out = updatesim.run_sim(exe, tmp_path, s0, s1, TAGS)
    envs = [dict(changed=bool(int(m.group(1))), w=int(m.group(2)), h=int(m.group(3)), black=int(m.group(4)), integral=float(m.group(5)))
            for m in re.finditer(r"^env \d+ texture \d+ changed (\d) w (\d+) h (\d+) blackRows (\d+) margIntegral (\S+)$", out, re.M)]
    classes = int(re.search(r"^classes changed (\d+)$", out, re.M).group(1))
    cdf = re.search(r"^power cdf: (\d+) entries, (\d+) equal to their predecessor, total (\S+)$", out, re.M)
    return dict(out=out, envs=envs, classes=classes, cdf_equal=int(cdf.group(2)), total=float(cdf.group(3)))


@pytest.mark.parametrize("name", CASES)
def test_rederived_lighting_equals_a_fresh_scene_on_bytes(sim, tmp_path, name):
    """Every case, every step between its states and the way back: lighting_update.hpp over buildHostImage(old) and the new
    descriptors / texels == buildHostImage(new) on materials, lobe classes, lights, envs, envData, envGuide (the lower-bound search
    against creation's running scan), areaPowerCdf, totalPower and texF32."""
    states, _ = build_case(name)
    for k, (s0, s1) in enumerate(steps_of(states)):
        args = update_args(s0, s1)
        assert args, "the step changes something"
        got = run_sim(sim, str(tmp_path), s0, s1)
        assert ("images" in args) == any(e["changed"] for e in got["envs"])
        if name.startswith("sky_"):
            w, h = (int(v) for v in name[4:].split("x"))
            assert [(e["w"], e["h"], e["changed"]) for e in got["envs"]] == [(w, h, True)]
        if name == "contents":
            e = got["envs"][0]
            target = (k + 1) % len(states)
            assert (e["black"] > 0 and e["integral"] > 0) == (target == 2), "some rows are black, not all"
            assert (e["integral"] == 0 and e["black"] == e["h"]) == (target == 3), "the all-black map: marginal integral 0"
        if name == "materials":
            assert got["classes"] >= 3 if k in (0, 2) else True, "materials move to another lobe class"
        if name == "records" and k == 0:
            assert got["cdf_equal"] >= 8, "dark lights: equal consecutive entries of the power CDF"
        if name in ("cornell", "records", "uniform", "two_skies"):
            assert "lights" in args and "images" not in args
        if name == "combined":
            assert set(args) == {"materials", "lights", "images"}


def test_a_1x1_map_cannot_exist(sim, tmp_path):
    """A 1 x 1 environment map is not a case: scene creation refuses textures below 2 x 2 texels, so no scene can hold one and an
    update cannot resize a map. The smallest case is 2 x 2."""
    s, _ = env_scene(np.ones((1, 1, 3), np.float32))
    a = os.path.join(tmp_path, "one.yscn")
    s.save(a)
    r = subprocess.run([sim, a, a], capture_output=True, text=True)
    assert r.returncode == 3 and "REFUSED by scene creation" in r.stdout and "2x2" in r.stdout, r.stdout + r.stderr


def test_the_cases_hold_what_they_claim(built):
    imgs = content_images()
    assert all(im.shape == (63, 65, 3) and im.dtype == np.float32 and np.isfinite(im).all() for im in imgs)
    assert (imgs[4] < 0).any() and (imgs[4] > 0).any()
    assert (imgs[5] == TWO_64).sum() == 1 and np.abs(imgs[5]).max() == TWO_64
    assert (np.abs(imgs[2]).sum(axis=(1, 2)) == 0).sum() > 3 and (np.abs(imgs[2]).sum(axis=(1, 2)) > 0).any()
    assert not imgs[3].any()
    states, _ = build_case("materials")
    for a, b in zip(states[0].materials, states[1].materials):
        assert (a.tex_base, a.tex_mr, a.tex_normal, a.tex_transmission, a.tex_clearcoat, a.tex_emission, a.thin_transmission) == \
               (b.tex_base, b.tex_mr, b.tex_normal, b.tex_transmission, b.tex_clearcoat, b.tex_emission, b.thin_transmission)
        assert (a.thin_transmission and a.transmission > 0) == (b.thin_transmission and b.transmission > 0)
    assert sum(a.pack() != b.pack() for a, b in zip(states[0].materials, states[1].materials)) >= 10
    assert not any(m.is_emissive for m in states[2].materials) and any(m.is_emissive for m in states[1].materials)


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), on the combined case and on the
    odd-sized map."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "lightingsim_san"), SIM_SOURCES, sanitized=True)
    for name in ("combined", "sky_65x63"):
        states, _ = build_case(name)
        run_sim(exe, str(tmp_path), states[0], states[1])


def test_argument_errors_without_a_device(built):
    """NULL arguments, struct_size, flags, all counts 0, a count with a NULL pointer and a small stats struct are refused with
    YART_E_INVALID before a scene or a device is looked at; the entries are exported and bound."""
    from yart_amd import api
    L = api.lib()
    for name in ("yart_hip_scene_update_lighting", "yart_hip_probe_lighting", "yart_hip_probe_texel_sum"):
        assert name in api.EXPORTS
    assert ctypes.sizeof(api.EnvImageUpdate) == 24 and ctypes.sizeof(api.SceneLightingUpdate) == 56
    size = ctypes.sizeof(api.SceneLightingUpdate)
    mats, lights = (api.MaterialDesc * 1)(), (api.LightDesc * 1)()
    px = np.zeros((2, 2, 3), np.float32)
    imgs = (api.EnvImageUpdate * 1)(api.EnvImageUpdate(0, 2, 2, px.ctypes.data_as(ctypes.c_void_p)))
    up = api.SceneLightingUpdate(size, 1, mats, 0, None, 0, None, 0)
    assert L.yart_hip_scene_update_lighting(None, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    assert L.yart_hip_probe_lighting(None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    fake = ctypes.c_void_p(0x1000)                            # a handle that is never dereferenced: the update itself is checked first
    assert L.yart_hip_scene_update_lighting(fake, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    U = api.SceneLightingUpdate
    for bad, word in ((U(8, 1, mats, 0, None, 0, None, 0), b"struct_size"), (U(0, 1, mats, 0, None, 0, None, 0), b"struct_size"),
                      (U(size, 1, mats, 0, None, 0, None, 1), b"flags"), (U(size, 0, mats, 0, lights, 0, imgs, 0), b"all 0"),
                      (U(size, 1, None, 0, None, 0, None, 0), b"materials pointer"), (U(size, 0, None, 1, None, 0, None, 0), b"lights pointer"),
                      (U(size, 0, None, 0, None, 1, None, 0), b"images pointer")):
        assert L.yart_hip_scene_update_lighting(fake, ctypes.byref(bad), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
    small = api.SceneUpdateStats(4)
    assert L.yart_hip_scene_update_lighting(fake, ctypes.byref(up), None, ctypes.byref(small)) == api.YART_E_INVALID
    assert b"stats" in L.yart_hip_last_error()
    # the host part of an image replacement: three sequential binary32 sums in row-major order
    img = content_images()[0]
    out = np.zeros(3, np.float32)
    assert L.yart_hip_probe_texel_sum(img.ctypes.data_as(ctypes.c_void_p), img.shape[0] * img.shape[1], out.ctypes.data_as(ctypes.c_void_p)) == 0
    want = np.zeros(3, np.float32)
    for texel in img.reshape(-1, 3):
        want += texel
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert L.yart_hip_abi_version() == 3


def test_cpp_mirror_and_struct_sizes(built, tmp_path):
    """YartEnvImageUpdate / YartSceneLightingUpdate / YartLightingProbe have the ctypes mirrors' sizes for a C++ compiler, and
    yart::hip::DeviceScene::updateLighting exists with the documented signature (include/yart_hip.hpp)."""
    from yart_amd import api
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %zu %zu\\n\", sizeof(YartEnvImageUpdate), sizeof(YartSceneLightingUpdate), sizeof(YartLightingProbe));\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartMaterialDesc>&, const std::vector<YartLightDesc>&,"
                " const std::vector<YartEnvImageUpdate>&, void*) = &yart::hip::DeviceScene::updateLighting;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.EnvImageUpdate), ctypes.sizeof(api.SceneLightingUpdate), ctypes.sizeof(api.LightingProbe)]
