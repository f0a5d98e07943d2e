"""yart_hip_scene_update_textures on the host: csrc/texture_update.hpp — the places that hold a texture's footprint records, "an alpha
byte below 255" per RGBA word, the leaf records' alpha bit, the range of the leaf order below a node of the final node array and the
link words' alpha bit, driven per word, per record and per node in a scrambled order the way the kernels drive them — against
host_scene.hpp::buildHostImage byte for byte (tests/texturesim/texturesim.cpp); the properties the cases rely on; and the argument
checks that need no device.

The cases (build_case; frames of 48 x 32 at 4 spp, textures of at most a few hundred texels), each a list of states of one scene that
differ in the texels of 8-bit textures only:
  size_WxHxC   four cards in the cornell room with a transmission (1 channel), metal-rough (2), emission (3) and base-colour (4) map of
               W x H texels, each followed by a 3 x 3 x 1 texture (9 bytes and 3 pad bytes); the C-channel map gets new texels. 2 x 2
               is the smallest texture a scene can hold; 5 x 3 and 3 x 3 give byte counts that are no multiples of 4 (15, 30, 45; 9, 27)
  forms        one scene with a base map sampled alone (records of its own), a base + normal + metal-rough bundle that two materials
               share, a two-member bundle (base + metal-rough) and a base map that one material bundles and another samples directly:
               one member of the shared bundle, then all three in one call, then the other three forms in one call
  reduce_WxH   a card whose RGBA base map has 4, 63, 64, 65, 255, 256 and 258 texels (2x2, 7x9, 8x8, 5x13, 3x85, 16x16, 2x129), behind
               a filler texture that moves its first word off / onto a 16-byte boundary: all alpha 255, then exactly one alpha byte of
               254 at the first texel, the last, and texels 63 / 64 and 255 / 256 where they exist — an all-255 state between them, so
               the flag flips both ways every time —, then all 0
  tri          a one-triangle mesh (its root is a leaf) whose base map turns from opaque to a cut-out, to other cut-out texels (the
               flag stays), and back
  mixed        a mesh of 72 opaque triangles and, in one corner, 8 of the flipped material: some link words gain the bit, some do not
  stacked      scenes.stacked_leaves with leaves of 40 and 64 coincident triangles (saturated span, long-span word), one of their
               four materials flipped
  instances    scenes.alpha_instances: transformed instances of a bush of cut-out cards and of a thin-glass pane (MAT_TRANSPARENT)
  shared       two materials that share the flipped map"""
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

SIZES = [(2, 2, c) for c in (1, 2, 3, 4)] + [(5, 3, c) for c in (1, 2, 3, 4)] + [(3, 3, 1), (3, 3, 3)]
REDUCE_SIZES = [(2, 2), (7, 9), (8, 8), (5, 13), (3, 85), (16, 16), (2, 129)]
FLIP_CASES = ["tri", "mixed", "stacked", "instances", "shared"]
CASES = [f"size_{w}x{h}x{c}" for w, h, c in SIZES] + ["forms"] + [f"reduce_{w}x{h}" for w, h in REDUCE_SIZES] + FLIP_CASES


def texels(w, h, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def rgba(w, h, seed, alpha=255):
    """random colours; alpha: a byte for every texel, or "cut": a checkerboard of 0 and 255"""
    px = texels(w, h, 4, seed)
    if isinstance(alpha, str):
        yy, xx = np.mgrid[0:h, 0:w]
        px[..., 3] = np.where((yy + xx + seed) % 2 == 0, 0, 255).astype(np.uint8)
    else:
        px[..., 3] = alpha
    return px


def with_texels(s, new):
    """a copy of the scene with the textures of `new` ({index: array}) replaced"""
    s1 = copy.deepcopy(s)
    for t, px in new.items():
        assert px.shape == s.textures[t].data.shape and px.dtype == np.uint8
        s1.textures[t].data = np.ascontiguousarray(px)
    return s1


def add_cards(s, materials, z=2.5, y=(3.0, 6.0)):
    """one quad per material in front of the cornell room's back wall, facing the camera"""
    from yart_amd import scenes
    b = scenes.MeshBuilder()
    n = len(materials)
    for i, m in enumerate(materials):
        x0 = -4.2 + 8.4 * i / n
        x1 = x0 + 8.4 / n - 0.2
        b.quad((x0, y[0], z), (x1, y[0], z), (x1, y[1], z), (x0, y[1], z), m, uv_scale=1.0)
    mesh = s.add_mesh(b.build())
    s.add_node(mesh)
    return mesh


def size_scene(w, h):
    from yart_amd import scenes, yscn
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    tex = {}
    for c, typ in ((1, yscn.TEX_NONCOLOR), (2, yscn.TEX_NONCOLOR), (3, yscn.TEX_SRGB), (4, yscn.TEX_SRGB)):
        px = texels(w, h, c, 10 + c) if c < 4 else rgba(w, h, 14)
        tex[c] = s.add_texture(yscn.Texture(px, typ))
        s.add_texture(yscn.Texture(texels(3, 3, 1, 20 + c), yscn.TEX_NONCOLOR))       # the texture behind it: 9 bytes + 3 pad bytes
    M = yscn.Material
    mats = [s.add_material(M(base=(0.9, 0.9, 1.0), transmission=1.0, roughness=0.3, ior=1.33, tex_transmission=tex[1])),
            s.add_material(M(base=(0.8, 0.7, 0.3), roughness=1.0, metallic=1.0, tex_mr=tex[2])),
            s.add_material(M(base=(0.5, 0.5, 0.5), roughness=1.0, emission=(4.0, 3.0, 2.0), tex_emission=tex[3])),
            s.add_material(M(base=(1, 1, 1), roughness=0.8, tex_base=tex[4]))]
    add_cards(s, mats)
    s.create_area_lights()
    return s, p, tex


FORM_SIZE = (6, 5)


def forms_scene():
    """-> (scene, params, dict of the texture indices)"""
    from yart_amd import scenes, yscn
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    w, h = FORM_SIZE
    T = lambda px, typ: s.add_texture(yscn.Texture(px, typ))
    t = dict(alone=T(rgba(w, h, 1), yscn.TEX_SRGB),
             b3_base=T(rgba(w, h, 2), yscn.TEX_SRGB), b3_normal=T(texels(w, h, 3, 3), yscn.TEX_NONCOLOR), b3_mr=T(texels(w, h, 2, 4), yscn.TEX_NONCOLOR),
             b2_base=T(rgba(w, h, 5), yscn.TEX_SRGB), b2_mr=T(texels(w, h, 2, 6), yscn.TEX_NONCOLOR),
             sh_base=T(rgba(w, h, 7), yscn.TEX_SRGB), sh_mr=T(texels(w, h, 2, 8), yscn.TEX_NONCOLOR))
    M = yscn.Material
    mats = [s.add_material(M(base=(1, 1, 1), roughness=0.8, tex_base=t["alone"])),
            s.add_material(M(base=(1, 1, 1), roughness=1.0, tex_base=t["b3_base"], tex_normal=t["b3_normal"], tex_mr=t["b3_mr"])),
            s.add_material(M(base=(0.6, 0.8, 1.0), roughness=0.5, tex_base=t["b3_base"], tex_normal=t["b3_normal"], tex_mr=t["b3_mr"])),
            s.add_material(M(base=(1, 1, 1), roughness=1.0, tex_base=t["b2_base"], tex_mr=t["b2_mr"])),
            s.add_material(M(base=(1, 1, 1), roughness=1.0, tex_base=t["sh_base"], tex_mr=t["sh_mr"])),
            s.add_material(M(base=(1.0, 0.8, 0.6), roughness=0.6, tex_base=t["sh_base"]))]
    add_cards(s, mats)
    s.create_area_lights()
    return s, p, t


def reduce_states(w, h):
    from yart_amd import scenes, yscn
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    k = REDUCE_SIZES.index((w, h)) % 4
    if k:                                                      # 4 k bytes in front: the map's first word at byte 4 k of a 16-byte line
        s.add_texture(yscn.Texture(texels(2, 2 * k, 1, 30), yscn.TEX_NONCOLOR))
    t = s.add_texture(yscn.Texture(rgba(w, h, 40), yscn.TEX_SRGB))
    add_cards(s, [s.add_material(yscn.Material(base=(1, 1, 1), roughness=0.8, tex_base=t))])
    s.create_area_lights()
    n = w * h
    states, seed = [s], 41
    for pos in [0, n - 1] + [q for q in (63, 64, 255, 256) if q < n - 1]:
        alpha = np.full(n, 255, np.uint8)
        alpha[pos] = 254
        states.append(with_texels(s, {t: rgba(w, h, seed, alpha.reshape(h, w))}))
        states.append(with_texels(s, {t: rgba(w, h, seed + 1)}))
        seed += 2
    states.append(with_texels(s, {t: rgba(w, h, seed, 0)}))
    return states, p, t


def flip_states(name):
    """-> (states, params, the flipped texture): [opaque, cut-out, other cut-out texels] (`instances`: [cut-out, opaque, cut-out])"""
    from yart_amd import scenes, yscn
    M = yscn.Material
    size = (8, 8)
    if name == "instances":
        s, p = scenes.alpha_instances(SIZE[0], SIZE[1], SPP, 5, n_instances=9, cards=40)
        t = next(m.tex_base for m in s.materials if m.tex_base >= 0)
        s.textures[t] = yscn.Texture(rgba(16, 16, 49, "cut"), yscn.TEX_SRGB)           # (a few hundred texels)
        assert (s.textures[t].data[..., 3] < 255).any() and any(m.thin_transmission and m.transmission > 0 for m in s.materials)
        return [s, with_texels(s, {t: rgba(16, 16, 50)}), with_texels(s, {t: rgba(16, 16, 51, "cut")})], p, t
    if name == "stacked":
        s, p = scenes.stacked_leaves(SIZE[0], SIZE[1], SPP, 4, stacks=(40, 64))
        t = s.add_texture(yscn.Texture(rgba(*size, 52), yscn.TEX_SRGB))
        s.materials[-4].tex_base = t                           # the first of the stacks' four materials
    else:
        s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
        t = s.add_texture(yscn.Texture(rgba(*size, 52), yscn.TEX_SRGB))
        flipped = s.add_material(M(base=(1, 1, 1), roughness=0.8, tex_base=t))
        if name == "tri":
            b = scenes.MeshBuilder()
            b.add([(-3, 2, 2.5), (3, 2, 2.5), (0, 7, 2.5)], (0, 0, 1), (1, 0, 0, 1), [(0, 0), (1, 0), (0.5, 1)], [[0, 1, 2]], flipped)
            s.add_node(s.add_mesh(b.build()))
        elif name == "mixed":
            plain = s.add_material(M(base=(0.3, 0.5, 0.8), roughness=0.7))
            b = scenes.MeshBuilder()
            b.grid(lambda U, V: (-4 + 8 * U, 2 + 5 * V, 2.0 + 0 * U), 6, 6, plain)
            for i in range(4):                                 # the flipped faces: four small quads in the upper right corner
                x0, y0 = 3.0 + 0.45 * (i % 2), 6.0 + 0.45 * (i // 2)
                b.quad((x0, y0, 2.6), (x0 + 0.4, y0, 2.6), (x0 + 0.4, y0 + 0.4, 2.6), (x0, y0 + 0.4, 2.6), flipped)
            s.add_node(s.add_mesh(b.build()))
        elif name == "shared":
            add_cards(s, [flipped, s.add_material(M(base=(0.9, 0.6, 0.3), roughness=0.2, metallic=1.0, tex_base=t))])
        else:
            raise KeyError(name)
        s.create_area_lights()
    return [s, with_texels(s, {t: rgba(*size, 53, "cut")}), with_texels(s, {t: rgba(*size, 54, "cut")})], p, t


def build_case(name):
    """-> (states, params)"""
    if name.startswith("size_"):
        w, h, c = (int(v) for v in name[5:].split("x"))
        s, p, tex = size_scene(w, h)
        return [s, with_texels(s, {tex[c]: texels(w, h, c, 60 + c) if c < 4 else rgba(w, h, 64)})], p
    if name == "forms":
        s, p, t = forms_scene()
        w, h = FORM_SIZE
        s1 = with_texels(s, {t["b3_base"]: rgba(w, h, 70)})
        s2 = with_texels(s1, {t["b3_base"]: rgba(w, h, 71), t["b3_normal"]: texels(w, h, 3, 72), t["b3_mr"]: texels(w, h, 2, 73)})
        s3 = with_texels(s2, {t["alone"]: rgba(w, h, 74), t["b2_mr"]: texels(w, h, 2, 75), t["sh_base"]: rgba(w, h, 76)})
        return [s, s1, s2, s3], p
    if name.startswith("reduce_"):
        w, h = (int(v) for v in name[7:].split("x"))
        return reduce_states(w, h)[:2]
    if name in FLIP_CASES:
        return flip_states(name)[:2]
    raise KeyError(name)


def update_args(prev, new):
    """the argument of DeviceScene.update_textures that takes a scene holding `prev` to `new`: the 8-bit textures that differ"""
    return {t: b.data for t, (a, b) in enumerate(zip(prev.textures, new.textures))
            if not b.is_float and a.data.tobytes() != b.data.tobytes()}


def steps_of(states):
    return list(zip(states[:-1], states[1:])) + [(states[-1], states[0])]


def has_alpha(s, m):
    t = s.materials[m].tex_base
    return t >= 0 and bool((s.textures[t].data[..., 3] < 255).any())


def flipped_materials(prev, new):
    return [m for m in range(len(new.materials)) if has_alpha(prev, m) != has_alpha(new, m)]


SIM_SOURCES = ["texturesim/texturesim.cpp"]


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    return updatesim.build_sim(str(tmp_path_factory.mktemp("texturesim") / "texturesim"), SIM_SOURCES)


TAGS = ("texU8", "materials", "leaf records", "bvh nodes", "meshes", "textures")


def run_sim(exe, tmp_path, s0, s1):
    out = updatesim.run_sim(exe, tmp_path, s0, s1, TAGS)
    textures = {int(m.group(1)): dict(changed=bool(int(m.group(2))), places=int(m.group(3)))
                for m in re.finditer(r"^texture (\d+) changed (\d) places (\d+)$", out, re.M)}
    meshes = [dict(nodes=int(m.group(1)), with_bit=int(m.group(2)), without_bit=int(m.group(3)), chain=bool(int(m.group(4))), max_span=int(m.group(5)))
              for m in re.finditer(r"^mesh \d+ nodes (\d+) withBit (\d+) withoutBit (\d+) chain (\d) maxSpan (\d+)$", out, re.M)]
    return dict(out=out, textures=textures, meshes=meshes, flipped=int(re.search(r"^flipped (\d+)$", out, re.M).group(1)))


@pytest.mark.parametrize("name", CASES)
def test_rederived_textures_equal_a_fresh_scene_on_bytes(sim, tmp_path, name):
    """Every case, every step between its states and the way back: texture_update.hpp over buildHostImage(old) and the new texels ==
    buildHostImage(new) on texU8 (pad bytes and neighbours included), materials, leaf records, BVH nodes, mesh records and texture
    records; the flags flip where the texels say so, and the chain runs for exactly the meshes with a face of a flipped material."""
    states, _ = build_case(name)
    for s0, s1 in steps_of(states):
        args = update_args(s0, s1)
        assert args, "the step changes something"
        got = run_sim(sim, str(tmp_path), s0, s1)
        assert sorted(t for t, v in got["textures"].items() if v["changed"]) == sorted(args)
        flips = flipped_materials(s0, s1)
        assert got["flipped"] == len(flips)
        for k, mesh in enumerate(s1.meshes):
            assert got["meshes"][k]["chain"] == bool(set(flips) & set(int(m) for m in mesh.faces[:, 3]))


def test_the_cases_hold_what_they_claim(sim, tmp_path):
    """On the host, from the two images: each flip case really flips at least one material on its first step and on the way back, and
    none on the step between its two cut-out states; the size and form cases flip none; every reduce step flips exactly one; the
    mixed mesh has nodes with and without the bit; the stacked leaves hold 40 and 64 triangles; the forms are the forms."""
    for name in FLIP_CASES:
        states, _, t = flip_states(name)
        steps = steps_of(states)
        assert len(steps) == 3
        flips = [run_sim(sim, str(tmp_path), a, b) for a, b in steps]
        counts = [f["flipped"] for f in flips]
        none = 2 if name == "instances" else 1                 # (instances starts from the cut-out: off, on, none)
        assert all((c == 0) == (k == none) for k, c in enumerate(counts)), (name, counts)
        assert max(counts) == (2 if name == "shared" else 1)
        on = flips[1 if name == "instances" else 0]
        if name == "mixed":
            m = on["meshes"][-1]
            assert m["chain"] and m["with_bit"] > 0 and m["without_bit"] > 0, m
            assert not on["meshes"][0]["chain"]
        if name == "tri":
            assert on["meshes"][-1] == dict(nodes=1, with_bit=1, without_bit=0, chain=True, max_span=1)
        if name == "stacked":
            m = on["meshes"][-1]
            assert m["chain"] and m["max_span"] == 64 and m["with_bit"] > 0, m
            assert sorted(len(x.faces) for x in states[0].meshes)[-1] == 2 * (40 + 64)
        if name == "instances":
            assert sum(m["chain"] for m in on["meshes"]) == 1, "the bush, not the pane or the room"
    for name in [c for c in CASES if c.startswith("size_")] + ["forms"]:
        states, _ = build_case(name)
        assert all(not flipped_materials(a, b) for a, b in steps_of(states))
    for w, h in REDUCE_SIZES:
        states, _, t = reduce_states(w, h)
        assert states[0].textures[t].data.shape == (h, w, 4)
        for a, b in steps_of(states):
            assert len(flipped_materials(a, b)) == 1
        ones = [s.textures[t].data[..., 3].reshape(-1) for s in states[1:-1:2]]
        assert all((a == 254).sum() == 1 and (a == 255).sum() == w * h - 1 for a in ones)
        want = sorted({0, w * h - 1} | {q for q in (63, 64, 255, 256) if q < w * h - 1})
        assert sorted(int(np.argmin(a)) for a in ones) == want
        assert not states[-1].textures[t].data[..., 3].any()
    s, _, t = forms_scene()
    got = run_sim(sim, str(tmp_path), s, with_texels(s, {t["alone"]: rgba(*FORM_SIZE, 99)}))
    places = {k: got["textures"][v]["places"] for k, v in t.items()}
    assert places == dict(alone=1, b3_base=1, b3_normal=1, b3_mr=1, b2_base=1, b2_mr=1, sh_base=2, sh_mr=1), places


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), on a flip with a mixed tree, on
    the long leaves, on the forms and on an odd-sized map."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "texturesim_san"), SIM_SOURCES, sanitized=True)
    for name in ("mixed", "stacked", "forms", "size_5x3x3", "reduce_2x129"):
        states, _ = build_case(name)
        run_sim(exe, str(tmp_path), states[0], states[1])
        run_sim(exe, str(tmp_path), states[1], states[0])


def test_argument_errors_without_a_device(built):
    """NULL arguments, struct_size, flags, n_textures 0, a NULL list and a small stats struct are refused with YART_E_INVALID before a
    scene or a device is looked at; the entries are exported and bound."""
    from yart_amd import api
    L = api.lib()
    for name in ("yart_hip_scene_update_textures", "yart_hip_probe_textures"):
        assert name in api.EXPORTS
    assert (ctypes.sizeof(api.TextureUpdate), ctypes.sizeof(api.SceneTextureUpdate), ctypes.sizeof(api.TexturesProbe)) == (32, 24, 40)
    size = ctypes.sizeof(api.SceneTextureUpdate)
    px = np.zeros((2, 2, 4), np.uint8)
    one = (api.TextureUpdate * 1)(api.TextureUpdate(0, 2, 2, 4, px.ctypes.data, 0))
    U = api.SceneTextureUpdate
    up = U(size, 1, one, 0)
    assert L.yart_hip_scene_update_textures(None, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    assert L.yart_hip_probe_textures(None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    fake = ctypes.c_void_p(0x1000)                            # a handle that is never dereferenced: the update itself is checked first
    assert L.yart_hip_scene_update_textures(fake, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    for bad, word in ((U(8, 1, one, 0), b"struct_size"), (U(0, 1, one, 0), b"struct_size"), (U(size, 1, one, 1), b"flags"),
                      (U(size, 0, one, 0), b"n_textures"), (U(size, 1, None, 0), b"textures pointer")):
        assert L.yart_hip_scene_update_textures(fake, ctypes.byref(bad), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
    small = api.SceneUpdateStats(4)
    assert L.yart_hip_scene_update_textures(fake, ctypes.byref(up), None, ctypes.byref(small)) == api.YART_E_INVALID
    assert b"stats" in L.yart_hip_last_error()
    assert L.yart_hip_abi_version() == 3


def test_cpp_mirror_and_struct_sizes(built, tmp_path):
    """YartTextureUpdate / YartSceneTextureUpdate / YartTexturesProbe have the ctypes mirrors' sizes for a C++ compiler, and
    yart::hip::DeviceScene::updateTextures exists with the documented signature (include/yart_hip.hpp)."""
    from yart_amd import api
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %zu %zu %u\\n\", sizeof(YartTextureUpdate), sizeof(YartSceneTextureUpdate), sizeof(YartTexturesProbe),"
                " unsigned(YART_TEXELS_ON_DEVICE));\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartTextureUpdate>&, void*) = &yart::hip::DeviceScene::updateTextures;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.TextureUpdate), ctypes.sizeof(api.SceneTextureUpdate), ctypes.sizeof(api.TexturesProbe),
                                     api.TEXELS_ON_DEVICE]
