"""yart_hip_scene_update_lighting on the device (include/yart_hip.h; csrc/lighting_update_kernels.inc): a scene that was handed new
material values, new light emission and new texels for its image lights' maps holds, and renders in every pipeline, the bits of a
scene freshly created from the same description.

The cases are tests/test_lighting_update_host.py's (build_case): frames of 48 x 32 at 4 spp. Per case a scene A is created from the
first state and updated to every further one; after each update yart_hip_probe_lighting's arrays of A and of a fresh scene B are
compared on bytes, the feature buffers and the frame on bits under the three pipelines; the frame differs from the previous state's;
the way back to the first state reproduces the first records and the first frame."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_lighting_update_host import CASES, TWO_64, build_case, scale_lights, update_args
from tests.test_scene_update import FLAGS, bits, raw, render_all, same_render

NO_QUADS = 0xffffffff


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def quad_bytes(rec, t):
    """the footprint records of texture t where it has an array of its own (records inside a material's shared 64-byte records
    leave bytes of the array unwritten: those textures are compared through their texels)"""
    td = rec["textures"][t]
    if len(rec["tex_quads"]) == 0 or td["quad_offset"] == NO_QUADS or td["quad_stride"] != 0 or td["width"] == 0:
        return None
    ch = int(td["channels"])
    size = (16 if ch == 1 else 32 if ch == 2 else 64) if td["is_float"] else (4 if ch == 1 else 8 if ch == 2 else 16)
    first = int(td["quad_offset"]) * 16
    return rec["tex_quads"][first:first + int(td["width"]) * int(td["height"]) * size]


def same_lighting(a, b, tag):
    assert a.keys() == b.keys()
    for name in a:
        if name == "tex_quads":
            assert len(a[name]) == len(b[name]), f"{tag}: size of the footprint-record array"
            for t in range(len(a["textures"])):
                qa, qb = quad_bytes(a, t), quad_bytes(b, t)
                assert (qa is None) == (qb is None) and (qa is None or np.array_equal(qa, qb)), f"{tag}: footprint records of texture {t}"
        elif name == "total_power":
            assert np.float32(a[name]).tobytes() == np.float32(b[name]).tobytes(), f"{tag}: total power {a[name]} != {b[name]}"
        else:
            assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), f"{tag}: {name}"


def run_case(api, name):
    states, p = build_case(name)
    A = api.DeviceScene(states[0], device=0)
    first = A.lighting_records()
    r0 = render_all(A, p)
    previous, held = r0, states[0]
    for k, s in enumerate(states[1:], 1):
        tag = f"{name} state {k}"
        args = update_args(held, s)
        A.update_lighting(**args)
        stats = A.last_update
        print(f"{tag}: {sorted(args)} update {stats}")
        assert (stats["launches"] > 0) == ("images" in args), f"{tag}: kernels are launched for a replaced image only: {stats}"
        assert stats["ms_total"] > 0
        B = api.DeviceScene(s, device=0)
        ra = A.lighting_records()
        same_lighting(ra, B.lighting_records(), tag)
        if "images" in args:
            assert any(quad_bytes(ra, t) is not None for t in args["images"]), f"{tag}: the map has footprint records"
        current = None
        for ftag, flags in FLAGS.items():
            fa, fb = render_all(A, p, flags), render_all(B, p, flags)
            same_render(fa, fb, f"{tag} {ftag}")
            current = current or fa
        B.close()
        assert (bits(current["frame"]) != bits(previous["frame"])).any(), f"{tag}: the update does not change the frame"
        previous, held = current, s
    A.update_lighting(**update_args(held, states[0]))         # the way back
    same_lighting(A.lighting_records(), first, f"{name} round trip")
    same_render(render_all(A, p), r0, f"{name} round trip")
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_updated_lighting_equals_a_fresh_scene(gpu_api, name):
    run_case(gpu_api, name)


@pytest.mark.gpu
def test_the_three_update_entries_combine_in_any_order(gpu_api):
    """update(nodes, lights) — tests/test_scene_update_host.py's `light` case —, update_meshes — tests/test_mesh_update_host.py's `light`
    case: the emissive mesh scaled by 1.5 — and update_lighting on one scene, in two orders, against a scene created from the
    final description."""
    from tests.test_scene_update_host import build_case as moved_case
    api = gpu_api
    s0, s1, p, _, _ = moved_case("light")                     # s1: the light's node and the lights' records moved
    mesh = s0.lights[0].mesh
    final = scale_lights(s1, lambda i, l: True, 0.25, (1.0, 0.5, 0.2))
    final.materials[0].base = (0.3, 0.6, 0.9)
    final.materials[1].roughness = 0.35
    final.meshes[mesh].positions = np.ascontiguousarray(s0.meshes[mesh].positions.astype(np.float32) * np.float32(1.5))
    arrays = {mesh: (final.meshes[mesh].positions, final.meshes[mesh].normals, final.meshes[mesh].tangents)}
    dimmed_in_place = copy.deepcopy(final.lights)             # the final emission at the first state's transforms
    for l, l0 in zip(dimmed_in_place, s0.lights):
        l.fwd, l.inv = l0.fwd, l0.inv
    B = api.DeviceScene(final, device=0)
    want, want_mesh, want_graph = B.lighting_records(), B.mesh_records(mesh), B.scene_graph()
    frames = {tag: render_all(B, p, flags) for tag, flags in FLAGS.items()}
    B.close()

    def transforms_first(A):
        A.update(final.nodes, s1.lights)
        A.update_meshes(arrays)
        A.update_lighting(materials=final.materials, lights=final.lights)

    def lighting_first(A):
        A.update_lighting(materials=final.materials, lights=dimmed_in_place)
        A.update_meshes(arrays)
        A.update(final.nodes, final.lights)

    for order in (transforms_first, lighting_first):
        A = api.DeviceScene(s0, device=0)
        order(A)
        tag = order.__name__
        same_lighting(A.lighting_records(), want, tag)
        got_mesh = A.mesh_records(mesh)
        for key in ("nodes", "leaves", "shade", "positions", "normals", "tangents"):
            assert got_mesh[key].tobytes() == want_mesh[key].tobytes(), f"{tag}: {key}"
        for a, b in zip(A.scene_graph()[:2], want_graph[:2]):
            assert np.array_equal(raw(a), raw(b)), f"{tag}: scene graph"
        for ftag, flags in FLAGS.items():
            same_render(render_all(A, p, flags), frames[ftag], f"{tag} {ftag}")
        A.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(gpu_api):
    """Every YART_E_INVALID condition of the entry once; after each the probe's arrays and the frame are what they were."""
    from yart_amd import yscn
    api = gpu_api
    L = api.lib()
    states, p = build_case("combined")
    s = copy.deepcopy(states[0])
    spare = s.add_texture(yscn.Texture(np.full((4, 4, 3), 0.5, np.float32), yscn.TEX_LINEAR))      # float RGB that no light uses
    sky = next(l.texture for l in s.lights if l.type == 2)
    sky_light = next(i for i, l in enumerate(s.lights) if l.type == 2)
    area = next(i for i, l in enumerate(s.lights) if l.type == 0)
    thin = next(i for i, m in enumerate(s.materials) if m.thin_transmission and m.transmission > 0)
    H, W = s.textures[sky].data.shape[:2]
    good = np.ascontiguousarray(states[1].textures[sky].data, np.float32)
    A = api.DeviceScene(s, device=0)
    before, frame = A.lighting_records(), render_all(A, p)

    def mats(edit=None):
        m = copy.deepcopy(states[1].materials)
        if edit:
            edit(m)
        a = (api.MaterialDesc * len(m))()
        for i, x in enumerate(m):
            ctypes.memmove(ctypes.byref(a[i]), x.pack(), ctypes.sizeof(api.MaterialDesc))
        return a

    def lights(edit=None):
        ls = copy.deepcopy(states[1].lights)
        if edit:
            edit(ls)
        a = (api.LightDesc * len(ls))()
        for i, l in enumerate(ls):
            a[i] = api.LightDesc(l.type, l.mesh, l.tri, int(l.two_sided), l.texture, l.radius, api._f(l.emission, 3), api._f(l.fwd, 16), api._f(l.inv, 16))
        return a

    keep = []

    def images(*items):
        a = (api.EnvImageUpdate * max(len(items), 1))()
        for k, (tex, w, h, px) in enumerate(items):
            if px is not None:
                px = np.ascontiguousarray(px, np.float32)
                keep.append(px)
            a[k] = api.EnvImageUpdate(tex, w, h, px.ctypes.data_as(ctypes.c_void_p) if px is not None else None)
        return a

    def texel(value):
        px = good.copy()
        px[H // 2, W // 3, 2] = value
        return px

    def setf(field, value, index):
        return lambda seq: setattr(seq[index], field, value)

    def nan_matrix(ls):
        ls[area].fwd = np.array(ls[area].fwd, np.float32).copy()
        ls[area].fwd.reshape(-1)[7] = np.nan

    nm, nl, size = len(s.materials), len(s.lights), ctypes.sizeof(api.SceneLightingUpdate)
    U = api.SceneLightingUpdate
    M, Ls, I = mats(), lights(), images((sky, W, H, good))
    cases = [
        ("scene NULL", None, U(size, nm, M, nl, Ls, 1, I, 0), None),
        ("update NULL", A.handle, None, None),
        ("struct_size", A.handle, U(size - 8, nm, M, nl, Ls, 1, I, 0), None),
        ("flags", A.handle, U(size, nm, M, nl, Ls, 1, I, 2), None),
        ("all counts 0", A.handle, U(size, 0, M, 0, Ls, 0, I, 0), None),
        ("n_materials", A.handle, U(size, nm - 1, M, 0, None, 0, None, 0), None),
        ("n_lights", A.handle, U(size, 0, None, nl - 1, Ls, 0, None, 0), None),
        ("materials NULL", A.handle, U(size, nm, None, 0, None, 0, None, 0), None),
        ("tex_base", A.handle, U(size, nm, mats(setf("tex_base", 0, 1)), 0, None, 0, None, 0), None),
        ("tex_emission", A.handle, U(size, nm, mats(setf("tex_emission", -1, 12)), 0, None, 0, None, 0), None),
        ("thin_transmission", A.handle, U(size, nm, mats(setf("thin_transmission", True, 1)), 0, None, 0, None, 0), None),
        ("transparent to opaque", A.handle, U(size, nm, mats(setf("transmission", 0.0, thin)), 0, None, 0, None, 0), None),
        ("material NaN", A.handle, U(size, nm, mats(setf("roughness", float("nan"), 3)), 0, None, 0, None, 0), None),
        ("material inf", A.handle, U(size, nm, mats(setf("volume_color", (1.0, float("inf"), 1.0), 5)), 0, None, 0, None, 0), None),
        ("light type", A.handle, U(size, 0, None, nl, lights(setf("type", 1, area)), 0, None, 0), None),
        ("light mesh", A.handle, U(size, 0, None, nl, lights(setf("mesh", 1, area)), 0, None, 0), None),
        ("light tri", A.handle, U(size, 0, None, nl, lights(setf("tri", 1 + s.lights[area].tri, area)), 0, None, 0), None),
        ("light two_sided", A.handle, U(size, 0, None, nl, lights(setf("two_sided", not s.lights[area].two_sided, area)), 0, None, 0), None),
        ("light texture", A.handle, U(size, 0, None, nl, lights(setf("texture", spare, sky_light)), 0, None, 0), None),
        ("light emission inf", A.handle, U(size, 0, None, nl, lights(setf("emission", (1.0, 1.0, float("inf")), area)), 0, None, 0), None),
        ("light radius NaN", A.handle, U(size, 0, None, nl, lights(setf("radius", float("nan"), sky_light)), 0, None, 0), None),
        ("light matrix NaN", A.handle, U(size, 0, None, nl, lights(nan_matrix), 0, None, 0), None),
        ("texture out of range", A.handle, U(size, 0, None, 0, None, 1, images((10000, W, H, good)), 0), None),
        ("texture twice", A.handle, U(size, 0, None, 0, None, 2, images((sky, W, H, good), (sky, W, H, good)), 0), None),
        ("texture not float", A.handle, U(size, 0, None, 0, None, 1, images((0, 32, 32, good)), 0), None),
        ("texture unused", A.handle, U(size, 0, None, 0, None, 1, images((spare, 4, 4, np.ones((4, 4, 3), np.float32))), 0), None),
        ("width", A.handle, U(size, 0, None, 0, None, 1, images((sky, W - 1, H, good)), 0), None),
        ("height", A.handle, U(size, 0, None, 0, None, 1, images((sky, W, H + 1, good)), 0), None),
        ("pixels NULL", A.handle, U(size, 0, None, 0, None, 1, images((sky, W, H, None)), 0), None),
        ("texel NaN", A.handle, U(size, nm, M, nl, Ls, 1, images((sky, W, H, texel(np.nan))), 0), None),
        ("texel inf", A.handle, U(size, nm, M, nl, Ls, 1, images((sky, W, H, texel(-np.inf))), 0), None),
        ("texel above 2^64", A.handle, U(size, nm, M, nl, Ls, 1, images((sky, W, H, texel(-np.nextafter(TWO_64, np.float32(np.inf))))), 0), None),
        ("stats struct_size", A.handle, U(size, nm, M, nl, Ls, 1, I, 0), api.SceneUpdateStats(4)),
    ]
    for what, handle, up, stats in cases:
        rc = L.yart_hip_scene_update_lighting(handle, ctypes.byref(up) if up is not None else None, None, ctypes.byref(stats) if stats is not None else None)
        print(f"{what}: {rc} {L.yart_hip_last_error().decode()}")
        assert rc == api.YART_E_INVALID, what
        same_lighting(A.lighting_records(), before, what)
        same_render(render_all(A, p), frame, what)
    # ... and the same arguments without a fault are taken: 2^64 itself is a texel the update accepts
    st = api.SceneUpdateStats(ctypes.sizeof(api.SceneUpdateStats))
    ok = U(size, nm, M, nl, Ls, 1, images((sky, W, H, texel(TWO_64))), 0)
    assert L.yart_hip_scene_update_lighting(A.handle, ctypes.byref(ok), None, ctypes.byref(st)) == 0, L.yart_hip_last_error()
    assert st.launches > 0
    after = A.lighting_records()
    assert after["tex_f32"].tobytes() != before["tex_f32"].tobytes() and after["materials"].tobytes() != before["materials"].tobytes()
    A.close()


@pytest.mark.gpu
def test_cpp_mirror_updates_a_scene(gpu_api, tmp_path):
    """yart::hip::DeviceScene::updateLighting (include/yart_hip.hpp) from a C++ program: the cornell container, its light dimmed."""
    states, _ = build_case("cornell")
    path = os.path.join(tmp_path, "cornell.yscn")
    states[0].save(path)
    lights = states[1].lights
    rows = ",\n".join("{%du, %d, %du, %du, %d, %.9ef, {%s}, {%s}, {%s}}" % (
        l.type, l.mesh, l.tri, int(l.two_sided), l.texture, l.radius, ", ".join("%.9ef" % v for v in l.emission),
        ", ".join("%.9ef" % v for v in np.asarray(l.fwd, np.float32).reshape(-1)), ", ".join("%.9ef" % v for v in np.asarray(l.inv, np.float32).reshape(-1)))
        for l in lights)
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main(int, char** argv) {\n"
                "  try {\n"
                "    yart::hip::DeviceScene scene(argv[1], 0);\n"
                "    std::vector<YartLightDesc> lights = {\n" + rows + "};\n"
                "    const YartSceneUpdateStats st = scene.updateLighting({}, lights, {});\n"
                "    YartLightingProbe pr{};\n    pr.struct_size = sizeof(pr);\n"
                "    if (yart_hip_probe_lighting(scene.handle(), &pr)) return 3;\n"
                "    std::printf(\"%u %.9g\\n\", st.launches, double(pr.total_power));\n"
                "  } catch (const std::exception& e) { std::printf(\"error: %s\\n\", e.what()); return 2; }\n"
                "  return 0; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    launches, power = r.stdout.split()
    B = gpu_api.DeviceScene(states[1], device=0)
    want = B.lighting_records()["total_power"]
    B.close()
    assert int(launches) == 0 and np.float32(float(power)) == np.float32(want) and want > 0
