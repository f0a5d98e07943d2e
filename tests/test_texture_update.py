"""yart_hip_scene_update_textures on the device (include/yart_hip.h; csrc/texture_update_kernels.inc): a scene whose 8-bit material
textures were handed new texels holds, and renders in every pipeline, the bits of a scene freshly created from the same description.

The cases are tests/test_texture_update_host.py's (frames of 48 x 32 at 4 spp, textures of a few hundred texels at most). Per case a
scene A is created from the first state and updated to every further one; after each update A and a fresh scene B are compared on
bytes — yart_hip_probe_textures' arrays (every texel byte of the scene: the neighbours and pad bytes of an updated texture with them),
yart_hip_probe_lighting's (materials; footprint records: a texture's own array, and per bundle member its own 16 bytes of every
64-byte record), yart_hip_probe_mesh's of every mesh (leaf records, link words, the alpha flag) — and on bits: the feature buffers and
the frame under the three pipelines. The frame differs from the previous state's; the way back to the first state reproduces the
first records and the first frame. YartSceneUpdateStats.launches says what ran: footprint records once per place, one reduction per
base-colour map, and the chain only where a material's flag changed."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_lighting_update import NO_QUADS, same_lighting
from tests.test_scene_update import FLAGS, bits, raw, render_all, same_render
from tests.test_texture_update_host import (FLIP_CASES, FORM_SIZE, REDUCE_SIZES, SIZES, build_case, flip_states, flipped_materials, forms_scene,
                                            has_alpha, reduce_states, rgba, size_scene, texels, update_args, with_texels)

MAT_HAS_ALPHA, MAT_TRANSPARENT, LINK_ALPHA = 2, 8, 1 << 26


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def record_size(td):
    ch = int(td["channels"])
    return 4 if ch == 1 else 8 if ch == 2 else 16


def member_bytes(rec, i):
    """the footprint records of texture entry i (one of the scene's textures, or a bundle clone): its own bytes per texel position —
    for a bundle member its 16 (8 for two channels) bytes at stride 64. None: the entry has no records (or the scene has none)."""
    td = rec["textures"][i]
    if len(rec["tex_quads"]) == 0 or td["quad_offset"] == NO_QUADS or td["width"] == 0 or td["is_float"]:
        return None
    size, n = record_size(td), int(td["width"]) * int(td["height"])
    stride = int(td["quad_stride"]) or size
    first = int(td["quad_offset"]) * 16
    q = rec["tex_quads"]
    return np.stack([q[first + k * stride:first + k * stride + size] for k in range(n)])


def places(rec, t):
    """texture_update.hpp::tuPlaces in Python: the entries through which texture t's footprint records are rewritten"""
    tex = rec["textures"]
    if len(rec["tex_quads"]) == 0:
        return []
    out = [t] if tex[t]["quad_offset"] != NO_QUADS else []
    seen = set()
    for i in range(len(tex)):
        if tex[i]["quad_stride"] and not tex[i]["is_float"] and tex[i]["offset"] == tex[t]["offset"] and int(tex[i]["quad_offset"]) not in seen:
            seen.add(int(tex[i]["quad_offset"]))
            out.append(i)
    return out


def records(scene, n_meshes):
    return dict(textures=scene.texture_records(), lighting=scene.lighting_records(), meshes=[scene.mesh_records(m) for m in range(n_meshes)])


def same_records(a, b, tag):
    for name in ("tex_u8", "textures"):
        assert a["textures"][name].tobytes() == b["textures"][name].tobytes(), f"{tag}: {name}"
    same_lighting(a["lighting"], b["lighting"], tag)
    la, lb = a["lighting"], b["lighting"]
    for i in range(len(la["textures"])):                      # every entry's own bytes, bundle members at stride 64
        qa, qb = member_bytes(la, i), member_bytes(lb, i)
        assert (qa is None) == (qb is None) and (qa is None or np.array_equal(qa, qb)), f"{tag}: footprint records of texture entry {i}"
    for m, (ma, mb) in enumerate(zip(a["meshes"], b["meshes"])):
        for key in ("nodes", "leaves", "shade", "positions", "normals", "tangents"):
            assert ma[key].tobytes() == mb[key].tobytes(), f"{tag}: mesh {m} {key}"
        assert ma["mesh"].tobytes() == mb["mesh"].tobytes() and ma["stack_bound"] == mb["stack_bound"], f"{tag}: mesh {m} record"


def expected_launches(rec, prev, new, args):
    """what steps 1 to 3 launch: k_tex_quads once per place, one reduction per listed base-colour map"""
    bases = {m.tex_base for m in new.materials if m.tex_base >= 0}
    return sum(len(places(rec, t)) + (1 if t in bases else 0) for t in args)


def run_case(api, name, states, p, render=True):
    n_meshes = len(states[0].meshes)
    A = api.DeviceScene(states[0], device=0)
    first = records(A, n_meshes)
    r0 = render_all(A, p) if render else None
    previous, held = r0, states[0]
    for k, s in enumerate(states[1:] + [states[0]], 1):
        back = k == len(states)
        tag = f"{name} state {k}" if not back else f"{name} round trip"
        args = update_args(held, s)
        assert args
        A.update_textures(args)
        stats = A.last_update
        ra = records(A, n_meshes)
        flips = flipped_materials(held, s)
        base = expected_launches(ra["lighting"], held, s, args)
        print(f"{tag}: textures {sorted(args)} flips {flips} update {stats}, {base} launches before the chain")
        assert stats["ms_total"] > 0
        if flips:
            assert stats["launches"] >= base + 2 * sum(1 for m in s.meshes if set(flips) & set(int(x) for x in m.faces[:, 3])), tag
        else:
            assert stats["launches"] == base, f"{tag}: no flag changed: no chain kernel runs"
        for m in range(len(s.materials)):
            assert bool(ra["lighting"]["materials"]["flags"][m] & MAT_HAS_ALPHA) == has_alpha(s, m), f"{tag}: flag of material {m}"
        if back:
            same_records(ra, first, tag)
            if render:
                same_render(render_all(A, p), r0, tag)
            break
        B = api.DeviceScene(s, device=0)
        same_records(ra, records(B, n_meshes), tag)
        if render:
            current = None
            for ftag, flags in FLAGS.items():
                fa, fb = render_all(A, p, flags), render_all(B, p, flags)
                same_render(fa, fb, f"{tag} {ftag}")
                current = current or fa
            assert (bits(current["frame"]) != bits(previous["frame"])).any(), f"{tag}: the update does not change the frame"
            previous = current
        B.close()
        held = s
    A.close()
    return first


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,c", SIZES)
def test_sizes_and_channels(gpu_api, w, h, c):
    """2 x 2, 5 x 3 and 3 x 3 texels with 1 to 4 channels: the texture behind the listed one, and the pad bytes of both, are unchanged."""
    states, p = build_case(f"size_{w}x{h}x{c}")
    first = run_case(gpu_api, f"size_{w}x{h}x{c}", states, p)
    _, _, tex = size_scene(w, h)
    A = gpu_api.DeviceScene(states[0], device=0)
    A.update_textures(update_args(states[0], states[1]))
    got = A.texture_records()
    A.close()
    td, u8 = got["textures"], got["tex_u8"]
    t, nbytes = tex[c], w * h * c
    start = int(td[t]["offset"])
    end = int(td[t + 1]["offset"])
    assert end == (start + nbytes + 3) // 4 * 4 and int(td[t + 1]["width"]) == 3
    assert u8[start:start + nbytes].tobytes() == states[1].textures[t].data.tobytes()
    assert not u8[start + nbytes:end].any(), "pad bytes stay 0"
    assert u8[end:end + 12].tobytes() == first["textures"]["tex_u8"][end:end + 12].tobytes(), "the texture behind it and its pad bytes"
    assert u8[:start].tobytes() == first["textures"]["tex_u8"][:start].tobytes()


@pytest.mark.gpu
def test_record_forms(gpu_api):
    """A map with records of its own, a three-member bundle shared by two materials (one member, then all three in one call), a
    two-member bundle, and a base map that one material bundles and another samples directly: both places are rewritten."""
    states, p = build_case("forms")
    first = run_case(gpu_api, "forms", states, p)
    _, _, t = forms_scene()
    rec = first["lighting"]
    assert len(rec["tex_quads"]) > 0
    assert [len(places(rec, t[k])) for k in ("alone", "b3_base", "b3_normal", "b3_mr", "b2_base", "b2_mr", "sh_base", "sh_mr")] == [1, 1, 1, 1, 1, 1, 2, 1]
    assert rec["textures"][t["b3_base"]]["quad_offset"] == NO_QUADS and rec["textures"][t["sh_base"]]["quad_offset"] != NO_QUADS
    assert len(rec["textures"]) == len(states[0].textures) + 3 + 3 + 2 + 2, "one clone per material and member"


@pytest.mark.gpu
def test_a_scene_without_footprint_records(gpu_api, monkeypatch):
    """The same scene created under YART_TEX_QUADS_MAX_MB=0: no records, the kernels take plain taps, nothing but the reductions runs."""
    monkeypatch.setenv("YART_TEX_QUADS_MAX_MB", "0")
    states, p = build_case("forms")
    first = run_case(gpu_api, "forms without records", states, p)
    assert len(first["lighting"]["tex_quads"]) == 0
    A = gpu_api.DeviceScene(states[0], device=0)
    A.update_textures(update_args(states[0], states[2]))
    assert A.last_update["launches"] == 1, "three members of a bundle: one reduction (the base map), no record kernels"
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", REDUCE_SIZES)
def test_alpha_reduction(gpu_api, w, h):
    """4 to 258 texels, the map's first word at every offset of a 16-byte line: exactly one alpha byte of 254 at the first texel, the
    last, and at 63 / 64 and 255 / 256 where they exist, all 255 in between, all 0 at the end — the flag, and everything that follows
    from it, equals the fresh scene's every time."""
    states, p, t = reduce_states(w, h)
    run_case(gpu_api, f"reduce_{w}x{h}", states, p, render=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLIP_CASES)
def test_flips_on_and_off(gpu_api, name):
    """The chain for a flag that turns on, stays (new texels, no chain kernel) and turns off: the leaf records' alpha bit with the
    transparent bit and the long-span word untouched, the link words' alpha bit, the mesh's flag."""
    api = gpu_api
    states, p, t = flip_states(name)
    run_case(api, name, states, p)
    cut = states[0] if name == "instances" else states[1]
    B = api.DeviceScene(cut, device=0)
    meshes = [B.mesh_records(m) for m in range(len(cut.meshes))]
    B.close()
    link = np.concatenate([m["nodes"]["link"] for m in meshes])
    if name == "tri":
        assert len(meshes[-1]["nodes"]) == 1 and meshes[-1]["nodes"]["span"][0] == 1 and meshes[-1]["mesh"]["has_alpha"] == 1
    if name == "mixed":
        with_bit = (meshes[-1]["nodes"]["link"] & LINK_ALPHA) != 0
        assert with_bit.any() and not with_bit.all(), "some link words gain the bit and some do not"
        assert not (meshes[0]["nodes"]["link"] & LINK_ALPHA).any() and meshes[0]["mesh"]["has_alpha"] == 0
    if name == "stacked":
        nodes, leaves = meshes[-1]["nodes"], meshes[-1]["leaves"]
        spans = sorted(int(s) for s in nodes["span"] if s)
        assert 40 in spans and spans[-1] == 64
        for n in nodes[nodes["span"] >= 31]:
            first = int(n["link"]) & ((1 << 26) - 1)
            assert (int(n["link"]) >> 27) == 31 and (int(leaves["mat_flags"][first]) >> 8) == int(n["span"]), "saturated span, long-span word"
    if name == "instances":
        pane = next(m for m in meshes if len(m["leaves"]) == 2)
        assert ((pane["leaves"]["mat_flags"] & 0xff) == MAT_TRANSPARENT).all() and pane["mesh"]["has_alpha"] == 0
        assert sum(int(m["mesh"]["has_alpha"]) for m in meshes) == 1
    assert (link & LINK_ALPHA).any()


def child_device_pixels():
    """(in a process of its own, torch imported first) the same updates from torch uint8 tensors on the device and from NumPy arrays"""
    import torch
    from yart_amd import api
    for name, states in (("forms", build_case("forms")[0]), ("mixed", flip_states("mixed")[0])):
        n_meshes = len(states[0].meshes)
        A, D = api.DeviceScene(states[0], device=0), api.DeviceScene(states[0], device=0)
        for k, (held, s) in enumerate(zip(states, states[1:] + [states[0]])):
            args = update_args(held, s)
            A.update_textures(args)
            host_stats = A.last_update
            tensors = {t: torch.from_numpy(np.ascontiguousarray(px)).to("cuda:0") for t, px in args.items()}
            torch.cuda.synchronize()
            D.update_textures(tensors)
            assert D.last_update["launches"] == host_stats["launches"]
            ra, rd = records(A, n_meshes), records(D, n_meshes)
            assert ra["textures"]["tex_u8"].tobytes() == rd["textures"]["tex_u8"].tobytes(), f"{name} step {k}: texels"
            for key in ("materials", "tex_quads", "textures"):
                assert ra["lighting"][key].tobytes() == rd["lighting"][key].tobytes(), f"{name} step {k}: {key}"
            for ma, md in zip(ra["meshes"], rd["meshes"]):
                assert all(ma[key].tobytes() == md[key].tobytes() for key in ("mesh", "nodes", "leaves")), f"{name} step {k}: meshes"
        # the library's host copy followed the device pixels: a later update of a neighbour leaves these texels alone
        A.close()
        D.close()
    s, _, tex = size_scene(5, 3)
    D = api.DeviceScene(s, device=0)
    px = texels(5, 3, 1, 77)
    D.update_textures({tex[1]: torch.from_numpy(px[..., 0].copy()).to("cuda:0")})          # (H, W) for one channel
    B = api.DeviceScene(with_texels(s, {tex[1]: px}), device=0)
    assert D.texture_records()["tex_u8"].tobytes() == B.texture_records()["tex_u8"].tobytes()
    for bad in (torch.zeros((3, 5, 1), dtype=torch.uint8), torch.zeros((3, 5, 1), dtype=torch.float32, device="cuda:0"),
                torch.zeros((3, 10, 1), dtype=torch.uint8, device="cuda:0")[:, ::2]):
        with pytest.raises(api.YartError):
            D.update_textures({tex[1]: bad})
    D.close()
    B.close()
    print("device pixels ok")


@pytest.mark.gpu
def test_device_pixels_give_the_same_bytes(gpu_api):
    code = "import torch\ntorch.cuda.set_device(0)\nfrom tests import test_texture_update as t\nt.child_device_pixels()\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "device pixels ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def moved_and_deformed(s, mesh, node):
    """a copy with the node translated and the mesh's positions scaled"""
    from yart_amd import yscn
    f = copy.deepcopy(s)
    f.nodes[node].fwd, f.nodes[node].inv = yscn.trs(translation=(0.3, 0.2, -0.5))
    f.meshes[mesh].positions = np.ascontiguousarray(s.meshes[mesh].positions * np.float32(0.9) + np.float32(0.25))
    return f


@pytest.mark.gpu
def test_a_flip_combines_with_the_other_entries(gpu_api):
    """A texture flip, then update_lighting(materials): the new flag is kept. update_meshes, a flip, update_meshes again on the
    affected mesh: equal to fresh (the mesh update's cached "a face has an alpha-tested material" is forgotten). The four entries in
    two orders against a scene created from the final description."""
    api = gpu_api
    states, p, t = flip_states("mixed")
    s0, cut = states[0], states[1]
    mesh, node = len(s0.meshes) - 1, len(s0.nodes) - 1
    n_meshes = len(s0.meshes)
    flipped = next(m for m in range(len(s0.materials)) if s0.materials[m].tex_base == t)

    final = copy.deepcopy(cut)
    final.materials[flipped].roughness = 0.3
    final.materials[flipped].base = (0.9, 0.7, 0.5)
    B = api.DeviceScene(final, device=0)
    want, frame = records(B, n_meshes), render_all(B, p)
    B.close()
    A = api.DeviceScene(s0, device=0)
    A.update_textures({t: cut.textures[t].data})
    A.update_lighting(materials=final.materials)
    got = records(A, n_meshes)
    assert got["lighting"]["materials"]["flags"][flipped] & MAT_HAS_ALPHA
    same_records(got, want, "flip, then materials")
    same_render(render_all(A, p), frame, "flip, then materials")
    A.close()

    final = moved_and_deformed(cut, mesh, node)
    final.nodes[node] = copy.deepcopy(cut.nodes[node])
    B = api.DeviceScene(final, device=0)
    want = records(B, n_meshes)
    frames = {tag: render_all(B, p, flags) for tag, flags in FLAGS.items()}
    B.close()
    A = api.DeviceScene(s0, device=0)
    A.update_meshes({mesh: s0.meshes[mesh].positions})         # (the mesh update looks at the materials' flags and remembers)
    A.update_textures({t: cut.textures[t].data})
    A.update_meshes({mesh: final.meshes[mesh].positions})
    same_records(records(A, n_meshes), want, "mesh update, flip, mesh update")
    for tag, flags in FLAGS.items():
        same_render(render_all(A, p, flags), frames[tag], f"mesh update, flip, mesh update {tag}")
    A.close()

    final = moved_and_deformed(cut, mesh, node)
    final.materials[flipped].roughness = 0.3
    final.materials[0].base = (0.3, 0.6, 0.9)
    B = api.DeviceScene(final, device=0)
    want, want_graph = records(B, n_meshes), B.scene_graph()
    frames = {tag: render_all(B, p, flags) for tag, flags in FLAGS.items()}
    B.close()
    arrays = {mesh: final.meshes[mesh].positions}

    def transforms_first(A):
        A.update(final.nodes)
        A.update_meshes(arrays)
        A.update_lighting(materials=final.materials)
        A.update_textures({t: final.textures[t].data})

    def textures_first(A):
        A.update_textures({t: final.textures[t].data})
        A.update_lighting(materials=final.materials)
        A.update_meshes(arrays)
        A.update(final.nodes)

    for order in (transforms_first, textures_first):
        A = api.DeviceScene(s0, device=0)
        order(A)
        tag = order.__name__
        same_records(records(A, n_meshes), want, tag)
        for a, b in zip(A.scene_graph()[:2], want_graph[:2]):
            assert np.array_equal(raw(a), raw(b)), f"{tag}: scene graph"
        for ftag, flags in FLAGS.items():
            same_render(render_all(A, p, flags), frames[ftag], f"{tag} {ftag}")
        A.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(gpu_api):
    """Every YART_E_INVALID condition of the entry once; after each the probes' arrays and the frame are what they were."""
    from yart_amd import yscn
    api = gpu_api
    L = api.lib()
    s, p, t = forms_scene()
    spare = s.add_texture(yscn.Texture(np.full((4, 4, 3), 0.5, np.float32), yscn.TEX_LINEAR))
    w, h = FORM_SIZE
    n_meshes = len(s.meshes)
    A = api.DeviceScene(s, device=0)
    before, frame = records(A, n_meshes), render_all(A, p)
    clone = len(s.textures)
    assert len(before["lighting"]["textures"]) > clone and before["lighting"]["textures"][clone]["quad_stride"] == 64
    good, good2 = rgba(w, h, 90, "cut"), texels(w, h, 2, 91)
    keep = []

    def entries(*items):
        a = (api.TextureUpdate * max(len(items), 1))()
        for k, (tex, ew, eh, ec, px, flags) in enumerate(items):
            if px is not None:
                px = np.ascontiguousarray(px)
                keep.append(px)
            a[k] = api.TextureUpdate(tex, ew, eh, ec, px.ctypes.data if px is not None else None, flags)
        return a

    size = ctypes.sizeof(api.SceneTextureUpdate)
    U = api.SceneTextureUpdate
    one = entries((t["alone"], w, h, 4, good, 0))
    cases = [
        ("scene NULL", None, U(size, 1, one, 0), None),
        ("update NULL", A.handle, None, None),
        ("struct_size", A.handle, U(size - 8, 1, one, 0), None),
        ("flags", A.handle, U(size, 1, one, 1), None),
        ("n_textures 0", A.handle, U(size, 0, one, 0), None),
        ("textures NULL", A.handle, U(size, 1, None, 0), None),
        ("entry flags", A.handle, U(size, 1, entries((t["alone"], w, h, 4, good, 2)), 0), None),
        ("index out of range", A.handle, U(size, 1, entries((10000, w, h, 4, good, 0)), 0), None),
        ("a clone's index", A.handle, U(size, 1, entries((clone, w, h, 4, good, 0)), 0), None),
        ("listed twice", A.handle, U(size, 3, entries((t["alone"], w, h, 4, good, 0), (t["b2_mr"], w, h, 2, good2, 0), (t["alone"], w, h, 4, good, 0)), 0), None),
        ("float texture", A.handle, U(size, 1, entries((spare, 4, 4, 3, np.zeros((4, 4, 3), np.uint8), 0)), 0), None),
        ("width", A.handle, U(size, 1, entries((t["alone"], w - 1, h, 4, good, 0)), 0), None),
        ("height", A.handle, U(size, 1, entries((t["alone"], w, h + 1, 4, good, 0)), 0), None),
        ("channels", A.handle, U(size, 1, entries((t["alone"], w, h, 3, good, 0)), 0), None),
        ("pixels NULL", A.handle, U(size, 2, entries((t["b2_mr"], w, h, 2, good2, 0), (t["alone"], w, h, 4, None, 0)), 0), None),
        ("stats struct_size", A.handle, U(size, 1, one, 0), api.SceneUpdateStats(4)),
    ]
    for what, handle, up, stats in cases:
        rc = L.yart_hip_scene_update_textures(handle, ctypes.byref(up) if up is not None else None, None, ctypes.byref(stats) if stats is not None else None)
        print(f"{what}: {rc} {L.yart_hip_last_error().decode()}")
        assert rc == api.YART_E_INVALID, what
        same_records(records(A, n_meshes), before, what)
        same_render(render_all(A, p), frame, what)
    # ... and the same arguments without a fault are taken
    st = api.SceneUpdateStats(ctypes.sizeof(api.SceneUpdateStats))
    ok = U(size, 2, entries((t["b2_mr"], w, h, 2, good2, 0), (t["alone"], w, h, 4, good, 0)), 0)
    assert L.yart_hip_scene_update_textures(A.handle, ctypes.byref(ok), None, ctypes.byref(st)) == 0, L.yart_hip_last_error()
    assert st.launches > 3
    after = records(A, n_meshes)
    assert after["textures"]["tex_u8"].tobytes() != before["textures"]["tex_u8"].tobytes()
    assert after["lighting"]["materials"]["flags"][len(s.materials) - 6] & MAT_HAS_ALPHA
    A.close()


@pytest.mark.gpu
def test_cpp_mirror_updates_a_scene(gpu_api, tmp_path):
    """yart::hip::DeviceScene::updateTextures (include/yart_hip.hpp) from a C++ program: the one-triangle case, its map cut out."""
    states, _, t = flip_states("tri")
    path = os.path.join(tmp_path, "tri.yscn")
    states[0].save(path)
    px = states[1].textures[t].data
    flipped = next(m for m in range(len(states[0].materials)) if states[0].materials[m].tex_base == t)
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n#include <cstring>\n'
                "int main(int, char** argv) {\n"
                "  try {\n"
                "    yart::hip::DeviceScene scene(argv[1], 0);\n"
                "    static const unsigned char px[] = {" + ", ".join(str(int(v)) for v in px.reshape(-1)) + "};\n"
                "    YartTextureUpdate e{};\n"
                f"    e.texture = {t}u; e.width = {px.shape[1]}u; e.height = {px.shape[0]}u; e.channels = 4u; e.pixels = px;\n"
                "    const YartSceneUpdateStats st = scene.updateTextures({e});\n"
                "    YartLightingProbe pr{};\n    pr.struct_size = sizeof(pr);\n"
                "    if (yart_hip_probe_lighting(scene.handle(), &pr)) return 3;\n"
                "    std::vector<unsigned char> mats(pr.n_materials * 176);\n    pr.materials = mats.data();\n"
                "    if (yart_hip_probe_lighting(scene.handle(), &pr)) return 3;\n"
                f"    unsigned flags = 0;\n    std::memcpy(&flags, mats.data() + {flipped} * 176 + 52, 4);\n"
                "    std::printf(\"%u %u\\n\", st.launches, flags);\n"
                "  } catch (const std::exception& e) { std::printf(\"error: %s\\n\", e.what()); return 2; }\n"
                "  return 0; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    launches, flags = (int(v) for v in r.stdout.split())
    B = gpu_api.DeviceScene(states[1], device=0)
    want = int(B.lighting_records()["materials"]["flags"][flipped])
    B.close()
    assert flags == want and flags & MAT_HAS_ALPHA and launches == 1 + 1 + 3, "records, reduction; leaf pass, scan, links"
