"""yart_hip_scene_replace_meshes on the host: csrc/mesh_replace.hpp — create's layout of the four offsets from the meshes' counts, the
segment tables, the repack with the triIdx delta, the zero pad records and the two tail records of bvhNodes, the ShadeTri derivation —
together with mesh_update.hpp's derivation over the host builder's tree, against host_scene.hpp::buildHostImage of the new
description byte for byte, pool by pool (tests/meshreplacesim/meshreplacesim.cpp); the counts the cases of tests/meshreplacecases.py
rely on; mutated scratch copies of the header, each of which has to make a case differ; and the argument checks that need no device."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import updatesim
from tests.conftest import ROOT
from tests.meshreplacecases import CASES, build_case, listed

SIM_SOURCES = ["meshreplacesim/meshreplacesim.cpp"]
POOLS = ("meshes", "shadeTris", "leafTris", "triVerts", "triLight", "vPos", "vNormal", "vTangent", "vUV", "bvhNodes")
TAGS = POOLS + ("stack bound", "nodes", "nodeWorld")
LINE = re.compile(r"^mesh (\d+) listed (\d) tris (\d+) was (\d+) verts (\d+) was (\d+) nodes (\d+) was (\d+) base (\d+) was (\d+) delta (-?\d+)$", re.M)
KEYS = ("listed", "tris", "tris_was", "verts", "verts_was", "nodes", "nodes_was", "base", "base_was", "delta")


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    return updatesim.build_sim(str(tmp_path_factory.mktemp("meshreplacesim") / "meshreplacesim"), SIM_SOURCES)


def steps_of(states):
    return list(zip(states[:-1], states[1:])) + ([(states[-1], states[0])] if states[-1] is not states[0] else [])


def run_sim(exe, tmp_path, s0, s1):
    out = updatesim.run_sim(exe, tmp_path, s0, s1, TAGS)
    meshes = {int(m.group(1)): dict(zip(KEYS, (int(v) for v in m.groups()[1:]))) for m in LINE.finditer(out)}
    assert len(meshes) == len(s1.meshes)
    for i in listed(s0, s1):
        for tag in ("stack need", "vertex box", "indices"):
            assert re.search(rf"^EQUAL mesh {i} {tag} ", out, re.M), (i, tag)
    return out, meshes


@pytest.mark.parametrize("name", CASES)
def test_repacked_pools_equal_a_fresh_scene_on_bytes(sim, tmp_path, name):
    """Every case, every step between its states and the way back: layout, segment tables, staged records and repack == buildHostImage of
    the new scene in every pool, in the MeshDev records, the stack bound and the nodes' boxes — and the step does to the layout what
    the case is there for."""
    states, _ = build_case(name)
    for k, (s0, s1) in enumerate(steps_of(states)):
        _, got = run_sim(sim, str(tmp_path), s0, s1)
        changed = listed(s0, s1)
        assert sorted(i for i, m in got.items() if m["listed"]) == changed and changed
        first = k == 0
        if name == "grow_first" and first:
            assert changed == [0] and (got[0]["tris_was"], got[0]["tris"]) == (12, 44) and got[0]["verts"] > got[0]["verts_was"]
            assert got[1]["delta"] == got[2]["delta"] == 32
        if name == "shrink_middle" and first:
            assert changed == [1] and got[2]["delta"] == 12 - 80 and got[0]["delta"] == 0
            assert got[2]["base"] < got[2]["base_was"]
        if name == "last":
            assert changed == [2] and all(got[i]["delta"] == 0 and got[i]["base"] == got[i]["base_was"] for i in range(3))
        if name == "same_counts":
            m = got[1]
            assert changed == [1] and (m["tris"], m["verts"], m["nodes"]) == (m["tris_was"], m["verts_was"], m["nodes_was"]), "the fast path's condition"
        if name == "two" and first:
            assert changed == [0, 2] and got[0]["tris"] - got[0]["tris_was"] == got[2]["tris_was"] - got[2]["tris"] == 24
            assert got[0]["verts"] - got[0]["verts_was"] == got[2]["verts_was"] - got[2]["verts"] > 0
            assert got[1]["delta"] == 24 and got[3]["delta"] == 0
        if name == "single_leaf" and k in (0, 2):
            i = changed[0]
            assert (got[i]["tris"], got[i]["nodes"]) == (1, 1)
            # (a binary tree has an odd node count, so behind every mesh the running count is even and a pad record follows: the bases
            # stay odd, and every later mesh moves by the difference of the two node counts)
            assert all(m["base"] % 2 == 1 for m in got.values())
            assert all(got[j]["base"] - got[j]["base_was"] == got[i]["nodes"] - got[i]["nodes_was"] for j in got if j > i)
        if name == "lod":
            assert changed == [1]
        if name == "deep" and first:
            assert changed == [len(s0.meshes) - 1]


def test_counts_the_cases_rely_on(built):
    """The fixtures alone (this test needs nothing of the entry: it says that the cases are what the other tests take them for). With
    the host builder (the device build gives the same tree): the re-triangulated patch of same_counts keeps its node count; the
    height fields of lod lie on both sides of devbvh::kBigSpan; the chain mesh of deep needs 80 stack entries, the row few; the
    alpha case brings a textured material to a mesh that had none."""
    from tests.test_mesh_update_host import host_tree, stack_need
    states, _ = build_case("same_counts")
    a, b = (len(host_tree(s, 1)[0]) for s in states)
    assert a == b and a > 1, (a, b)
    assert not np.array_equal(states[0].meshes[1].faces, states[1].meshes[1].faces)
    assert len(set(states[1].meshes[1].faces[:, 3].tolist())) == 3
    states, _ = build_case("lod")
    tris = [len(s.meshes[1].faces) for s in states]
    assert tris == [1152, 4608, 288, 1152] and max(tris) >= 2048 > tris[0]
    states, _ = build_case("deep")
    chain = len(states[0].meshes) - 1
    deep, flat = (stack_need(host_tree(s, chain)[0]) for s in states)
    assert deep == 80 and 0 < flat < 64, (deep, flat)
    states, _ = build_case("alpha")
    mesh = listed(states[0], states[1])[0]
    leaf = int(states[1].meshes[mesh].faces[0, 3])
    assert states[0].materials[leaf].tex_base >= 0 and leaf not in set(states[0].meshes[mesh].faces[:, 3].tolist())


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), once, on the two case."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "meshreplacesim_san"), SIM_SOURCES, sanitized=True)
    states, _ = build_case("two")
    run_sim(exe, str(tmp_path), states[0], states[1])


# (what, the text of csrc/mesh_replace.hpp it replaces, the replacement): README's table is this test's printout
MUTATIONS = [
    ("delta dropped", "s.delta = n.triOffset - o.triOffset;", "s.delta = 0u;"),
    ("delta's sign flipped", "s.delta = n.triOffset - o.triOffset;", "s.delta = o.triOffset - n.triOffset;"),
    ("pad parity inverted", "if (nodes % 2u == 0u) nodes++;", "if (nodes % 2u == 1u) nodes++;"),
    ("tail records left out", "nodes += 2u; ", "nodes += 0u; "),
    ("uv of vertex 0 for all corners", "st.uv[k][c] = uvs[2u * size_t(vi[k]) + c];", "st.uv[k][c] = uvs[2u * size_t(vi[0]) + c];"),
    ("light left 0", "st.light = -1;", "st.light = 0;"),
]


def test_every_mutation_of_the_header_makes_a_case_differ(built, tmp_path):
    """Scratch copies of the host headers with one statement of mesh_replace.hpp changed, the simulator built on each: every mutation
    makes at least one step of one case DIFFERENT (the counts per case are printed: README's table)."""
    pairs = []
    for name in CASES:
        states, _ = build_case(name)
        for k, (s0, s1) in enumerate(steps_of(states)):
            a, b = os.path.join(tmp_path, f"{name}{k}a.yscn"), os.path.join(tmp_path, f"{name}{k}b.yscn")
            s0.save(a); s1.save(b)
            pairs.append((name, a, b))
    text = open(os.path.join(ROOT, "yart_amd", "csrc", "mesh_replace.hpp")).read()
    table = {}
    for k, (what, old, new) in enumerate(MUTATIONS):
        assert text.count(old) == 1, what
        tree = os.path.join(tmp_path, f"m{k}")
        os.makedirs(os.path.join(tree, "yart_amd", "csrc")); os.makedirs(os.path.join(tree, "include")); os.makedirs(os.path.join(tree, "tests", "meshreplacesim"))
        for h in glob.glob(os.path.join(ROOT, "yart_amd", "csrc", "*.hpp")):
            shutil.copy(h, os.path.join(tree, "yart_amd", "csrc"))
        shutil.copy(os.path.join(ROOT, "include", "yart_hip.h"), os.path.join(tree, "include"))
        shutil.copy(os.path.join(ROOT, "tests", SIM_SOURCES[0]), os.path.join(tree, "tests", "meshreplacesim"))
        with open(os.path.join(tree, "yart_amd", "csrc", "mesh_replace.hpp"), "w") as f:
            f.write(text.replace(old, new))
        exe = os.path.join(tree, "sim")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(tree, "tests", SIM_SOURCES[0]),
                            os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lz", "-lpthread"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        counts = {name: 0 for name in CASES}
        for name, a, b in pairs:
            r = subprocess.run([exe, a, b], capture_output=True, text=True)
            assert r.returncode in (0, 1), r.stderr[-2000:]
            counts[name] += 1 if "DIFFERENT" in r.stdout else 0
        table[what] = counts
        print(f"{what:<32}" + " ".join(f"{name}={counts[name]}" for name in CASES))
    for what, counts in table.items():
        assert sum(counts.values()) >= 1, f"{what}: no case differs"


def test_argument_errors_without_a_device(built):
    """NULL arguments, struct_size, flags and n_meshes = 0 are refused with YART_E_INVALID before a scene or a device is looked at; the
    entries are exported and bound."""
    from yart_amd import api
    L = api.lib()
    assert "yart_hip_scene_replace_meshes" in api.EXPORTS and "yart_hip_probe_geometry" in api.EXPORTS
    assert ctypes.sizeof(api.MeshReplace) == 64 and ctypes.sizeof(api.SceneMeshReplace) == 24 and ctypes.sizeof(api.GeometryProbe) == 168
    one = (api.MeshReplace * 1)()
    size = ctypes.sizeof(api.SceneMeshReplace)
    up = api.SceneMeshReplace(size, 1, one, 0)
    assert L.yart_hip_scene_replace_meshes(None, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"scene_replace_meshes" in L.yart_hip_last_error() and b"null" in L.yart_hip_last_error()
    fake = ctypes.c_void_p(0x1000)                            # a handle that is never dereferenced: the update itself is checked first
    assert L.yart_hip_scene_replace_meshes(fake, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    for bad, word in ((api.SceneMeshReplace(8, 1, one, 0), b"struct_size"), (api.SceneMeshReplace(0, 1, one, 0), b"struct_size"),
                      (api.SceneMeshReplace(size, 1, None, 0), b"null"), (api.SceneMeshReplace(size, 1, one, 4), b"flags"),
                      (api.SceneMeshReplace(size, 1, one, 3), b"exclude"), (api.SceneMeshReplace(size, 1, one, 2), b"live scene"),
                      (api.SceneMeshReplace(size, 0, one, 0), b"n_meshes")):
        assert L.yart_hip_scene_replace_meshes(fake, ctypes.byref(bad), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
    small = api.SceneUpdateStats(4)
    assert L.yart_hip_scene_replace_meshes(fake, ctypes.byref(up), None, ctypes.byref(small)) == api.YART_E_INVALID
    assert b"stats" in L.yart_hip_last_error()
    assert L.yart_hip_probe_geometry(None, None) == api.YART_E_INVALID and b"null" in L.yart_hip_last_error()
    pr = api.GeometryProbe(8)
    assert L.yart_hip_probe_geometry(fake, ctypes.byref(pr)) == api.YART_E_INVALID and b"struct_size" in L.yart_hip_last_error()
    with pytest.raises(api.YartError):
        api.DeviceScene.replace_meshes(None, {}, rebuild_top=2)
    with pytest.raises(api.YartError):
        api.DeviceScene.replace_meshes(None, {0: (np.zeros((3, 3)), np.zeros((2, 3)), np.zeros((3, 4)), np.zeros((3, 2)), np.zeros((1, 4)))})
    assert L.yart_hip_abi_version() == 3


def test_cpp_mirror_and_struct_sizes(built, tmp_path):
    """YartMeshReplace / YartSceneMeshReplace / YartGeometryProbe have the ctypes mirrors' sizes for a C++ compiler, and
    yart::hip::DeviceScene::replaceMeshes exists with the documented signatures (include/yart_hip.hpp)."""
    from yart_amd import api
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %zu %zu\\n\", sizeof(YartMeshReplace), sizeof(YartSceneMeshReplace), sizeof(YartGeometryProbe));\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartMeshReplace>&, bool, void*)"
                " = &yart::hip::DeviceScene::replaceMeshes;\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fm)(const std::vector<YartMeshReplace>&, yart::hip::DeviceScene::TopLevel, void*)"
                " = &yart::hip::DeviceScene::replaceMeshes;\n"
                "  return fn && fm ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.MeshReplace), ctypes.sizeof(api.SceneMeshReplace), ctypes.sizeof(api.GeometryProbe)]
