"""yart_hip_scene_update_meshes on the host: csrc/mesh_update.hpp — leaf records through the permutation, link words (alpha bit from a
prefix sum over a node's index range, saturated span), the long-span word, the alpha flag, the stack need, the vertex box — fed with
the host builder's tree, against host_scene.hpp::buildHostImage byte for byte (tests/meshupdatesim/meshupdatesim.cpp); the node
counts and stack needs the cases of tests/test_mesh_update.py rely on; and the argument checks that need no device.

The cases (build_case; frames of 48 x 32 at 4 spp), each a list of states of one scene that differ in vertex data only:
  cube       the two-cube cornell of test_scene_update_host._two_cubes, the shared 12-triangle cube mesh sheared
  wave24     cornell + the height field of scenes.heightfield on a 24 x 24 grid (1152 triangles), its phase shifted:
             y = 0.6 + 0.5 sin(3.1 x + t) cos(2.3 z) + 0.15 sin(11 x + 5 z + 2 t), t = 0, 0.35, 0.70, normals recomputed; the node
             count shrinks and grows
  wave40     the same on 40 x 40 (3200 triangles: nodes of devbvh::kBigSpan triangles and more)
  collapse   wave24 with every vertex at exactly (+0, 0.6, +0): one node, a single leaf of 1152 triangles (saturated span field,
             long-span word)
  alpha      scenes.alpha_instances with its card mesh bent: alpha bits of the link words, hasAlpha
  light      cornell with its (emissive) mesh scaled by 1.5: area, power, CDF, total power
  instances  scenes.instances(70, 4) with the instanced cube tapered: 64 nodes and more, the top-level hierarchy changes
  deep       scenes.deep_tree's scene with scenes.chain_mesh(80): the chain mesh (stack need 80 > 64) against the same faces with their triangles in a regular row
  negzero    the cube case with the cube's min x moved to exactly -0.0f: the vertex box keeps the sign"""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import updatesim
from tests.conftest import ROOT
from tests.test_scene_update_host import SIZE, SPP, _two_cubes

CASES = ["cube", "wave24", "wave40", "collapse", "alpha", "light", "instances", "deep"]
WAVE_T = (0.0, 0.35, 0.70)


def wave_scene(n, t):
    from yart_amd import scenes
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    b = scenes.MeshBuilder()

    def fn(U, V):
        x = (U - 0.5) * 9.0; z = (V - 0.5) * 9.0
        y = 0.6 + 0.5 * np.sin(3.1 * x + t) * np.cos(2.3 * z) + 0.15 * np.sin(11.0 * x + 5.0 * z + 2.0 * t)
        return x, y, z
    b.grid(fn, n, n, 0, flip=True)
    s.add_node(s.add_mesh(b.build()))
    s.create_area_lights()
    return s, p


def with_positions(s, mesh, positions):
    """a copy of the scene with one mesh's positions replaced (float32, same count)"""
    s1 = copy.deepcopy(s)
    positions = np.ascontiguousarray(positions, np.float32)
    assert positions.shape == s.meshes[mesh].positions.shape
    s1.meshes[mesh].positions = positions
    return s1


def row_of_triangles(n):
    """n small triangles with three vertices of their own each, side by side along x"""
    k = np.arange(n, dtype=np.float64)
    x0 = (k - n / 2.0) * 0.11
    tri = np.stack([np.stack([x0, np.full(n, -0.5), np.zeros(n)], -1), np.stack([x0 + 0.1, np.full(n, -0.5), np.zeros(n)], -1),
                    np.stack([x0 + 0.05, np.full(n, 1.5), np.full(n, 0.3)], -1)], 1)
    return tri.reshape(-1, 3).astype(np.float32)


def build_case(name):
    """-> (states: scenes that differ in vertex data only, params, meshes: the indices of the meshes that deform)"""
    from yart_amd import scenes
    if name in ("cube", "negzero"):
        s0, p = _two_cubes()
        mesh = len(s0.meshes) - 1
        pos = s0.meshes[mesh].positions.astype(np.float32).copy()
        if name == "cube":
            pos[:, 0] += np.float32(0.4) * pos[:, 1]                     # a shear
            pos[:, 1] *= np.float32(1.2)
        else:
            pos[pos[:, 0] < 0, 0] = np.float32(-0.0)
            assert np.signbit(pos[:, 0]).any() and (pos[:, 0] >= 0).all()
        return [s0, with_positions(s0, mesh, pos)], p, [mesh]
    if name in ("wave24", "wave40"):
        n = 24 if name == "wave24" else 40
        made = [wave_scene(n, t) for t in WAVE_T]
        assert len(made[0][0].meshes[1].faces) == 2 * n * n
        return [s for s, _ in made], made[0][1], [1]
    if name == "collapse":
        s0, p = wave_scene(24, 0.0)
        pos = np.zeros_like(s0.meshes[1].positions, dtype=np.float32)
        pos[:, 1] = np.float32(0.6)
        assert not np.signbit(pos).any()
        return [s0, with_positions(s0, 1, pos)], p, [1]
    if name == "alpha":
        s0, p = scenes.alpha_instances(SIZE[0], SIZE[1], SPP, 5)
        bush = next(i for i, m in enumerate(s0.meshes) if len(m.faces) > 100)
        pos = s0.meshes[bush].positions.astype(np.float32).copy()
        pos[:, 0] += np.float32(0.9) * pos[:, 1] * pos[:, 1]             # bent
        pos[:, 2] *= np.float32(1.3)
        return [s0, with_positions(s0, bush, pos)], p, [bush]
    if name == "light":
        s0, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
        mesh = s0.lights[0].mesh
        assert all(l.mesh == mesh for l in s0.lights)
        return [s0, with_positions(s0, mesh, s0.meshes[mesh].positions.astype(np.float32) * np.float32(1.5))], p, [mesh]
    if name == "instances":
        s0, p = scenes.instances(SIZE[0], SIZE[1], SPP, 4, n_instances=70, groups=4)
        assert len(s0.nodes) >= 64
        cube = len(s0.meshes) - 1
        pos = s0.meshes[cube].positions.astype(np.float32).copy()
        top = pos[:, 1] > 0
        pos[top, 0] *= np.float32(0.3); pos[top, 2] *= np.float32(0.3); pos[top, 1] *= np.float32(2.5)     # tapered and taller
        return [s0, with_positions(s0, cube, pos)], p, [cube]
    if name == "deep":
        s0, p = scenes.deep_tree(8, width=SIZE[0], height=SIZE[1], spp=SPP)
        chain = len(s0.meshes) - 1
        # (deep_tree's own ratio of 24 ends at 78 levels in f32; 21 is still above the builder's 20 bins)
        s0.meshes[chain] = scenes.chain_mesh(80, sorted({int(f[3]) for f in s0.meshes[chain].faces}), ratio=21.0)
        m = s0.meshes[chain]
        assert len(m.positions) == 3 * len(m.faces) and (np.sort(np.asarray(m.faces)[:, :3].reshape(-1)) == np.arange(len(m.positions))).all(), \
            "every triangle has vertices of its own"
        order = np.asarray(m.faces)[:, :3].reshape(-1)
        pos = np.zeros_like(m.positions, dtype=np.float32)
        pos[order] = row_of_triangles(len(m.faces))
        return [s0, with_positions(s0, chain, pos)], p, [chain]
    raise KeyError(name)


def deformed_nodes(s, meshes):
    return [i for i, n in enumerate(s.nodes) if n.mesh in meshes]


def update_arrays(s, meshes, normals=True):
    """the argument of DeviceScene.update_meshes for state s"""
    return {m: (s.meshes[m].positions, s.meshes[m].normals, s.meshes[m].tangents) if normals else (s.meshes[m].positions,) for m in meshes}


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    return updatesim.build_sim(str(tmp_path_factory.mktemp("meshupdatesim") / "meshupdatesim"), SIM_SOURCES)


SIM_SOURCES = ["meshupdatesim/meshupdatesim.cpp"]
TAGS = ("stack bound", "vPos", "lights", "areaPowerCdf", "totalPower", "nodes", "nodeWorld", "rebuilt tlas")


def run_sim(exe, tmp_path, s0, s1):
    out = updatesim.run_sim(exe, tmp_path, s0, s1, TAGS)
    meshes = {}
    for m in re.finditer(r"^mesh (\d+) changed (\d) nodes (\d+) was (\d+) need (\d+) was (\d+) alpha (\d)$", out, re.M):
        i, changed, nodes, nodes_was, need, need_was, alpha = (int(v) for v in m.groups())
        meshes[i] = dict(changed=bool(changed), nodes=nodes, nodes_was=nodes_was, need=need, need_was=need_was, alpha=alpha)
        for tag in ("node count", "nodes", "leaves", "hasAlpha", "stack need", "vertex box", "indices"):
            assert re.search(rf"^EQUAL mesh {i} {tag} ", out, re.M), (i, tag)
    return out, meshes


def host_tree(s, mesh):
    from yart_amd import api
    nodes, idx, _ = api.bvh_build(s.meshes[mesh].positions, s.meshes[mesh].faces, device=None)
    return nodes, idx


def stack_need(nodes):
    depth, need = np.zeros(len(nodes), np.int64), 0
    for k in range(len(nodes)):                               # children are allocated after their parent
        if nodes[k, 7]:
            need = max(need, int(depth[k]))
        else:
            depth[nodes[k, 6]] = depth[nodes[k, 6] + 1] = depth[k] + 1
    return need


@pytest.mark.parametrize("name", CASES + ["negzero"])
def test_rederived_mesh_equals_a_fresh_one_on_bytes(sim, tmp_path, name):
    """Every case, every step between its states and the way back: mesh_update.hpp over the host builder's tree of the new vertices
    == buildHostImage of the new scene — link-word nodes, leaf records, alpha flag, stack need, vertex box, permutation; then the stack
    bound, the lights and the nodes' boxes re-derived from them."""
    states, _, meshes = build_case(name)
    steps = list(zip(states[:-1], states[1:])) + [(states[-1], states[0])]
    for s0, s1 in steps:
        out, got = run_sim(sim, str(tmp_path), s0, s1)
        assert sorted(i for i, m in got.items() if m["changed"]) == sorted(meshes)
        if name == "negzero":
            assert (f"NEGATIVE_ZERO mesh {meshes[0]}" in out) == (s1 is states[1])
        if name == "alpha":
            assert got[meshes[0]]["alpha"] == 1 and any(m["alpha"] == 0 for m in got.values())
        if name == "collapse" and s1 is states[1]:
            assert got[1]["nodes"] == 1 and got[1]["need"] == 0
        if name == "deep":
            needs = (got[meshes[0]]["need_was"], got[meshes[0]]["need"])
            assert max(needs) > 64 > min(needs), needs


def test_node_counts_and_depths_the_cases_rely_on(built):
    """With the host builder (api.bvh_build(..., device=None); the device build gives the same tree): the node count of the wave meshes
    changes between the states, down and up; the collapsed mesh is one leaf of all its triangles; the chain mesh needs more than 64
    stack entries and the row of its triangles fewer; the alpha mesh is more than one leaf."""
    signs = set()
    for name, n in (("wave24", 24), ("wave40", 40)):
        states, _, _ = build_case(name)
        counts = [len(host_tree(s, 1)[0]) for s in states]
        print(name, counts)                                   # (measured: 1291, 1297, 1279 and 3689, 3681, 3689)
        assert all(a != b for a, b in zip(counts, counts[1:])), f"{name}: every step changes the count: {counts}"
        assert all(c <= 2 * 2 * n * n - 1 for c in counts)
        assert (counts[1] - counts[0]) * (counts[2] - counts[1]) < 0, f"{name}: the count shrinks and grows: {counts}"
        signs |= {np.sign(b - a) for a, b in zip(counts, counts[1:])}
    assert signs == {-1, 1}
    assert 2 * 40 * 40 >= 2048, "wave40's root is a node of kBigSpan triangles and more"
    states, _, meshes = build_case("collapse")
    nodes, _ = host_tree(states[1], 1)
    assert len(nodes) == 1 and nodes[0, 7] == 1152 and nodes[0, 6] == 0
    states, _, meshes = build_case("deep")
    deep, flat = (stack_need(host_tree(s, meshes[0])[0]) for s in states)
    print("deep", deep, flat)
    assert deep == 80 and 0 < flat < 64
    states, _, meshes = build_case("alpha")
    a, b = (len(host_tree(s, meshes[0])[0]) for s in states)
    assert a > 1 and b > 1
    states, _, meshes = build_case("cube")
    assert len(states[0].meshes[meshes[0]].faces) == 12


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), once, on the alpha case."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "meshupdatesim_san"), SIM_SOURCES, sanitized=True)
    states, _, _ = build_case("alpha")
    run_sim(exe, str(tmp_path), states[0], states[1])


def test_argument_errors_without_a_device(built):
    """NULL arguments, struct_size, flags and n_meshes = 0 are refused with YART_E_INVALID before a scene or a device is looked at; the
    entries are exported and bound."""
    from yart_amd import api
    L = api.lib()
    assert "yart_hip_scene_update_meshes" in api.EXPORTS and "yart_hip_probe_mesh" in api.EXPORTS
    assert ctypes.sizeof(api.MeshUpdate) == 32 and ctypes.sizeof(api.SceneMeshUpdate) == 24
    pos = np.zeros((3, 3), np.float32)
    one = (api.MeshUpdate * 1)(api.MeshUpdate(0, 3, pos.ctypes.data_as(ctypes.c_void_p), None, None))
    size = ctypes.sizeof(api.SceneMeshUpdate)
    up = api.SceneMeshUpdate(size, 1, one, 0)
    assert L.yart_hip_scene_update_meshes(None, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    assert L.yart_hip_probe_mesh(None, 0, None, None, None, None, None, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    fake = ctypes.c_void_p(0x1000)                            # a handle that is never dereferenced: the update itself is checked first
    assert L.yart_hip_scene_update_meshes(fake, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    for bad, word in ((api.SceneMeshUpdate(8, 1, one, 0), b"struct_size"), (api.SceneMeshUpdate(0, 1, one, 0), b"struct_size"),
                      (api.SceneMeshUpdate(size, 1, None, 0), b"null"), (api.SceneMeshUpdate(size, 1, one, 2), b"flags"),
                      (api.SceneMeshUpdate(size, 1, one, 0x80000001), b"flags"), (api.SceneMeshUpdate(size, 0, one, 0), b"n_meshes")):
        assert L.yart_hip_scene_update_meshes(fake, ctypes.byref(bad), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
    small = api.SceneUpdateStats(4)
    assert L.yart_hip_scene_update_meshes(fake, ctypes.byref(up), None, ctypes.byref(small)) == api.YART_E_INVALID
    assert b"stats" in L.yart_hip_last_error()
    assert L.yart_hip_abi_version() == 3


def test_cpp_mirror_and_struct_sizes(built, tmp_path):
    """YartMeshUpdate / YartSceneMeshUpdate have the ctypes mirrors' sizes for a C++ compiler, and yart::hip::DeviceScene::updateMeshes
    exists with the documented signature (include/yart_hip.hpp)."""
    from yart_amd import api
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %zu\\n\", sizeof(YartMeshUpdate), sizeof(YartSceneMeshUpdate));\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartMeshUpdate>&, bool, void*)"
                " = &yart::hip::DeviceScene::updateMeshes;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.MeshUpdate), ctypes.sizeof(api.SceneMeshUpdate)]
