"""yart_hip_scene_update on the host: csrc/scene_update.hpp — a child's contribution to its parent's box, the (value, index) fold and
the binary64 world box — against host_scene.hpp::buildHostImage, byte for byte (tests/sceneupdatesim/sceneupdatesim.cpp), and the
argument checks of the entry point that need no device.

The scenes and moves are those of tests/test_scene_update.py (CASES below), plus one in which the sign of a zero decides a byte.

THE SIGNED-ZERO CASE, worked out here. A child's contribution is bounds::fromPoints of eight corners: min over the corners minus
0.001f, max plus 0.001f. In round-to-nearest x - x and -x + x are +0, so a contribution's bound is never -0: two children cannot put
+0 and -0 on one bound. The one candidate that can carry -0 is the node's own mesh box (a vertex coordinate of -0.0f is kept as it
is). So the case is a parent whose own mesh has min x = -0.0f, with two children: a box [0, 1]^3 translated by exactly
(0.001f, 2, 0), whose contribution's min x is 0.001f - 0.001f = +0.0f, and one translated by (3, 2, 0). Bounds3::join lets the
later operand — a child — win the tie: the parent's bmin.x is +0.0f (bits 0x00000000), not the mesh's 0x80000000. The test checks
these bits on the NumPy side (float32 arithmetic below), the program reports the tie (`SIGNED_ZERO_TIE`: two candidates equal as
floats and different in bits) and every fold order reproduces buildHostImage's bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import updatesim
from tests.conftest import ROOT

SIZE, SPP = (48, 32), 4


def _compose(m, fwd):
    f = (np.asarray(m, np.float64) @ np.asarray(fwd, np.float64)).astype(np.float32)
    return f, np.linalg.inv(f.astype(np.float64)).astype(np.float32)


def _depths(nodes):
    d = []
    for n in nodes:
        d.append(0 if n.parent < 0 else d[n.parent] + 1)
    return d


def _mesh_nodes_under(nodes, roots):
    inside, out = set(roots), set()
    for i, n in enumerate(nodes):
        if n.parent in inside:
            inside.add(i)
    for i in inside:
        if nodes[i].mesh >= 0:
            out.add(i)
    return sorted(out)


def _two_cubes():
    """The two-cube cornell of tests/test_temporal_motion.py (cubes of edge 3 under the root), both cubes at the identity"""
    from yart_amd import scenes
    from yart_amd.yscn import Material
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    b = scenes.MeshBuilder()
    b.box((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), s.add_material(Material(base=(0.3, 0.5, 0.8), roughness=0.8)))
    cube = s.add_mesh(b.build())
    s.add_node(cube, 0)
    s.add_node(cube, 0)
    s.create_area_lights()
    return s, p


def build_case(name):
    """-> (scene at T0, scene at T1, params, moved: the mesh nodes whose world placement changes, pass_lights)"""
    from yart_amd import scenes
    from yart_amd.yscn import trs

    def make():
        if name == "identity":
            return _two_cubes()
        if name == "instances":
            return scenes.instances(SIZE[0], SIZE[1], SPP, 4, n_instances=70, groups=4)
        if name == "deep12":
            return scenes.deep_instances(depth=12, width=SIZE[0], height=SIZE[1], spp=SPP)
        if name == "deep80":
            return scenes.deep_instances(depth=80, width=SIZE[0], height=SIZE[1], spp=SPP)
        if name == "light":
            return scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
        raise KeyError(name)
    s0, p = make()
    s1, _ = make()
    depth = _depths(s1.nodes)
    if name == "identity":
        assert len(s0.nodes) < 16 and all(np.array_equal(n.fwd, np.eye(4, dtype=np.float32)) for n in s0.nodes)
        roots, moves = [2], {2: trs((0.5, 5.0, 3.0), (1, 2, 0.5), 0.7)[0]}
    elif name == "instances":
        assert len(s0.nodes) >= 64
        group = next(i for i, n in enumerate(s0.nodes) if n.mesh < 0 and n.parent == 0)
        leaves = [i for i, n in enumerate(s0.nodes) if n.mesh >= 0 and depth[i] == 2 and n.parent != group]
        picked = [leaves[3], leaves[20], leaves[40], leaves[30]]
        moves = {group: trs((0.6, 0.4, -0.3), (0, 1, 0), 0.3)[0], picked[0]: trs((0.0, 1.0, 0.5))[0], picked[1]: trs((-0.7, 0.2, 0.0))[0],
                 picked[2]: trs((0.3, -0.2, 0.8), (1, 0, 0), 0.5)[0], picked[3]: trs(scale=(1.7, 0.6, 1.2))[0]}
        roots = list(moves)
    elif name in ("deep12", "deep80"):
        levels = (3, 10) if name == "deep12" else (2,)
        picked = [max(i for i, d in enumerate(depth) if d == lv) for lv in levels]
        assert max(depth) + 1 == (12 if name == "deep12" else 80)
        moves = {k: trs((0.3, 0.2, 0.4) if j == 0 else (0.1, -0.15, 0.05), (0, 1, 1), 0.4)[0] for j, k in enumerate(picked)}
        roots = picked
    else:
        roots, moves = [1], {1: trs((0.4, -0.6, 0.3), scale=1.5)[0]}
    for k, m in moves.items():
        # a move in the parent's space; for the scaled instance in its own
        if name == "instances" and k == picked[3]:
            f = (np.asarray(s1.nodes[k].fwd, np.float64) @ m.astype(np.float64)).astype(np.float32)
            s1.nodes[k].fwd, s1.nodes[k].inv = f, np.linalg.inv(f.astype(np.float64)).astype(np.float32)
        else:
            s1.nodes[k].fwd, s1.nodes[k].inv = _compose(m, s1.nodes[k].fwd)
    s1.create_area_lights()
    lights_change = any(not np.array_equal(a.fwd, b.fwd) for a, b in zip(s0.lights, s1.lights))
    assert lights_change == (name in ("deep12", "deep80", "light")), name
    return s0, s1, p, _mesh_nodes_under(s1.nodes, roots), lights_change


CASES = ["identity", "instances", "deep12", "deep80", "light"]


def signed_zero_scenes():
    from yart_amd import scenes
    from yart_amd.yscn import Material, trs
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    mat = s.add_material(Material(base=(0.5, 0.5, 0.5), roughness=0.9))
    b = scenes.MeshBuilder()
    b.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), mat)
    unit = s.add_mesh(b.build())
    own = b.build()
    own.positions = own.positions.copy()
    own.positions[own.positions[:, 0] == 0.0, 0] = -0.0            # the parent's own mesh: min x is -0.0f
    assert np.signbit(own.positions[:, 0]).any()
    parent = s.add_node(s.add_mesh(own), 0)
    f = np.eye(4, dtype=np.float32)
    f[:3, 3] = (np.float32(0.001), 2.0, 0.0)
    a = s.add_node(unit, parent, f, np.linalg.inv(f.astype(np.float64)).astype(np.float32))
    s.add_node(unit, parent, *trs((3.0, 2.0, 0.0)))
    s.create_area_lights()
    # the arithmetic of the contribution, in float32: corner x = ((0 + 1 * 0) + 0 * y) + 0 * z) + 0.001f * 1 = 0.001f; minus the pad
    corner = np.float32(0.0) + np.float32(1.0) * np.float32(0.0) + f[0, 3] * np.float32(1.0)
    contribution = np.float32(corner - np.float32(0.001))
    assert contribution == 0 and not np.signbit(contribution)
    assert np.float32(-0.0) == contribution and np.signbit(np.float32(-0.0))            # equal as floats, different bits
    import copy
    s0 = copy.deepcopy(s)
    s0.nodes[a].fwd, s0.nodes[a].inv = trs((1.0, 2.0, 0.0))
    return s0, s, parent


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    return updatesim.build_sim(str(tmp_path_factory.mktemp("sceneupdatesim") / "sceneupdatesim"), SIM_SOURCES)


SIM_SOURCES = ["sceneupdatesim/sceneupdatesim.cpp"]
TAGS = [f"{order} {what}" for order in ("host-path", "ascending", "descending", "shuffled-7", "round-trip") for what in ("nodes", "nodeWorld")] + \
       ["rebuilt tlas", "lights", "areaPowerCdf", "totalPower"]


def run_sim(exe, tmp_path, s0, s1, seed=1):
    return updatesim.run_sim(exe, tmp_path, s0, s1, TAGS, seed)


@pytest.mark.parametrize("name", CASES)
def test_rederived_image_equals_a_fresh_one_on_bytes(sim, tmp_path, name):
    """Every case of tests/test_scene_update.py: scene_update.hpp over buildHostImage(T0) with T1's transforms == buildHostImage(T1):
    NodeDev records (all 176 bytes), nodeWorld, the rebuilt top-level hierarchy, lights, CDF, total power; ascending, descending and
    shuffled 7-way folds, the library's host path, and the way back."""
    s0, s1, _, moved, _ = build_case(name)
    assert moved
    out = run_sim(sim, str(tmp_path), s0, s1)
    first = out.splitlines()[0].split()
    assert int(first[1]) == len(s1.nodes)
    if name == "deep80":
        assert int(first[3]) == 80 > 64                 # more levels than kSceneUpdateMaxLevels


def test_signed_zero_tie(sim, tmp_path):
    """The case of the module docstring: the program sees the tie between -0.0f (own mesh box) and +0.0f (a child) on the parent's
    bmin.x, and all fold orders give buildHostImage's bytes."""
    s0, s1, parent = signed_zero_scenes()
    out = run_sim(sim, str(tmp_path), s0, s1, seed=3)
    assert f"SIGNED_ZERO_TIE {parent} 0" in out


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), once, on the 70-instance case."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "sceneupdatesim_san"), SIM_SOURCES, sanitized=True)
    s0, s1, _, _, _ = build_case("instances")
    run_sim(exe, str(tmp_path), s0, s1)


def test_argument_errors_without_a_device(built):
    """NULL arguments, struct_size and flags are refused with YART_E_INVALID before a scene or a device is looked at; the entries are
    exported and bound."""
    from yart_amd import api
    L = api.lib()
    assert "yart_hip_scene_update" in api.EXPORTS and "yart_hip_probe_scene_graph" in api.EXPORTS
    assert ctypes.sizeof(api.SceneUpdate) == 40 and ctypes.sizeof(api.SceneUpdateStats) == 24
    nodes = (api.NodeDesc * 1)()
    up = api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, nodes, 0, None, 0)
    assert L.yart_hip_scene_update(None, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    assert L.yart_hip_probe_scene_graph(None, None, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    # a handle that is never dereferenced: the update itself is checked first
    fake = ctypes.c_void_p(0x1000)
    assert L.yart_hip_scene_update(fake, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    for bad, word in ((api.SceneUpdate(8, 1, nodes, 0, None, 0), b"struct_size"), (api.SceneUpdate(0, 1, nodes, 0, None, 0), b"struct_size"),
                      (api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, None, 0, None, 0), b"null"),
                      (api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, nodes, 0, None, 2), b"flags"),
                      (api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, nodes, 0, None, 0x80000001), b"flags")):
        assert L.yart_hip_scene_update(fake, ctypes.byref(bad), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
    assert L.yart_hip_abi_version() == 3


def test_cpp_mirror_and_struct_sizes(built, tmp_path):
    """YartSceneUpdate / YartSceneUpdateStats have the ctypes mirrors' sizes for a C++ compiler, and yart::hip::DeviceScene::update
    exists with the documented signature (include/yart_hip.hpp)."""
    from yart_amd import api
    src = os.path.join(tmp_path, "u.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %zu %u\\n\", sizeof(YartSceneUpdate), sizeof(YartSceneUpdateStats), YART_UPDATE_REBUILD_TOP);\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartNodeDesc>&, const std::vector<YartLightDesc>&, bool, void*)"
                " = &yart::hip::DeviceScene::update;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "u")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.SceneUpdate), ctypes.sizeof(api.SceneUpdateStats), api.UPDATE_REBUILD_TOP]
