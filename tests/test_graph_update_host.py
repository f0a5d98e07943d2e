"""yart_hip_scene_update_graph on the host: csrc/graph_update.hpp — the integer pass over a new node list (skip links, depths, the .w
words of the world boxes, identity flags, the level tables, the leaf list) — with scene_update.hpp and buildTopLevel against
host_scene.hpp::buildHostImage of the new scene, byte for byte (tests/graphupdatesim/graphupdatesim.cpp), and the argument checks of
the entry point that need no device.

The cases (graph_case) are those of tests/test_graph_update.py: the smallest shapes at which a changed node list can go wrong.
  hide / remove / add / swap   the two-cube cornell (7 nodes: the LDS form): a cube hidden (mesh = -1), removed, a third one added, a
                               cube's mesh swapped for another mesh of the scene
  lean15-17                    scenes.instances with 15 and 17 nodes: kLeanSceneNodes = 16 between them
  mask63-64, mask60-70         63 / 64 and 60 / 70 nodes: the 64-bit candidate mask ends, the top-level hierarchy appears
  hide-all                     every mesh node of a 70-node scene hidden: 70 nodes and no leaf
  reparent                     an instance moved from one group to another, the list reordered to stay pre-order
  deep12, deep80               deep_instances(12) with a branch of two nodes, a 13th level, below level 10; deep_instances(80) with an 81st level: more
                               levels than kSceneUpdateMaxLevels, the host path
Every case runs in both directions (the program's round trip)."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import updatesim
from tests.conftest import ROOT

SIZE, SPP = (48, 32), 4


def two_cubes():
    """cornell + two cubes of edge 2.4 side by side and a second, smaller mesh that no node uses yet -> (scene, params, cube, small)"""
    from yart_amd import scenes
    from yart_amd.yscn import Material, trs
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    b = scenes.MeshBuilder()
    b.box((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2), s.add_material(Material(base=(0.3, 0.5, 0.8), roughness=0.8)))
    cube = s.add_mesh(b.build())
    b = scenes.MeshBuilder()
    b.box((-0.6, -1.8, -0.6), (0.6, 1.8, 0.6), s.add_material(Material(base=(0.8, 0.4, 0.2), roughness=0.5)))
    small = s.add_mesh(b.build())
    s.add_node(cube, 0, *trs((-2.0, 2.0, 0.5), (0, 1, 0), 0.3))
    s.add_node(cube, 0, *trs((2.0, 3.0, 1.0), (1, 1, 0), 0.5))
    s.create_area_lights()
    return s, p, cube, small


def with_nodes(s, nodes):
    """a copy of the scene with another node list (meshes, materials and LIGHTS as they are: lights do not depend on the nodes)"""
    s1 = copy.copy(s)
    s1.nodes = copy.deepcopy(list(nodes))
    return s1


def depths(nodes):
    d = []
    for n in nodes:
        d.append(0 if n.parent < 0 else d[n.parent] + 1)
    return d


def reordered(nodes, order):
    """the nodes in the order `order` (old indices), parents renumbered; asserts the result is in pre-order"""
    new_of = {old: new for new, old in enumerate(order)}
    out = []
    for new, old in enumerate(order):
        n = copy.deepcopy(nodes[old])
        n.parent = -1 if n.parent < 0 else new_of[n.parent]
        assert n.parent < new
        out.append(n)
    return out


def instances(n_nodes, groups):
    from yart_amd import scenes
    s, p = scenes.instances(SIZE[0], SIZE[1], SPP, 4, n_instances=n_nodes - 2 - groups, groups=groups)
    assert len(s.nodes) == n_nodes
    return s, p


def graph_case(name):
    """-> (scene before, scene after, params, shown: nodes of `after` that are new or changed and have a mesh, gone: nodes of `before`
    whose mesh the change takes away)"""
    from yart_amd import scenes
    from yart_amd.yscn import Node, trs
    if name in ("hide", "remove", "add", "swap"):
        s0, p, cube, small = two_cubes()
        last = len(s0.nodes) - 1
        nodes = copy.deepcopy(s0.nodes)
        if name == "hide":
            nodes[last - 1].mesh = -1
            return s0, with_nodes(s0, nodes), p, [], [last - 1]
        if name == "remove":
            return s0, with_nodes(s0, nodes[:-1]), p, [], [last]
        if name == "add":
            f, i = trs((0.0, 6.0, 0.0), (0, 0, 1), 0.4)
            nodes.append(Node(parent=0, mesh=cube, fwd=f, inv=i))
            return s0, with_nodes(s0, nodes), p, [last + 1], []
        nodes[last].mesh = small
        return s0, with_nodes(s0, nodes), p, [last], []
    if name in ("lean15-17", "mask63-64", "mask60-70"):
        a, b, groups = {"lean15-17": (15, 17, 2), "mask63-64": (63, 64, 4), "mask60-70": (60, 70, 4)}[name]
        (s0, p), (s1, _) = instances(a, groups), instances(b, groups)
        # (the generator draws the instances' placements in another order for another count: every node differs)
        return s0, with_nodes(s0, s1.nodes), p, [i for i, n in enumerate(s1.nodes) if n.mesh >= 0 and i >= 2], []
    if name == "hide-all":
        s0, p = instances(70, 4)
        nodes = copy.deepcopy(s0.nodes)
        gone = [i for i, n in enumerate(nodes) if n.mesh >= 0]
        for i in gone:
            nodes[i].mesh = -1
        return s0, with_nodes(s0, nodes), p, [], gone
    if name == "reparent":
        s0, p = instances(70, 4)
        groups = [i for i, n in enumerate(s0.nodes) if n.mesh < 0 and n.parent == 0]
        # the eighth instance of the first group (camera rays see it in either place) ...
        mover = [i for i, n in enumerate(s0.nodes) if n.parent == groups[0]][7]
        order = [i for i in range(len(s0.nodes)) if i != mover]
        at = order.index(groups[2])                                                          # ... becomes the last one of the second
        order.insert(at, mover)
        nodes = reordered(s0.nodes, order)
        moved = order.index(mover)
        nodes[moved].parent = order.index(groups[1])
        assert nodes[moved].parent < moved and nodes[moved - 1].parent == nodes[moved].parent
        return s0, with_nodes(s0, nodes), p, [moved], []
    if name in ("deep12", "deep80"):
        levels = 12 if name == "deep12" else 80
        s0, p = scenes.deep_instances(depth=levels, width=SIZE[0], height=SIZE[1], spp=SPP)
        d = depths(s0.nodes)
        assert max(d) + 1 == levels and d[-1] == levels - 1, "the spine ends the list"
        box = next(n.mesh for n in s0.nodes[2:] if n.mesh >= 0 and not any(l.mesh == n.mesh for l in s0.lights))
        nodes = copy.deepcopy(s0.nodes)
        if name == "deep12":                 # below the level-10 node, behind its subtree: a level-11 node and a level-12 child of it
            at = d.index(10)
            nodes.append(Node(parent=at, mesh=box, fwd=trs((0.5, 0.3, 0.2), (0, 1, 0), 0.5, (2.0, 2.0, 2.0))[0], inv=trs((0.5, 0.3, 0.2), (0, 1, 0), 0.5, (2.0, 2.0, 2.0))[1]))
            nodes.append(Node(parent=len(nodes) - 1, mesh=box, fwd=trs((0.0, 0.6, 0.0))[0], inv=trs((0.0, 0.6, 0.0))[1]))
            shown = [len(nodes) - 2, len(nodes) - 1]
        else:                                # an 81st level below the deepest node
            nodes.append(Node(parent=len(nodes) - 1, mesh=box, fwd=trs((0.0, 0.5, 0.0), scale=(3.0, 3.0, 3.0))[0], inv=trs((0.0, 0.5, 0.0), scale=(3.0, 3.0, 3.0))[1]))
            shown = [len(nodes) - 1]
        assert max(depths(nodes)) + 1 == levels + 1
        return s0, with_nodes(s0, nodes), p, shown, []
    raise KeyError(name)


CASES = ["hide", "remove", "add", "swap", "lean15-17", "mask63-64", "mask60-70", "hide-all", "reparent", "deep12", "deep80"]

SIM_SOURCES = ["graphupdatesim/graphupdatesim.cpp"]
FIELDS = ("nodes", "nodeWorld", "tlas", "tlasHeight", "stackBound", "maxNodeDepth", "allIdentity")


def tags(deep):
    paths = ("host-path",) if deep else ("host-path", "tables")
    return [f"{way}{path} {field}" for way in ("", "round-trip ") for path in paths for field in FIELDS] + \
           [f"{way}{what}" for way in ("", "round-trip ") for what in ("leafIds", "predicted tlas records", "predicted tlas height")]


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    return updatesim.build_sim(str(tmp_path_factory.mktemp("graphupdatesim") / "graphupdatesim"), SIM_SOURCES)


@pytest.mark.parametrize("name", CASES)
def test_rederived_image_equals_a_fresh_one_on_bytes(sim, tmp_path, name):
    """graph_update.hpp's pass + scene_update.hpp + buildTopLevel over buildHostImage(before) with the new list == buildHostImage(after):
    NodeDev records (all 176 bytes), nodeWorld with its .w words, the hierarchy, its height, the stack bound, the deepest level and
    allIdentity; by suRederiveHost and, for graphs of at most 64 levels, level by level over the pass's tables; and the way back."""
    s0, s1, _, shown, gone = graph_case(name)
    assert shown or gone
    out = updatesim.run_sim(sim, str(tmp_path), s0, s1, tags(name == "deep80"))
    head = out.splitlines()[0].split()
    assert (int(head[1]), int(head[3])) == (len(s0.nodes), len(s1.nodes))
    if name == "deep80":
        assert int(head[7]) == 81 > 64 and "no tables" in out          # more levels than kSceneUpdateMaxLevels
    if name in ("mask63-64", "mask60-70"):
        assert (int(head[9]), int(head[11])) == (1, 2 * sum(n.mesh >= 0 for n in s1.nodes) - 1), "the hierarchy appears"
    if name == "hide-all":
        assert int(head[9]) > 1 and int(head[11]) == 1, "70 nodes and no leaf: no hierarchy"


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), once, on the case in which the
    hierarchy appears and disappears."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "graphupdatesim_san"), SIM_SOURCES, sanitized=True)
    s0, s1, _, _, _ = graph_case("mask60-70")
    updatesim.run_sim(exe, str(tmp_path), s0, s1, tags(False))


def test_argument_errors_without_a_device(built):
    """NULL arguments, struct_size, flags, the node count and the list's order are refused with YART_E_INVALID before a scene or a
    device is looked at — and, with valid arguments, a handle that is no live scene for flags 0 as for the device flag; the entry is
    exported and bound."""
    from yart_amd import api
    L = api.lib()
    assert "yart_hip_scene_update_graph" in api.EXPORTS
    size = ctypes.sizeof(api.SceneGraphUpdate)
    assert size == 40
    nodes = (api.NodeDesc * 3)()
    eye = api._f(np.eye(4, dtype=np.float32), 16)
    for i in range(3):
        nodes[i] = api.NodeDesc(-1 if i == 0 else 0, -1, eye, eye)
    up = api.SceneGraphUpdate(size, 3, nodes, 0, None, 0)
    assert L.yart_hip_scene_update_graph(None, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()
    fake = ctypes.c_void_p(0x1000)                    # a handle that is never dereferenced
    assert L.yart_hip_scene_update_graph(fake, None, None, None) == api.YART_E_INVALID
    assert b"null" in L.yart_hip_last_error()

    keep = []

    def with_parents(*parents):
        nd = (api.NodeDesc * len(parents))()
        for i, parent in enumerate(parents):
            nd[i] = api.NodeDesc(parent, -1, eye, eye)
        keep.append(nd)
        return api.SceneGraphUpdate(size, len(parents), nd, 0, None, 0)
    small_stats = api.SceneUpdateStats(4)
    for bad, stats, word in ((api.SceneGraphUpdate(8, 3, nodes, 0, None, 0), None, b"struct_size"),
                             (api.SceneGraphUpdate(0, 3, nodes, 0, None, 0), None, b"struct_size"),
                             (api.SceneGraphUpdate(size, 3, None, 0, None, 0), None, b"null"),
                             (api.SceneGraphUpdate(size, 3, nodes, 0, None, 3), None, b"exclude"),
                             (api.SceneGraphUpdate(size, 3, nodes, 0, None, 4), None, b"unknown flags"),
                             (api.SceneGraphUpdate(size, 3, nodes, 0, None, 0x80000001), None, b"unknown flags"),
                             (api.SceneGraphUpdate(size, 0, nodes, 0, None, 0), None, b"n_nodes is 0"),
                             (api.SceneGraphUpdate(size, 1 << 20, nodes, 0, None, 0), None, b"n_nodes is 1048576"),
                             (with_parents(0, 0, 0), None, b"node 0"),
                             (with_parents(-1, 0, -1), None, b"node 2"),
                             (with_parents(-1, 1, 0), None, b"node 1"),
                             (with_parents(-1, 0, 2), None, b"node 2"),
                             (up, None, b"not a live scene"),
                             (api.SceneGraphUpdate(size, 3, nodes, 0, None, 2), None, b"not a live scene"),
                             (api.SceneGraphUpdate(size, 3, nodes, 0, None, 1), small_stats, b"stats")):
        rc = L.yart_hip_scene_update_graph(fake, ctypes.byref(bad), None, ctypes.byref(stats) if stats else None)
        assert rc == api.YART_E_INVALID and word in L.yart_hip_last_error(), (word, L.yart_hip_last_error())
    with pytest.raises(api.YartError, match="rebuild_top"):
        api.DeviceScene.update_graph(None, [], rebuild_top=False)
    assert L.yart_hip_abi_version() == 3


def test_cpp_mirror_and_struct_sizes(built, tmp_path):
    """YartSceneGraphUpdate has the ctypes mirror's size for a C++ compiler, and yart::hip::DeviceScene::updateGraph exists with the
    documented signature (include/yart_hip.hpp)."""
    from yart_amd import api
    src = os.path.join(tmp_path, "g.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n#include <cstddef>\n'
                "int main() { std::printf(\"%zu %zu %zu\\n\", sizeof(YartSceneGraphUpdate), offsetof(YartSceneGraphUpdate, lights), offsetof(YartSceneGraphUpdate, flags));\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartNodeDesc>&, const std::vector<YartLightDesc>&,"
                " yart::hip::DeviceScene::TopLevel, void*) = &yart::hip::DeviceScene::updateGraph;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "g")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.SceneGraphUpdate), api.SceneGraphUpdate.lights.offset, api.SceneGraphUpdate.flags.offset]
