"""The top-level hierarchy built on the device (csrc/tlas_build_kernels.inc; YART_UPDATE_REBUILD_TOP_DEVICE of include/yart_hip.h)
against the project's own host_scene.hpp::buildTopLevel — through yart_hip_tlas_build_host and through scene creation —, byte for
byte: the aimed inputs of tests/tlassuite.py through the stand-alone entries, and scenes through update / update_meshes.

LAUNCHES. The device build of a tree over L mesh nodes takes, with cap = kTlasLocalLeaves, P = the power of two >= max(L, cap):
  per top level (a level on which a range holds more than cap leaves)   2 + sum over the merge stages 2 cap, 4 cap, .. P of
                                                                        (log2(stage / cap) global steps + 1 local merge)
  + 1 for all subtrees + (height + 1) for the records, one per level of the tree
(`launch_formula` below; yart_hip_tlas_build_launches is the library's statement of it). An update with the device rebuild launches
exactly the chain's launches (what YART_UPDATE_REBUILD_TOP counts: scatter, folds, world boxes) plus that."""
import copy
import ctypes

import numpy as np
import pytest

from tests import tlassuite
from tests.test_scene_update import bits, raw, refit_reference, render_all, same_render, tlas_height
from tests.test_scene_update_host import build_case

SIZE, SPP = (48, 32), 4


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def launch_formula(leaves, cap):
    def largest(n, depth):
        for _ in range(depth):
            n -= n // 2
        return n
    if not leaves:
        return 0
    top = next(d for d in range(32) if largest(leaves, d) <= cap)
    height = next(d for d in range(32) if largest(leaves, d) <= 1)
    padded = cap
    while padded < leaves:
        padded *= 2
    per_level, stage, steps = 2, 2 * cap, 1
    while stage <= padded:
        per_level += steps + 1
        stage, steps = 2 * stage, steps + 1
    return top * per_level + 1 + height + 1


def same_graph(A, B, tag):
    (na, wa, ta), (nb, wb, tb) = A.scene_graph(), B.scene_graph()
    assert np.array_equal(raw(na), raw(nb)), f"{tag}: NodeDev records"
    assert np.array_equal(raw(wa), raw(wb)), f"{tag}: nodeWorld"
    assert len(ta) == len(tb) and np.array_equal(raw(ta), raw(tb)), f"{tag}: top-level hierarchy"
    return na, wa, ta


def permute_instances(s0, seed=3):
    """a copy of an instances scene with the instances' transforms (mesh nodes below a group) permuted among themselves"""
    s1 = copy.deepcopy(s0)
    inst = [i for i, n in enumerate(s0.nodes) if n.mesh >= 0 and n.parent > 0]
    perm = np.random.default_rng(seed).permutation(len(inst))
    assert len(inst) >= 64 and (perm != np.arange(len(inst))).any()
    for i, j in zip(inst, perm):
        s1.nodes[i].fwd, s1.nodes[i].inv = s0.nodes[inst[j]].fwd.copy(), s0.nodes[inst[j]].inv.copy()
    return s1


def moved_large_instances(n_instances):
    """scenes.instances of n_instances, and the same scene after tests/test_scene_update_host.py::build_case's moves of its
    "instances" case — a group node, three instances translated or rotated, one scaled in its own space — plus a permutation of the
    instances' transforms"""
    from yart_amd import scenes
    from yart_amd.yscn import trs
    from tests.test_scene_update_host import _compose
    s0, p = scenes.instances(SIZE[0], SIZE[1], SPP, 4, n_instances=n_instances, groups=4, child_extent=3.0, scale=(0.05, 0.15))
    s1 = permute_instances(s0)
    group = next(i for i, n in enumerate(s0.nodes) if n.mesh < 0 and n.parent == 0)
    leaves = [i for i, n in enumerate(s0.nodes) if n.mesh >= 0 and n.parent > 0 and n.parent != group]
    picked = [leaves[3], leaves[20], leaves[40], leaves[30]]
    moves = {group: trs((0.6, 0.4, -0.3), (0, 1, 0), 0.3)[0], picked[0]: trs((0.0, 1.0, 0.5))[0], picked[1]: trs((-0.7, 0.2, 0.0))[0],
             picked[2]: trs((0.3, -0.2, 0.8), (1, 0, 0), 0.5)[0]}
    for k, m in moves.items():
        s1.nodes[k].fwd, s1.nodes[k].inv = _compose(m, s1.nodes[k].fwd)
    f = (np.asarray(s1.nodes[picked[3]].fwd, np.float64) @ trs(scale=(1.7, 0.6, 1.2))[0].astype(np.float64)).astype(np.float32)
    s1.nodes[picked[3]].fwd, s1.nodes[picked[3]].inv = f, np.linalg.inv(f.astype(np.float64)).astype(np.float32)
    return s0, s1, p


@pytest.mark.gpu
def test_suite_parity(gpu_api):
    """Every case of the suite: the device entry == the host entry in record count, height and bytes."""
    api = gpu_api
    cases = tlassuite.suite(api.TLAS_LOCAL_LEAVES)
    tlassuite.check_signed_zero_rule(cases)
    assert all(n >= 8 for n in tlassuite.counts(cases).values())
    bad = []
    for kind, leaves, mesh, world in cases:
        want, hw = api.tlas_build(world, mesh, device=None)
        got, hg = api.tlas_build(world, mesh, device=0)
        assert len(want) == 2 * leaves - 1
        if not (len(got) == len(want) and hg == hw and np.array_equal(raw(got), raw(want))):
            bad.append((kind, leaves, len(got), hg, int((raw(got) != raw(want)).any(1).sum()) if len(got) == len(want) else -1))
    assert not bad, bad
    # below 64 nodes and without mesh nodes: no records from either
    kind, leaves, mesh, world = cases[0]
    assert len(api.tlas_build(world[:63], mesh[:63], device=0)[0]) == 0
    assert len(api.tlas_build(world, np.full(len(mesh), -1, np.int32), device=0)[0]) == 0
    L = api.lib()
    for leaves in tlassuite.leaf_counts(api.TLAS_LOCAL_LEAVES) + [0, 65542, (1 << 20) - 1]:
        assert L.yart_hip_tlas_build_launches(leaves) == launch_formula(leaves, api.TLAS_LOCAL_LEAVES), leaves


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["instances70", "instances_large", "deep80"])
def test_device_rebuild_equals_a_fresh_scene(gpu_api, name):
    """update(rebuild_top="device") leaves scene_graph() — nodes, node_world, tlas — and the frame of a freshly created scene of the
    moved description; then a refit (flags 0) of the new tree equals the NumPy refit, and a host rebuild of the same state leaves
    the device rebuild's bytes."""
    api = gpu_api
    cap = api.TLAS_LOCAL_LEAVES
    if name == "instances70":
        s0, s1, p, _, pass_lights = build_case("instances")
        assert len(s0.nodes) == 76
    elif name == "instances_large":
        s0, s1, p = moved_large_instances(2 * cap + 100)
        pass_lights = False
    else:
        s0, s1, p, _, pass_lights = build_case("deep80")
    lights = s1.lights if pass_lights else None
    A = api.DeviceScene(s0, device=0)
    r0 = render_all(A, p)
    _, _, t0 = A.scene_graph()
    leaves = sum(1 for n in s0.nodes if n.mesh >= 0)
    assert len(t0) == 2 * leaves - 1
    if name == "instances_large":
        assert leaves > 2 * cap and launch_formula(leaves, cap) > tlas_height(t0) + 2        # it has top levels and several subtrees
    A.update(s1.nodes, lights, rebuild_top="device")
    device_launches = A.last_update["launches"]
    B = api.DeviceScene(s1, device=0)
    _, wa, ta = same_graph(A, B, f"{name} device rebuild")
    assert (raw(ta) != raw(t0)).any(), "the moves do not change the tree"
    if name == "instances_large":
        assert (ta["a"][ta["b"] == 1] != t0["a"][t0["b"] == 1]).any(), "no leaf changed its place"
    ra, rb = render_all(A, p), render_all(B, p)
    same_render(ra, rb, f"{name} device rebuild")
    assert (bits(ra["frame"]) != bits(r0["frame"])).any()
    # a host rebuild of the same state: the same bytes, and the chain's launches alone
    A.update(s1.nodes, lights, rebuild_top="host")
    chain_launches = A.last_update["launches"]
    same_graph(A, B, f"{name} host rebuild after the device's")
    assert device_launches == chain_launches + launch_formula(leaves, cap)
    # the way back on the device, then a refit with flags 0 to the moved state: the tree of s0, the boxes of s1
    A.update(s0.nodes, s0.lights if pass_lights else None, rebuild_top="device")
    _, _, tback = A.scene_graph()
    assert np.array_equal(raw(tback), raw(t0)), "the way back"
    same_render(render_all(A, p), r0, f"{name} round trip")
    A.update(s1.nodes, lights)
    _, wr, tr = A.scene_graph()
    assert np.array_equal(raw(wr), raw(wa))
    assert np.array_equal(tr["a"], t0["a"]) and np.array_equal(tr["b"], t0["b"]), "a refit keeps the tree"
    lo, hi = refit_reference(tr, wr)
    assert (tr["lo"] == lo).all() and (tr["hi"] == hi).all(), "refitted boxes after a device rebuild"
    same_render(render_all(A, p), rb, f"{name} refit after a device rebuild")
    A.close()
    B.close()


@pytest.mark.gpu
def test_mesh_update_with_a_device_rebuild(gpu_api):
    """update_meshes(rebuild_top="device") on the 76-node instances scene whose tree is stale — the instances' transforms were
    permuted and the tree only refitted —: records and tree of the fresh scene, the same frame; leaves changed places, which a
    refit cannot do."""
    from tests.test_mesh_update_host import build_case as mesh_case, update_arrays
    api = gpu_api
    states, p, meshes = mesh_case("instances")
    assert len(states[0].nodes) >= 64
    moved = permute_instances(states[1])
    A = api.DeviceScene(states[0], device=0)
    A.update(moved.nodes)
    _, _, t_refit = A.scene_graph()
    A.update_meshes(update_arrays(states[1], meshes, True), rebuild_top="device")
    B = api.DeviceScene(moved, device=0)
    _, _, ta = same_graph(A, B, "mesh update")
    leaf = ta["b"] == 1
    assert len(ta) and np.array_equal(ta["b"], t_refit["b"]) and (ta["a"][leaf] != t_refit["a"][leaf]).any(), "no leaf changed its place"
    same_render(render_all(A, p), render_all(B, p), "mesh update")
    A.close()
    B.close()


@pytest.mark.gpu
def test_scene_without_a_tree_and_the_refused_flag_pair(gpu_api):
    """cornell (fewer than 64 nodes): the flag is accepted and scene_graph() is unchanged by an update with the scene's own nodes.
    Flags 3 through the C ABI on a live scene with a tree: YART_E_INVALID, "flags" in the message, graph and frame unchanged."""
    from yart_amd import scenes
    api = gpu_api
    s, p = scenes.cornell(SIZE[0], SIZE[1], SPP, 4)
    A = api.DeviceScene(s, device=0)
    before = A.scene_graph()
    assert len(before[2]) == 0 and len(s.nodes) < 64
    A.update(s.nodes, rebuild_top="device")
    flags0 = A.last_update["launches"]
    after = A.scene_graph()
    assert all(np.array_equal(raw(a), raw(b)) for a, b in zip(before, after))
    A.update(s.nodes)
    assert A.last_update["launches"] == flags0
    with pytest.raises(api.YartError):
        A.update(s.nodes, rebuild_top="gpu")
    A.close()

    s0, s1, p, _, _ = build_case("instances")
    A = api.DeviceScene(s0, device=0)
    graph, frame = A.scene_graph(), render_all(A, p)
    nd = (api.NodeDesc * len(s1.nodes))()
    for i, n in enumerate(s1.nodes):
        nd[i] = api.NodeDesc(n.parent, n.mesh, api._f(n.fwd, 16), api._f(n.inv, 16))
    L = api.lib()
    up = api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), len(s1.nodes), nd, 0, None, 3)
    assert L.yart_hip_scene_update(A.handle, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"flags" in L.yart_hip_last_error()
    assert all(np.array_equal(raw(a), raw(b)) for a, b in zip(graph, A.scene_graph()))
    same_render(render_all(A, p), frame, "refused flags")
    A.close()


@pytest.mark.gpu
def test_launch_counts_of_the_device_rebuild(gpu_api):
    """last_update["launches"] under the device rebuild: more than the chain alone (flags 0 minus the refit's height + 1 launches),
    and exactly the chain plus launch_formula(leaves) — the bound of the module docstring — for a tree of one subtree."""
    api = gpu_api
    s0, s1, _, _, _ = build_case("instances")
    A = api.DeviceScene(s0, device=0)
    _, _, tlas = A.scene_graph()
    height, leaves = tlas_height(tlas), (len(tlas) + 1) // 2
    A.update(s1.nodes)
    chain = A.last_update["launches"] - (height + 1)
    A.update(s1.nodes, rebuild_top="device")
    device = A.last_update["launches"]
    A.close()
    print(f"{leaves} leaves, height {height}: chain {chain}, device rebuild {device}")
    assert launch_formula(leaves, api.TLAS_LOCAL_LEAVES) == 1 + height + 1
    assert chain < device <= chain + launch_formula(leaves, api.TLAS_LOCAL_LEAVES)
