"""yart_hip_scene_update on the device (include/yart_hip.h; csrc/scene_update_kernels.inc): a scene that was handed new node and
light transforms holds, and renders, the bits of a scene freshly created from the same description.

The cases are tests/test_scene_update_host.py's (build_case): frames of 48 x 32 at 4 spp with the scenes' own bounce counts.
  identity   the two-cube cornell (under 16 nodes, the LDS form), every node at the identity; one cube translated and rotated —
             the TRAV_IDENTITY kernel variants are left, and taken again on the way back
  instances  scenes.instances(70, 4): 64 nodes and more (kNodesTlas); a group node and three leaf instances moved, one instance
             scaled non-uniformly
  deep12     scenes.deep_instances(12): a level-3 and a level-10 node moved; nodes at and beyond kMaxNodeDepth have unbounded boxes
  deep80     scenes.deep_instances(80): more levels than kSceneUpdateMaxLevels, re-derived on the host
  light      cornell: the node that carries the light, and the light's record, translated and scaled by 1.5"""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_scene_update_host import CASES, build_case

FLAGS = {"default": 0, "general": 4, "megakernel": 1}        # YART_FLAG_GENERAL_TRACE, YART_FLAG_MEGAKERNEL


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype.itemsize == 4 else np.ascontiguousarray(a).view(np.uint8)


def render_all(scene, p, flags=0):
    frame, bufs, _ = scene.render_aovs(p, flags=flags)
    return dict(bufs, frame=frame)


def same_render(a, b, tag):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(bits(a[name]), bits(b[name])), f"{tag}: {name} differs"


def raw(arr):
    return np.ascontiguousarray(arr).view(np.uint8).reshape(len(arr), arr.dtype.itemsize)


def tlas_height(tlas):
    level = np.zeros(len(tlas), np.int64)
    for k in range(len(tlas)):                                # children are allocated after their parent
        if not tlas["b"][k]:
            level[tlas["a"][k]] = level[tlas["a"][k] + 1] = level[k] + 1
    return int(level.max()) if len(tlas) else 0


def refit_reference(tlas, world):
    """every box as the min / max over its leaves' nodeWorld boxes, in NumPy"""
    lo, hi = np.zeros((len(tlas), 3), np.float32), np.zeros((len(tlas), 3), np.float32)
    for k in range(len(tlas) - 1, -1, -1):
        a = int(tlas["a"][k])
        if tlas["b"][k]:
            lo[k], hi[k] = world["lo"][a], world["hi"][a]
        else:
            lo[k], hi[k] = np.minimum(lo[a], lo[a + 1]), np.maximum(hi[a], hi[a + 1])
    return lo, hi


@pytest.mark.gpu
@pytest.mark.parametrize("rebuild_top", [False, True], ids=["refit", "rebuild"])
@pytest.mark.parametrize("name", CASES)
def test_updated_scene_equals_a_fresh_one(gpu_api, name, rebuild_top):
    api = gpu_api
    s0, s1, p, moved, pass_lights = build_case(name)
    lights = (lambda s: s.lights) if pass_lights else (lambda s: None)
    A = api.DeviceScene(s0, device=0)
    r0 = render_all(A, p)
    _, _, tlas_before = A.scene_graph()
    A.update(s1.nodes, lights(s1), rebuild_top=rebuild_top)
    stats = A.last_update
    B = api.DeviceScene(s1, device=0)
    (na, wa, ta), (nb, wb, tb) = A.scene_graph(), B.scene_graph()
    print(f"{name}: {len(na)} nodes, depth {int(na['depth'].max())}, tlas {len(ta)} nodes of height {tlas_height(ta)}, update {stats}")
    assert np.array_equal(raw(na), raw(nb)), "NodeDev records"
    assert np.array_equal(raw(wa), raw(wb)), "nodeWorld"
    assert len(ta) == len(tb) and (len(ta) > 0) == (len(na) >= 64)
    if rebuild_top:
        assert np.array_equal(raw(ta), raw(tb)), "rebuilt top-level hierarchy"
    else:
        assert np.array_equal(ta["a"], tlas_before["a"]) and np.array_equal(ta["b"], tlas_before["b"]), "a refit keeps the tree"
        lo, hi = refit_reference(ta, wa)
        assert (ta["lo"] == lo).all() and (ta["hi"] == hi).all(), "refitted boxes"
    # launches: a level per launch on the device path, none per level on the host path
    depth, height = int(na["depth"].max()), tlas_height(ta)
    if name == "deep80":
        assert depth + 1 == 80 and stats["launches"] <= height + 1 < depth, stats        # the top-level refit alone
    else:
        assert 2 <= stats["launches"] <= (depth + 1) + (height + 1) + 4, stats
        if len(ta) and not rebuild_top:
            assert stats["launches"] >= height + 1 + 2
    r1 = None
    for tag, flags in FLAGS.items():
        ra, rb = render_all(A, p, flags), render_all(B, p, flags)
        same_render(ra, rb, f"{name} {tag}")
        r1 = r1 or ra
    B.close()
    # the case proves something: the frame changed, and a moved node is seen
    assert (bits(r1["frame"]) != bits(r0["frame"])).any(), "the move does not change the frame"
    seen = np.isin(r1["ids"][..., 0], moved)
    print(f"{name}: moved nodes {moved[:8]}{'...' if len(moved) > 8 else ''} seen in {int(seen.sum())} pixels")
    assert seen.any(), "no pixel shows a moved node"
    # the round trip
    A.update(s0.nodes, lights(s0), rebuild_top=rebuild_top)
    same_render(render_all(A, p), r0, f"{name} round trip")
    A.close()


@pytest.mark.gpu
def test_launch_counts(gpu_api):
    """YartSceneUpdateStats.launches: on the device path at most (scene depth + 1) + (tlas height + 1) + 4, and what the launches
    are — one scatter, one fold per level that has parents, one for the world boxes, one per level of the top-level tree; for the
    80-level graph the bounds did not run per level: only the top-level refit launches, none at all with a rebuilt top."""
    api = gpu_api
    for name, fold_levels in (("identity", 1), ("instances", 2), ("deep12", 11)):
        s0, s1, _, _, _ = build_case(name)
        A = api.DeviceScene(s0, device=0)
        nodes, _, tlas = A.scene_graph()
        depth, height = int(nodes["depth"].max()), tlas_height(tlas)
        A.update(s1.nodes)
        refit = A.last_update["launches"]
        A.update(s1.nodes, rebuild_top=True)
        rebuilt = A.last_update["launches"]
        A.close()
        print(f"{name}: depth {depth}, tlas height {height}: {refit} launches with a refit, {rebuilt} with a rebuild")
        assert rebuilt == 2 + fold_levels and refit == rebuilt + (height + 1 if len(tlas) else 0)
        assert refit <= (depth + 1) + (height + 1) + 4
    s0, s1, _, _, _ = build_case("deep80")
    A = api.DeviceScene(s0, device=0)
    nodes, _, tlas = A.scene_graph()
    assert int(nodes["depth"].max()) == 79 and len(tlas)
    A.update(s1.nodes, s1.lights)
    assert A.last_update["launches"] == tlas_height(tlas) + 1
    A.update(s1.nodes, s1.lights, rebuild_top=True)
    assert A.last_update["launches"] == 0
    A.close()


@pytest.mark.gpu
def test_motion_of_a_scene_animated_in_place(gpu_api):
    """One yscn.Scene whose Node objects are moved in place between update(motion=True) calls — the natural way to animate: the
    records are node_motion over explicit copies of the previous and the current node lists, on bits, and mark the moved node and
    its subtree. (The scene object must remember what the nodes WERE, not the caller's mutable Node objects.)"""
    import copy
    from yart_amd.temporal import node_motion
    from yart_amd.yscn import trs
    api = gpu_api
    s, _, _, _, _ = build_case("instances")
    group = next(i for i, n in enumerate(s.nodes) if n.mesh < 0 and n.parent == 0)
    subtree = [group] + [i for i, n in enumerate(s.nodes) if n.parent == group]
    A = api.DeviceScene(s, device=0)
    for step in range(1, 3):
        before = copy.deepcopy(s.nodes)
        m = trs((0.25 * step, 0.1, -0.2 * step), (0, 1, 0), 0.2 * step)[0].astype(np.float64)
        f = (m @ np.asarray(s.nodes[group].fwd, np.float64)).astype(np.float32)
        s.nodes[group].fwd, s.nodes[group].inv = f, np.linalg.inv(f.astype(np.float64)).astype(np.float32)
        if step == 2:                                           # ... and a word of the same array object changed in place
            s.nodes[subtree[1]].fwd[0, 3] += np.float32(0.5)
            s.nodes[subtree[1]].inv = np.linalg.inv(s.nodes[subtree[1]].fwd.astype(np.float64)).astype(np.float32)
        got = A.update(s.nodes, motion=True)
        want = node_motion(before, copy.deepcopy(s.nodes))
        kind = got.view(np.uint32)[:, 15]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"step {step}"
        assert sorted(np.flatnonzero(kind).tolist()) == sorted(subtree), f"step {step}"
    A.close()


def child_sequence():
    """test_temporal_motion.child_render_denoised's three frames, once with the scene re-created per frame and once with one scene
    updated per frame (update(..., motion=True)): accumulated frame, variance and length on bits."""
    from yart_amd import api
    from yart_amd.temporal import node_motion
    from tests.test_temporal_motion import RENDER_FRAMES, RENDER_SIZE, render_scene
    w, h = RENDER_SIZE
    acc_a, acc_b = api.TemporalAccumulator(w, h, device=0), api.TemporalAccumulator(w, h, device=0)
    updated, prev = None, None
    for k in range(RENDER_FRAMES):
        s, p = render_scene(k)
        fresh = api.DeviceScene(s, device=0)
        motion_b = None if prev is None else node_motion(prev, s.nodes)
        _, clean_b, gb = fresh.render_denoised(p, temporal=acc_b, motion=motion_b)
        fresh.close()
        if updated is None:
            updated, motion_a = api.DeviceScene(s, device=0), None
        else:
            motion_a = updated.update(s.nodes, s.lights, motion=True)
            assert np.array_equal(motion_a.view(np.uint32), motion_b.view(np.uint32))
        _, clean_a, ga = updated.render_denoised(p, temporal=acc_a, motion=motion_a)
        for name in ("accumulated", "accumulated_variance", "length"):
            a, b = ga[name].cpu().numpy(), gb[name].cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"frame {k}: {name}"
        assert np.array_equal(clean_a.cpu().numpy().view(np.uint32), clean_b.cpu().numpy().view(np.uint32)), f"frame {k}: denoised"
        prev = s.nodes
    assert int(ga["length"].cpu().numpy().view(np.uint32).max()) == RENDER_FRAMES
    updated.close()
    acc_a.close()
    acc_b.close()


@pytest.mark.gpu
def test_sequence_with_updates_equals_the_recreating_run(gpu_api):
    code = "import torch\ntorch.cuda.set_device(0)\nfrom tests import test_scene_update as t\nt.child_sequence()\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_refused_updates_leave_the_scene_alone(gpu_api):
    """Every YART_E_INVALID condition that needs a scene: scene_graph() is byte-identical afterwards, and a render gives the frame
    from before."""
    import copy
    api = gpu_api
    L = api.lib()
    s0, s1, p, _, _ = build_case("light")
    A = api.DeviceScene(s0, device=0)
    before = A.scene_graph()
    frame0 = render_all(A, p)

    def refused(nodes, lights, word, **kw):
        with pytest.raises(api.YartError, match=word) as e:
            A.update(nodes, lights, **kw)
        assert e.value.code == api.YART_E_INVALID
        for x, y in zip(A.scene_graph(), before):
            assert np.array_equal(raw(x), raw(y)), word

    def nodes_with(i, **kw):
        n = copy.deepcopy(s1.nodes)
        for k, v in kw.items():
            setattr(n[i], k, v)
        return n

    def lights_with(i, **kw):
        l = copy.deepcopy(s1.lights)
        for k, v in kw.items():
            setattr(l[i], k, v)
        return l
    refused(s1.nodes[:-1], None, "n_nodes")
    refused(s1.nodes + [s1.nodes[-1]], None, "n_nodes")
    refused(nodes_with(1, mesh=-1), None, "parent / mesh")
    refused(nodes_with(1, parent=-1), None, "parent / mesh")
    refused(s1.nodes, s1.lights[:-1], "n_lights")
    refused(s1.nodes, lights_with(0, tri=s1.lights[0].tri + 1), "light 0")
    refused(s1.nodes, lights_with(1, emission=(1.0, 2.0, 3.0)), "light 1")
    refused(s1.nodes, lights_with(0, two_sided=True), "light 0")
    refused(s1.nodes, lights_with(0, radius=5.0), "light 0")
    for bad in (np.nan, np.inf, -np.inf):
        for field, word in (("fwd", 3), ("inv", 15)):
            m = s1.nodes[1].fwd.copy() if field == "fwd" else s1.nodes[1].inv.copy()
            m.reshape(-1)[word] = bad
            refused(nodes_with(1, **{field: m}), None, "node 1.*finite")
            m = np.array(s1.lights[0].fwd if field == "fwd" else s1.lights[0].inv, np.float32).copy()
            m.reshape(-1)[word] = bad
            refused(s1.nodes, lights_with(0, **{field: m}), "light 0.*finite")
    # through the C ABI: unknown flags and a small struct with a live scene
    nd = (api.NodeDesc * len(s1.nodes))()
    for i, n in enumerate(s1.nodes):
        nd[i] = api.NodeDesc(n.parent, n.mesh, api._f(n.fwd, 16), api._f(n.inv, 16))
    for up in (api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), len(s1.nodes), nd, 0, None, 6), api.SceneUpdate(16, len(s1.nodes), nd, 0, None, 0)):
        assert L.yart_hip_scene_update(A.handle, ctypes.byref(up), None, None) == api.YART_E_INVALID
    for x, y in zip(A.scene_graph(), before):
        assert np.array_equal(raw(x), raw(y))
    same_render(render_all(A, p), frame0, "after the refused updates")
    A.close()
    # a mesh whose vertex box is not finite (an unused vertex at +inf): the scene is created, and cannot be updated
    s2 = copy.deepcopy(s0)
    m = s2.meshes[0]
    m.positions = np.concatenate([m.positions, np.array([[np.inf, 0.0, 0.0]], np.float32)])
    m.normals = np.concatenate([m.normals, m.normals[-1:]])
    m.tangents = np.concatenate([m.tangents, m.tangents[-1:]])
    m.uvs = np.concatenate([m.uvs, m.uvs[-1:]])
    C2 = api.DeviceScene(s2, device=0)
    g = C2.scene_graph()
    with pytest.raises(api.YartError, match="vertex box is not finite"):
        C2.update(s2.nodes)
    for x, y in zip(C2.scene_graph(), g):
        assert np.array_equal(raw(x), raw(y))
    C2.close()
