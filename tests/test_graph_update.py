"""yart_hip_scene_update_graph on the device (include/yart_hip.h; csrc/graph_update_kernels.inc): a scene that was handed a new node
list — nodes added, removed, hidden, re-meshed, re-parented — holds, and renders in every pipeline, the bits of a scene freshly
created from the same description with that list.

The cases are tests/test_graph_update_host.py's (graph_case): frames of 48 x 32 at 4 spp. Behind them, each with its own test: the
hand-over of the device builder of the top-level hierarchy (2047 -> 2049 and 2049 -> 4099 mesh nodes around kTlasLocalLeaves = 2048),
one handle whose list grows, shrinks and grows again, the combination with update (transforms) and update_meshes (a height field), the
kept previous frame, and every refusal.

One refusal of the header cannot be produced: a top-level hierarchy higher than the 192 entries of the traversal stack. Its height is
ceil(log2(mesh nodes)), and a list has fewer than 2^20 nodes: at most 20."""
import copy
import ctypes

import numpy as np
import pytest

from tests.test_graph_update_host import CASES, graph_case, instances, two_cubes, with_nodes
from tests.test_scene_update import FLAGS, bits, raw, render_all, same_render, tlas_height

REBUILD = ["device", "host"]


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def same_graph(a, b, tag):
    for what, x, y in zip(("NodeDev records", "nodeWorld", "top-level hierarchy"), a, b):
        assert len(x) == len(y), f"{tag}: {what}: {len(x)} and {len(y)} records"
        assert np.array_equal(raw(x), raw(y)), f"{tag}: {what}"


def expected_tlas_records(nodes):
    leaves = sum(n.mesh >= 0 for n in nodes)
    return 2 * leaves - 1 if len(nodes) >= 64 and leaves else 0


def instances_with_mesh_nodes(mesh_nodes):
    """scenes.instances whose mesh nodes — the room and the instances — number `mesh_nodes`"""
    s, p = instances(mesh_nodes - 1 + 2 + 4, 4)
    assert sum(n.mesh >= 0 for n in s.nodes) == mesh_nodes
    return s, p


@pytest.mark.gpu
@pytest.mark.parametrize("rebuild_top", REBUILD)
@pytest.mark.parametrize("name", CASES)
def test_updated_graph_equals_a_fresh_one(gpu_api, name, rebuild_top):
    api = gpu_api
    s0, s1, p, shown, gone = graph_case(name)
    A = api.DeviceScene(s0, device=0)
    r0, g0 = render_all(A, p), A.scene_graph()
    A.update_graph(s1.nodes, rebuild_top=rebuild_top)
    stats = A.last_update
    B = api.DeviceScene(s1, device=0)
    ga, gb = A.scene_graph(), B.scene_graph()
    print(f"{name}: {len(g0[0])} -> {len(ga[0])} nodes, depth {int(ga[0]['depth'].max())}, tlas {len(g0[2])} -> {len(ga[2])} records of height "
          f"{tlas_height(ga[2])}, update {stats}")
    assert len(ga[0]) == len(s1.nodes) and len(ga[2]) == expected_tlas_records(s1.nodes)
    same_graph(ga, gb, name)
    # launches: the topology kernel and the chain on the device path; on the host path (more than 64 levels) the device build alone
    depth, height = int(ga[0]["depth"].max()), tlas_height(ga[2])
    build = (height + 2 if len(ga[2]) else 0) if rebuild_top == "device" else 0
    if name == "deep80":
        assert depth + 1 == 81 and stats["launches"] == build, stats
    else:
        assert 3 + build <= stats["launches"] <= 3 + (depth + 1) + build, stats
    r1 = None
    for tag, flags in FLAGS.items():
        ra, rb = render_all(A, p, flags), render_all(B, p, flags)
        same_render(ra, rb, f"{name} {tag}")
        r1 = r1 or ra
    B.close()
    # the case proves something: the frame changed, a new or changed node is seen, a node that lost its mesh was seen and is not any more
    assert (bits(r1["frame"]) != bits(r0["frame"])).any(), "the change does not change the frame"
    if shown:
        seen = np.isin(r1["ids"][..., 0], shown)
        print(f"{name}: nodes {shown[:8]}{'...' if len(shown) > 8 else ''} seen in {int(seen.sum())} pixels")
        assert seen.any(), "no pixel shows a new or changed node"
    if gone:
        assert np.isin(r0["ids"][..., 0], gone).any(), "no pixel showed a node the change takes away"
        if name != "remove":                               # (a removed node's index belongs to no node, or to another)
            assert not np.isin(r1["ids"][..., 0], gone).any(), "a hidden node is still seen"
    if name == "hide-all":
        assert (r1["ids"][..., 0] < 0).all()
    # the round trip
    A.update_graph(s0.nodes, rebuild_top=rebuild_top)
    same_graph(A.scene_graph(), g0, f"{name} round trip")
    same_render(render_all(A, p), r0, f"{name} round trip")
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rebuild_top", REBUILD)
@pytest.mark.parametrize("before,after", [(2047, 2049), (2049, 4099)])
def test_hand_over_of_the_device_builder(gpu_api, before, after, rebuild_top):
    """Mesh-node counts on both sides of kTlasLocalLeaves = 2048, and of twice that: the build goes from one workgroup's subtree to a
    sorted top level and subtrees, and to two top levels. Scene-graph bytes, and one render."""
    api = gpu_api
    assert api.TLAS_LOCAL_LEAVES == 2048
    (s0, p), (s1, _) = instances_with_mesh_nodes(before), instances_with_mesh_nodes(after)
    s1 = with_nodes(s0, s1.nodes)
    A = api.DeviceScene(s0, device=0)
    A.update_graph(s1.nodes, rebuild_top=rebuild_top)
    print(f"{before} -> {after} mesh nodes ({rebuild_top}): {A.last_update}")
    B = api.DeviceScene(s1, device=0)
    ga, gb = A.scene_graph(), B.scene_graph()
    assert len(ga[2]) == 2 * after - 1
    same_graph(ga, gb, f"{before} -> {after}")
    same_render(render_all(A, p), render_all(B, p), f"{before} -> {after}")
    A.close()
    B.close()


@pytest.mark.gpu
def test_one_handle_grows_shrinks_and_grows_again(gpu_api):
    """70 -> 300 -> 20 -> 500 -> 70 nodes on one handle: the arrays grow and are reused; after every step the scene graph and a frame
    are a fresh scene's."""
    api = gpu_api
    s0, p = instances(70, 4)
    A = api.DeviceScene(s0, device=0)
    for k, n in enumerate((300, 20, 500, 70)):
        s1 = with_nodes(s0, instances(n, 4)[0].nodes)
        A.update_graph(s1.nodes, rebuild_top=REBUILD[k % 2])
        B = api.DeviceScene(s1, device=0)
        same_graph(A.scene_graph(), B.scene_graph(), f"step {k}: {n} nodes")
        same_render(render_all(A, p), render_all(B, p), f"step {k}: {n} nodes")
        B.close()
    A.close()


@pytest.mark.gpu
def test_combines_with_update_and_update_meshes(gpu_api):
    """The height field of tests/test_mesh_update_host.py (wave24) plus a cube mesh: update_meshes, then update_graph (a cube node
    added), then update (the cube moved) == a fresh scene of that description; then the list back, the vertices back."""
    from tests.test_mesh_update_host import update_arrays, wave_scene, with_positions
    from yart_amd import scenes
    from yart_amd.yscn import Material, Node, trs
    api = gpu_api

    def scene(t):
        s, p = wave_scene(24, t)
        b = scenes.MeshBuilder()
        b.box((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8), s.add_material(Material(base=(0.2, 0.7, 0.3), roughness=0.6)))
        return s, p, s.add_mesh(b.build())
    (s0, p, cube), (s_t1, _, _) = scene(0.0), scene(0.35)
    wave = next(n.mesh for n in s0.nodes if n.mesh >= 0 and len(s0.meshes[n.mesh].positions) == len(s_t1.meshes[n.mesh].positions) > 100)
    added = copy.deepcopy(s0.nodes) + [Node(parent=0, mesh=cube, fwd=trs((0.0, 3.0, 0.0))[0], inv=trs((0.0, 3.0, 0.0))[1])]
    moved = copy.deepcopy(added)
    moved[-1].fwd, moved[-1].inv = trs((1.0, 4.0, -0.5), (0, 1, 1), 0.6, (1.5, 0.7, 1.0))
    A = api.DeviceScene(s0, device=0)
    r0, g0 = render_all(A, p), A.scene_graph()
    A.update_meshes(update_arrays(s_t1, [wave]))
    A.update_graph(added)
    A.update(moved)
    final = with_nodes(with_positions(s0, wave, s_t1.meshes[wave].positions), moved)
    final.meshes[wave].normals, final.meshes[wave].tangents = s_t1.meshes[wave].normals, s_t1.meshes[wave].tangents
    B = api.DeviceScene(final, device=0)
    same_graph(A.scene_graph(), B.scene_graph(), "meshes, graph, transforms")
    for tag, flags in FLAGS.items():
        ra = render_all(A, p, flags)
        same_render(ra, render_all(B, p, flags), f"combined {tag}")
    assert (ra["ids"][..., 0] == len(moved) - 1).any(), "the added cube is not seen"
    B.close()
    # ... and in the other order on the way back: the list first, then the vertices
    A.update_graph(s0.nodes, rebuild_top="host")
    A.update_meshes(update_arrays(s0, [wave]))
    same_graph(A.scene_graph(), g0, "back")
    same_render(render_all(A, p), r0, "back")
    A.close()


@pytest.mark.gpu
def test_a_graph_update_discards_the_kept_previous_frame(gpu_api):
    """keep_previous, update_graph, pixel_motion: the answer of a scene that never kept a frame — YART_E_INVALID with that message —,
    until the next keep_previous."""
    api = gpu_api
    s0, s1, p, _, _ = graph_case("add")
    never = api.DeviceScene(s0, device=0)
    aovs = render_all(never, p)
    with pytest.raises(api.YartError) as e0:
        never.pixel_motion(aovs)
    never.close()
    assert e0.value.code == api.YART_E_INVALID and "keep_previous was never called" in str(e0.value)
    A = api.DeviceScene(s0, device=0)
    A.keep_previous()
    assert A.pixel_motion(render_all(A, p)).shape == (p["size"][1], p["size"][0], 8)
    A.update_graph(s1.nodes)
    aovs = render_all(A, p)
    with pytest.raises(api.YartError) as e1:
        A.pixel_motion(aovs)
    assert e1.value.code == api.YART_E_INVALID and str(e1.value) == str(e0.value)
    A.keep_previous()
    rec = A.pixel_motion(aovs)
    assert not rec.view(np.uint32).any(), "nothing moved since the frame was kept: every record is static"
    A.close()


@pytest.mark.gpu
def test_refused_graph_updates_leave_the_scene_alone(gpu_api):
    """Every YART_E_INVALID condition that needs a scene (the others: tests/test_graph_update_host.py), and those of the list itself
    once more with a live handle: scene_graph() is byte-identical afterwards, and a render gives the frame from before."""
    api = gpu_api
    L = api.lib()
    s0, p, cube, small = two_cubes()
    A = api.DeviceScene(s0, device=0)
    before, frame0 = A.scene_graph(), render_all(A, p)

    def untouched(word):
        same_graph(A.scene_graph(), before, word)

    def refused(nodes, lights, word, **kw):
        with pytest.raises(api.YartError, match=word) as e:
            A.update_graph(nodes, lights, **kw)
        assert e.value.code == api.YART_E_INVALID
        untouched(word)

    def nodes_with(i, **kw):
        n = copy.deepcopy(s0.nodes)
        for k, v in kw.items():
            setattr(n[i], k, v)
        return n

    def lights_with(i, **kw):
        l = copy.deepcopy(s0.lights)
        for k, v in kw.items():
            setattr(l[i], k, v)
        return l
    last = len(s0.nodes) - 1
    refused([], None, "n_nodes is 0")
    refused(nodes_with(0, parent=0), None, "node 0")
    refused(nodes_with(last, parent=-1), None, f"node {last}.*parent")
    refused(nodes_with(last, parent=-2), None, f"node {last}.*parent")
    refused(nodes_with(last, parent=last), None, f"node {last}.*parent")
    refused(nodes_with(1, parent=2), None, "node 1.*parent")
    refused(nodes_with(last, mesh=len(s0.meshes)), None, f"node {last}: mesh index")
    refused(nodes_with(last, mesh=1 << 20), None, f"node {last}: mesh index")
    for bad in (np.nan, np.inf, -np.inf):
        for field, word in (("fwd", 3), ("inv", 15)):
            m = np.array(getattr(s0.nodes[last], field), np.float32).copy()
            m.reshape(-1)[word] = bad
            refused(nodes_with(last, **{field: m}), None, f"node {last}.*finite")
            m = np.array(getattr(s0.lights[0], field), np.float32).copy()
            m.reshape(-1)[word] = bad
            refused(s0.nodes, lights_with(0, **{field: m}), "light 0.*finite")
    refused(s0.nodes, s0.lights[:-1], "n_lights")
    refused(s0.nodes, s0.lights + [s0.lights[-1]], "n_lights")
    refused(s0.nodes, lights_with(0, tri=s0.lights[0].tri + 1), "light 0")
    refused(s0.nodes, lights_with(1, emission=(1.0, 2.0, 3.0)), "light 1")
    refused(s0.nodes, lights_with(0, two_sided=True), "light 0")
    # through the C ABI: both rebuild flags, unknown flags, a small struct, a node count of 2^20, a small stats struct
    nd = (api.NodeDesc * len(s0.nodes))()
    for i, n in enumerate(s0.nodes):
        nd[i] = api.NodeDesc(n.parent, n.mesh, api._f(n.fwd, 16), api._f(n.inv, 16))
    size, n = ctypes.sizeof(api.SceneGraphUpdate), len(s0.nodes)
    for up, word in ((api.SceneGraphUpdate(size, n, nd, 0, None, 3), b"exclude"), (api.SceneGraphUpdate(size, n, nd, 0, None, 4), b"unknown flags"),
                     (api.SceneGraphUpdate(16, n, nd, 0, None, 0), b"struct_size"), (api.SceneGraphUpdate(size, 1 << 20, nd, 0, None, 0), b"n_nodes"),
                     (api.SceneGraphUpdate(size, n, None, 0, None, 0), b"null"), (api.SceneGraphUpdate(size, n, nd, len(s0.lights), None, 0), b"lights pointer")):
        assert L.yart_hip_scene_update_graph(A.handle, ctypes.byref(up), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
    small_stats = api.SceneUpdateStats(4)
    up = api.SceneGraphUpdate(size, n, nd, 0, None, 0)
    assert L.yart_hip_scene_update_graph(A.handle, ctypes.byref(up), None, ctypes.byref(small_stats)) == api.YART_E_INVALID
    assert b"stats" in L.yart_hip_last_error()
    untouched("C ABI")
    same_render(render_all(A, p), frame0, "after the refused updates")
    # ... and the same list is taken: the scene was usable all along
    A.update_graph(s0.nodes)
    untouched("the scene's own list")
    same_render(render_all(A, p), frame0, "after the scene's own list")
    A.close()
    # a mesh whose vertex box is not finite (an unused vertex at +inf): the scene is created, and its list cannot be replaced
    s2 = copy.deepcopy(s0)
    m = s2.meshes[0]
    m.positions = np.concatenate([m.positions, np.array([[np.inf, 0.0, 0.0]], np.float32)])
    m.normals = np.concatenate([m.normals, m.normals[-1:]])
    m.tangents = np.concatenate([m.tangents, m.tangents[-1:]])
    m.uvs = np.concatenate([m.uvs, m.uvs[-1:]])
    C2 = api.DeviceScene(s2, device=0)
    g = C2.scene_graph()
    with pytest.raises(api.YartError, match="vertex box is not finite"):
        C2.update_graph(s2.nodes[:-1])
    same_graph(C2.scene_graph(), g, "vertex box")
    C2.close()
