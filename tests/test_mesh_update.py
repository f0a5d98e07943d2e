"""yart_hip_scene_update_meshes on the device (include/yart_hip.h; csrc/mesh_update_kernels.inc): a scene whose meshes were handed new
vertices holds, and renders, the bits of a scene freshly created from the same description.

The cases are tests/test_mesh_update_host.py's (build_case: cube, wave24, wave40, collapse, alpha, light, instances, deep), frames of
48 x 32 at 4 spp. Per case A = DeviceScene(first state); for every further state A.update_meshes(state) is compared with
B = DeviceScene(state): mesh_records of every mesh (MeshDev, link-word nodes, leaf records, shading records, vertex arrays — byte
for byte; the node array is repacked as create packs it, so even the offsets are create's), scene_graph(), the stack bound (before
any render), yart_hip_bvh_copy against the host builder, render_aovs under the default, general and megakernel pipelines; the frame
differs from the previous state's, a deformed node is seen in `ids`, and the way back reproduces the first frame.

The one YART_E_INVALID condition without a case here: a rebuilt tree deeper than 192 levels. Finite f32 geometry drives the builder to
about 80 levels (scenes.chain_mesh), so no mesh reaches it; the check is scene creation's own (host_scene.hpp::checkStackBound,
tests/test_traversal_stack.py), applied to the need the `deep` case compares."""
import copy
import ctypes

import numpy as np
import pytest

from tests.test_mesh_update_host import CASES, build_case, deformed_nodes, host_tree, update_arrays
from tests.test_scene_update import FLAGS, bits, raw, refit_reference, render_all, same_render


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def same_records(A, B, n_meshes, tag):
    """mesh_records of every mesh on bytes; returns A's"""
    out = []
    for m in range(n_meshes):
        a, b = A.mesh_records(m), B.mesh_records(m)
        assert int(a["mesh"]["node_offset"]) % 2 == 1, f"{tag}: mesh {m}: its base is odd"
        assert a["mesh"].tobytes() == b["mesh"].tobytes(), f"{tag}: mesh {m}: MeshDev {a['mesh']} != {b['mesh']}"
        for name in ("nodes", "leaves", "shade", "positions", "normals", "tangents"):
            assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), f"{tag}: mesh {m}: {name}"
        out.append(a)
    return out


def same_graph(A, B, rebuild_top, tlas_before, tag):
    (na, wa, ta), (nb, wb, tb) = A.scene_graph(), B.scene_graph()
    assert np.array_equal(raw(na), raw(nb)), f"{tag}: NodeDev records"
    assert np.array_equal(raw(wa), raw(wb)), f"{tag}: nodeWorld"
    assert len(ta) == len(tb) and (len(ta) > 0) == (len(na) >= 64)
    if rebuild_top or len(ta) == 0:
        assert np.array_equal(raw(ta), raw(tb)), f"{tag}: top-level hierarchy"
    else:                                                     # a refit keeps the tree: checked as tests/test_scene_update.py checks it
        assert np.array_equal(ta["a"], tlas_before["a"]) and np.array_equal(ta["b"], tlas_before["b"]), f"{tag}: a refit keeps the tree"
        lo, hi = refit_reference(ta, wa)
        assert (ta["lo"] == lo).all() and (ta["hi"] == hi).all(), f"{tag}: refitted boxes"
    return ta


def same_tree_as_host_builder(api, A, s, mesh):
    """yart_hip_bvh_info / yart_hip_bvh_copy return the new tree: the host builder's, on bytes"""
    L = api.lib()
    nn, nt = ctypes.c_uint32(), ctypes.c_uint32()
    api._check(L.yart_hip_bvh_info(A.handle, mesh, ctypes.byref(nn), ctypes.byref(nt)), L)
    nodes, idx = np.zeros((nn.value, 8), np.uint32), np.zeros(nt.value, np.uint32)
    api._check(L.yart_hip_bvh_copy(A.handle, mesh, nodes.ctypes.data_as(ctypes.c_void_p), idx.ctypes.data_as(ctypes.c_void_p)), L)
    want_nodes, want_idx = host_tree(s, mesh)
    assert nodes.shape == want_nodes.shape and np.array_equal(nodes, want_nodes) and np.array_equal(idx, want_idx)


def run_case(api, name, rebuild_top=False, normals=True, min_launches=8):
    states, p, meshes = build_case(name)
    A = api.DeviceScene(states[0], device=0)
    first = [A.mesh_records(m) for m in range(len(states[0].meshes))]
    bound0 = first[0]["stack_bound"]
    r0 = render_all(A, p)
    _, _, tlas = A.scene_graph()
    previous, counts = r0, [int(first[meshes[0]]["mesh"]["n_nodes"])]
    for k, s in enumerate(states[1:], 1):
        tag = f"{name} state {k}"
        A.update_meshes(update_arrays(s, meshes, normals), rebuild_top=rebuild_top)
        stats = A.last_update
        assert stats["launches"] >= min_launches and stats["ms_total"] > 0, stats
        assert (stats["launches"] < 8) == (min_launches < 8), f"device build or host build as asked: {stats}"
        B = api.DeviceScene(s, device=0)
        recs = same_records(A, B, len(s.meshes), tag)
        tlas = same_graph(A, B, rebuild_top, tlas, tag)
        assert recs[0]["stack_bound"] == B.mesh_records(0)["stack_bound"], f"{tag}: stack bound"       # before any render
        for m in meshes:
            same_tree_as_host_builder(api, A, s, m)
        counts.append(int(recs[meshes[0]]["mesh"]["n_nodes"]))
        print(f"{tag}: mesh {meshes[0]}: {counts[-1]} nodes, stack bound {recs[0]['stack_bound']}, update {stats}")
        if name == "deep":
            assert bound0 == 80 and recs[0]["stack_bound"] < 64, "the bound follows the tree down"
        if name == "collapse":
            assert counts[-1] == 1 and int(recs[meshes[0]]["nodes"]["span"][0]) == 1152
            assert int(recs[meshes[0]]["nodes"]["link"][0]) >> 27 == 31 and int(recs[meshes[0]]["leaves"]["mat_flags"][0]) >> 8 == 1152
        if name == "alpha":
            link = recs[meshes[0]]["nodes"]["link"]
            assert int(recs[meshes[0]]["mesh"]["has_alpha"]) == 1 and (link >> 26 & 1).any() and not (link >> 26 & 1).all()
        current = None
        for ftag, flags in FLAGS.items():
            ra, rb = render_all(A, p, flags), render_all(B, p, flags)
            same_render(ra, rb, f"{tag} {ftag}")
            current = current or ra
        B.close()
        assert (bits(current["frame"]) != bits(previous["frame"])).any(), f"{tag}: the deformation does not change the frame"
        seen = np.isin(current["ids"][..., 0], deformed_nodes(s, meshes))
        if name == "collapse":                                # (triangles of no area: nothing of the mesh is hit; it is seen in the first state)
            assert not seen.any() and np.isin(r0["ids"][..., 0], deformed_nodes(s, meshes)).any()
        else:
            assert seen.any(), f"{tag}: no pixel shows a deformed node"
        previous = current
    if name in ("wave24", "wave40"):
        assert all(a != b for a, b in zip(counts, counts[1:])), f"nNodes differs between the states: {counts}"
    # the round trip
    A.update_meshes(update_arrays(states[0], meshes, normals), rebuild_top=rebuild_top)
    back = [A.mesh_records(m) for m in range(len(states[0].meshes))]
    assert back[0]["stack_bound"] == bound0, "the bound follows the tree back"
    for a, b in zip(back, first):
        for key in ("nodes", "leaves", "shade", "positions", "normals", "tangents"):
            assert a[key].tobytes() == b[key].tobytes(), f"{name} round trip: {key}"
        assert a["mesh"].tobytes() == b["mesh"].tobytes()
    same_render(render_all(A, p), r0, f"{name} round trip")
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_updated_meshes_equal_a_fresh_scene(gpu_api, name):
    run_case(gpu_api, name)


@pytest.mark.gpu
def test_instances_with_a_rebuilt_top_level(gpu_api):
    run_case(gpu_api, "instances", rebuild_top=True)


@pytest.mark.gpu
def test_alpha_with_kept_normals(gpu_api):
    """normals=None, tangents=None: the fresh scene has the new positions and the old normals and tangents"""
    run_case(gpu_api, "alpha", normals=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["alpha", "wave24"])
def test_host_builder_path(gpu_api, monkeypatch, name):
    """Under YART_HOST_BVH — and for a mesh the device build refuses — the tree is built and derived on the host (mesh_update.hpp's
    muDeriveHost) and uploaded: the same bytes, the same frames; the build launches nothing."""
    monkeypatch.setenv("YART_HOST_BVH", "1")
    run_case(gpu_api, name, min_launches=2)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["nodes_first", "meshes_first"])
def test_combined_with_a_node_update(gpu_api, order):
    """update(nodes) then update_meshes, and the reverse: each equal to the fresh scene"""
    from yart_amd.yscn import trs
    api = gpu_api
    states, p, meshes = build_case("cube")
    s1 = copy.deepcopy(states[1])
    m = trs((0.5, 5.0, 3.0), (1, 2, 0.5), 0.7)[0].astype(np.float64)
    f = (m @ np.asarray(s1.nodes[2].fwd, np.float64)).astype(np.float32)
    s1.nodes[2].fwd, s1.nodes[2].inv = f, np.linalg.inv(f.astype(np.float64)).astype(np.float32)
    A = api.DeviceScene(states[0], device=0)
    r0 = render_all(A, p)
    if order == "nodes_first":
        A.update(s1.nodes)
        A.update_meshes(update_arrays(s1, meshes))
    else:
        A.update_meshes(update_arrays(s1, meshes))
        A.update(s1.nodes)
    B = api.DeviceScene(s1, device=0)
    same_records(A, B, len(s1.meshes), order)
    same_graph(A, B, False, None, order)
    for ftag, flags in FLAGS.items():
        ra = render_all(A, p, flags)
        same_render(ra, render_all(B, p, flags), f"{order} {ftag}")
    assert (bits(ra["frame"]) != bits(r0["frame"])).any()
    A.close()
    B.close()


@pytest.mark.gpu
def test_refused_updates_leave_the_scene_alone(gpu_api):
    """Every YART_E_INVALID condition that needs a scene: mesh_records and scene_graph() are byte-identical afterwards, and a render
    gives the frame from before."""
    api = gpu_api
    L = api.lib()
    states, p, meshes = build_case("alpha")
    s0, s1 = states
    mesh = meshes[0]
    A = api.DeviceScene(s0, device=0)
    n_meshes = len(s0.meshes)
    before = [A.mesh_records(m) for m in range(n_meshes)]
    graph = A.scene_graph()
    frame0 = render_all(A, p)

    def untouched(word):
        for m, b in enumerate(before):
            a = A.mesh_records(m)
            assert a["stack_bound"] == b["stack_bound"]
            for key in ("mesh", "nodes", "leaves", "shade", "positions", "normals", "tangents"):
                assert a[key].tobytes() == b[key].tobytes(), (word, m, key)
        for x, y in zip(A.scene_graph(), graph):
            assert np.array_equal(raw(x), raw(y)), word

    def refused(arrays, word, **kw):
        with pytest.raises(api.YartError, match=word) as e:
            A.update_meshes(arrays, **kw)
        assert e.value.code == api.YART_E_INVALID
        untouched(word)
    pos, nrm, tan = (np.asarray(a, np.float32) for a in (s1.meshes[mesh].positions, s1.meshes[mesh].normals, s1.meshes[mesh].tangents))
    refused({}, "n_meshes")
    refused({n_meshes: (pos,)}, "out of range")
    refused({mesh: (pos[:-1],)}, "n_vertices")
    refused({mesh: (np.concatenate([pos, pos[:1]]),)}, "n_vertices")
    refused({mesh: (None, nrm, tan)}, "positions pointer is null")
    other = next(m for m in range(n_meshes) if m != mesh)
    refused({other: (np.asarray(s0.meshes[other].positions, np.float32),), mesh: (pos[:-1],)}, "n_vertices")       # the second of two
    for bad in (np.nan, np.inf, -np.inf):
        for k, (arr, word) in enumerate(((pos, "position"), (nrm, "normal"), (tan, "tangent"))):
            broken = arr.copy()
            broken.reshape(-1)[7] = bad
            arrays = [pos, nrm, tan]
            arrays[k] = broken
            refused({mesh: tuple(arrays)}, f"{word} word is not finite")
    # through the C ABI: listed twice, more meshes than the scene has, unknown flags, a small struct, a small stats struct
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    size = ctypes.sizeof(api.SceneMeshUpdate)
    one = api.MeshUpdate(mesh, len(pos), vp(pos), None, None)
    twice = (api.MeshUpdate * 2)(one, one)
    many = (api.MeshUpdate * (n_meshes + 1))(*([one] * (n_meshes + 1)))
    small_stats = api.SceneUpdateStats(4)
    for up, stats, word in ((api.SceneMeshUpdate(size, 2, twice, 0), None, b"listed twice"), (api.SceneMeshUpdate(size, n_meshes + 1, many, 0), None, b"n_meshes"),
                            (api.SceneMeshUpdate(size, 1, twice, 6), None, b"flags"), (api.SceneMeshUpdate(16, 1, twice, 0), None, b"struct_size"),
                            (api.SceneMeshUpdate(size, 1, twice, 0), ctypes.byref(small_stats), b"stats")):
        assert L.yart_hip_scene_update_meshes(A.handle, ctypes.byref(up), None, stats) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
        untouched(word)
    same_render(render_all(A, p), frame0, "after the refused updates")
    # ... and the scene still takes an update
    A.update_meshes(update_arrays(s1, meshes))
    B = api.DeviceScene(s1, device=0)
    same_records(A, B, n_meshes, "after the refused updates")
    B.close()
    A.close()
