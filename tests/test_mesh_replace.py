"""yart_hip_scene_replace_meshes on the device (include/yart_hip.h; csrc/mesh_replace_kernels.inc): a scene whose meshes were replaced
by meshes with other faces and other triangle and vertex counts holds, and renders, the bits of a scene freshly created from the
same description.

The cases are tests/meshreplacecases.py's (grow_first, shrink_middle, last, same_counts, two, single_leaf, lod, alpha, instances,
deep), frames of 48 x 32 at 4 spp. Per case A = DeviceScene(state 0); for every further state A.replace_meshes(the meshes that
differ) is compared with B = DeviceScene(state): geometry() — every pool whole, the zero pad and tail records of bvhNodes and the
MeshDev records included — on bytes, scene_graph(), the stack bound (before any render), yart_hip_bvh_copy against the host builder,
render_aovs under the default, general and megakernel pipelines; the way back to state 0 reproduces the first pools and frame.

The one YART_E_INVALID condition without a case here: a rebuilt tree deeper than 192 levels (tests/test_mesh_update.py says why no
finite mesh reaches it); the check is the one scene creation and update_meshes apply (host_scene.hpp::checkStackBound)."""
import copy
import ctypes

import numpy as np
import pytest

from tests.meshreplacecases import CASES, build_case, cube, listed, one_triangle, patch, replacement, room
from tests.test_mesh_update import same_graph, same_tree_as_host_builder
from tests.test_scene_update import FLAGS, bits, raw, render_all, same_render

POOLS = ("bvh_nodes", "leaf_tris", "shade_tris", "tri_verts", "tri_light", "vpos", "vnormal", "vtangent", "vuv", "meshes")
REPACK_LAUNCHES = 9                                           # one k_mr_repack per pool


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def same_geometry(a, b, tag):
    for name in POOLS:
        assert a[name].shape == b[name].shape, f"{tag}: {name}: {a[name].shape} != {b[name].shape}"
        assert a[name].tobytes() == b[name].tobytes(), f"{tag}: {name}"
    assert a["stack_bound"] == b["stack_bound"], f"{tag}: stack bound {a['stack_bound']} != {b['stack_bound']}"


def layout_is_creates(g, tag):
    """running sums, odd node bases behind a zero pad record, two zero records behind the last mesh"""
    m = g["meshes"]
    assert (m["tri_offset"] == np.concatenate([[0], np.cumsum(m["n_tris"])[:-1]])).all() and (m["leaf_offset"] == m["tri_offset"]).all(), tag
    assert (m["vert_offset"] == np.concatenate([[0], np.cumsum(m["n_verts"])[:-1]])).all(), tag
    assert (m["node_offset"] % 2 == 1).all(), tag
    nodes = raw(g["bvh_nodes"])
    assert len(nodes) == int(m["node_offset"][-1] + m["n_nodes"][-1]) + 2 and not nodes[-2:].any(), f"{tag}: the two tail records"
    end = 0
    for k in range(len(m)):
        assert not nodes[end:int(m["node_offset"][k])].any(), f"{tag}: the pad record in front of mesh {k}"
        end = int(m["node_offset"][k] + m["n_nodes"][k])
    for k in range(len(m)):                                   # every leaf record points into its own mesh's ShadeTri range
        t = g["leaf_tris"]["tri"][int(m["leaf_offset"][k]):int(m["leaf_offset"][k] + m["n_tris"][k])]
        assert np.array_equal(np.sort(t), np.arange(m["tri_offset"][k], m["tri_offset"][k] + m["n_tris"][k], dtype=np.uint32)), f"{tag}: triIdx of mesh {k}"


def compare_with_fresh(api, A, s, p, meshes, tag, rebuild_top=False, tlas=None):
    B = api.DeviceScene(s, device=0)
    ga, gb = A.geometry(), B.geometry()
    same_geometry(ga, gb, tag)                                # (before any render: the stack bound is in it)
    layout_is_creates(ga, tag)
    tlas = same_graph(A, B, rebuild_top, tlas, tag)
    for m in meshes:
        same_tree_as_host_builder(api, A, s, m)
    frames = None
    for ftag, flags in FLAGS.items():
        ra = render_all(A, p, flags)
        same_render(ra, render_all(B, p, flags), f"{tag} {ftag}")
        frames = frames or ra
    B.close()
    return ga, frames, tlas


def run_case(api, name, rebuild_top=False):
    states, p = build_case(name)
    A = api.DeviceScene(states[0], device=0)
    g0, r0 = A.geometry(), render_all(A, p)
    _, _, tlas = A.scene_graph()
    steps = list(zip(states[:-1], states[1:])) + ([(states[-1], states[0])] if states[-1] is not states[0] else [])
    launches, prev = [], g0
    for k, (s0, s1) in enumerate(steps):
        tag = f"{name} step {k}"
        meshes = listed(s0, s1)
        A.replace_meshes(replacement(s1, meshes), rebuild_top=rebuild_top)
        stats = dict(A.last_update)
        assert stats["launches"] >= 3 and stats["ms_total"] > 0, stats
        g, frames, tlas = compare_with_fresh(api, A, s1, p, meshes, tag, rebuild_top, tlas)
        launches.append(stats["launches"])
        keys = ("n_tris", "n_verts", "n_nodes")
        counts = [(int(prev["meshes"][key][m]), int(g["meshes"][key][m])) for m in meshes for key in keys]
        print(f"{tag}: meshes {meshes}: (was, is) {counts}, stack bound {g['stack_bound']}, {stats}")
        # the launches of update_meshes on the same meshes with the same arrays: the staging, two derivation kernels per mesh and the
        # scene-update chain are the replacement's too, so the difference is the repack — 9 launches, or none on the fast path
        A.update_meshes({m: (s1.meshes[m].positions, s1.meshes[m].normals, s1.meshes[m].tangents) for m in meshes}, rebuild_top=rebuild_top)
        same_geometry(A.geometry(), g, f"{tag}: update_meshes with the same arrays")
        extra = stats["launches"] - A.last_update["launches"]
        changed = any(was != now for was, now in counts)
        assert (name == "same_counts") == (not changed), f"{tag}: only same_counts keeps every count: {counts}"
        assert extra == (REPACK_LAUNCHES if changed else 0), f"{tag}: {stats} against {A.last_update}"
        prev = g
        if name == "deep" and k == 0:
            assert g0["stack_bound"] == 80 and g["stack_bound"] < 64, "the bound follows the tree down"
        if name == "alpha" and k == 0:
            md = g["meshes"][meshes[0]]
            link = g["bvh_nodes"]["link"][int(md["node_offset"]):int(md["node_offset"] + md["n_nodes"])]
            assert int(md["has_alpha"]) == 1 and (link >> 26 & 1).all() and int(g0["meshes"]["has_alpha"][meshes[0]]) == 0
        if name == "single_leaf" and k in (0, 2):
            assert int(g["meshes"]["n_nodes"][meshes[0]]) == 1
        if k == 0:
            assert (bits(frames["frame"]) != bits(r0["frame"])).any(), f"{tag}: the replacement does not change the frame"
    # the way back has been the last step
    same_geometry(A.geometry(), g0, f"{name} round trip")
    same_render(render_all(A, p), r0, f"{name} round trip")
    A.close()
    return launches


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_replaced_meshes_equal_a_fresh_scene(gpu_api, name):
    run_case(gpu_api, name)


@pytest.mark.gpu
@pytest.mark.parametrize("rebuild_top", ["host", "device"])
def test_instances_with_a_rebuilt_top_level(gpu_api, rebuild_top):
    run_case(gpu_api, "instances", rebuild_top=rebuild_top)


@pytest.mark.gpu
def test_host_builder_path(gpu_api, monkeypatch):
    """Under YART_HOST_BVH the tree is built and derived on the host and uploaded: the same bytes, the same frames, fewer launches."""
    device = run_case(gpu_api, "two")
    monkeypatch.setenv("YART_HOST_BVH", "1")
    host = run_case(gpu_api, "two")
    assert all(h < d for h, d in zip(host, device)), (host, device)


@pytest.mark.gpu
def test_lod_twice_on_one_handle(gpu_api):
    """The 24^2 -> 48^2 -> 12^2 -> 24^2 sequence twice on one handle — by the second round both arrays of every pool have held the
    largest frame and are reused as they are — ends on the first pools and the first frame."""
    api = gpu_api
    states, p = build_case("lod")
    A = api.DeviceScene(states[0], device=0)
    g0, r0 = A.geometry(), render_all(A, p)
    for _ in range(2):
        for s in states[1:]:
            A.replace_meshes(replacement(s, [1]))
    same_geometry(A.geometry(), g0, "lod twice")
    same_render(render_all(A, p), r0, "lod twice")
    A.close()


@pytest.mark.gpu
def test_alpha_then_update_meshes_and_update_textures(gpu_api):
    """New faces bring an alpha-tested material to a mesh that had none; then update_meshes on that mesh (the cached "no alpha-tested
    face" was forgotten: the link words keep their alpha bits) and update_textures making the texture opaque (the cached material list
    of the mesh was forgotten: its flag and alpha bits are cleared). Both against fresh scenes."""
    api = gpu_api
    states, p = build_case("alpha")
    s0, s1 = states
    mesh = listed(s0, s1)[0]
    leaf = int(s1.meshes[mesh].faces[0, 3])
    tex = s1.materials[leaf].tex_base
    A = api.DeviceScene(s0, device=0)
    A.update_meshes({mesh: s0.meshes[mesh].positions})        # (remembers: no face of the mesh is alpha-tested)
    opaque = np.array(s0.textures[tex].data, copy=True)
    opaque[..., 3] = 255
    A.update_textures({tex: opaque})                           # (flips the flag off and lists the materials of every mesh)
    A.update_textures({tex: s0.textures[tex].data})            # ... and on again
    A.replace_meshes(replacement(s1, [mesh]))
    compare_with_fresh(api, A, s1, p, [mesh], "replace")
    s2 = copy.deepcopy(s1)
    s2.meshes[mesh].positions = np.ascontiguousarray(s1.meshes[mesh].positions * np.float32(1.2) + np.float32(0.05))
    A.update_meshes({mesh: s2.meshes[mesh].positions})
    g, _, _ = compare_with_fresh(api, A, s2, p, [mesh], "replace, update_meshes")
    assert int(g["meshes"]["has_alpha"][mesh]) == 1
    s3 = copy.deepcopy(s2)
    s3.textures[tex].data = opaque
    A.update_textures({tex: opaque})
    g, _, _ = compare_with_fresh(api, A, s3, p, [mesh], "replace, update_meshes, update_textures")
    assert int(g["meshes"]["has_alpha"][mesh]) == 0 and not (g["bvh_nodes"]["link"] >> 26 & 1).any()
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["replace_first", "replace_last"])
def test_combined_with_the_other_entries(gpu_api, order):
    """replace_meshes with update (a node moved), update_graph (a node added) and update_lighting (a material changed), in both
    orders: equal to a scene created from the final description."""
    from yart_amd.yscn import Node, trs
    api = gpu_api
    states, p = build_case("two")
    s0, s1 = states
    moved = copy.deepcopy(s1)
    moved.nodes[2].fwd, moved.nodes[2].inv = trs(translation=(0.2, 0.5, -0.4), axis=(0, 1, 0), angle=0.8)
    final = copy.deepcopy(moved)
    f, i = trs(translation=(0.0, 1.6, 0.5), scale=(0.5, 0.5, 0.5))
    final.nodes.append(Node(parent=0, mesh=1, fwd=f, inv=i))
    final.materials[2].base = (0.9, 0.6, 0.1)
    final.materials[2].roughness = 0.2
    meshes = listed(s0, s1)
    A = api.DeviceScene(s0, device=0)
    if order == "replace_first":
        A.replace_meshes(replacement(final, meshes))
        A.update(moved.nodes)
        A.update_graph(final.nodes)
        A.update_lighting(materials=final.materials)
    else:
        A.update_lighting(materials=final.materials)
        A.update([moved.nodes[k] for k in range(len(s0.nodes))])
        A.update_graph(final.nodes)
        A.replace_meshes(replacement(final, meshes))
    B = api.DeviceScene(final, device=0)
    same_geometry(A.geometry(), B.geometry(), order)
    (na, wa, ta), (nb, wb, tb) = A.scene_graph(), B.scene_graph()
    assert np.array_equal(raw(na), raw(nb)) and np.array_equal(raw(wa), raw(wb)) and np.array_equal(raw(ta), raw(tb)), f"{order}: scene graph"
    la, lb = A.lighting_records(), B.lighting_records()
    assert la["materials"].tobytes() == lb["materials"].tobytes(), f"{order}: materials"
    for ftag, flags in FLAGS.items():
        same_render(render_all(A, p, flags), render_all(B, p, flags), f"{order} {ftag}")
    A.close()
    B.close()


@pytest.mark.gpu
def test_replace_discards_the_kept_frame(gpu_api):
    """keep_previous, then replace_meshes, then pixel_motion: the kept vertex array is indexed by scene-wide vertex, so the frame is
    gone — the "never called" error; keep_previous afterwards works again."""
    api = gpu_api
    states, p = build_case("grow_first")
    A = api.DeviceScene(states[0], device=0)
    A.keep_previous()
    aovs = render_all(A, p)
    assert A.pixel_motion(aovs).shape == (p["size"][1], p["size"][0], 8)
    A.replace_meshes(replacement(states[1], [0]))
    aovs = render_all(A, p)
    with pytest.raises(api.YartError, match="never called") as e:
        A.pixel_motion(aovs)
    assert e.value.code == api.YART_E_INVALID
    A.keep_previous()
    assert A.pixel_motion(aovs).shape == (p["size"][1], p["size"][0], 8)
    A.close()


@pytest.mark.gpu
def test_refused_replacements_leave_the_scene_alone(gpu_api):
    """Every YART_E_INVALID condition that needs a scene (all but the 192-level tree): geometry() and scene_graph() are byte-identical
    after each of them, and a render gives the frame from before."""
    api = gpu_api
    L = api.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    from yart_amd import scenes
    # the room of `lod` in front (mesh 0: emissive, with area lights), two meshes behind it: a cube that no light names but whose
    # face_light has an entry (create asks only that the entry is below the light count), and a plain patch
    s0, p = scenes.cornell(48, 32, 4, 4)
    for k, m in enumerate((cube(0), patch(4, 3, 1))):
        s0.add_node(s0.add_mesh(m), 0)
    s0.create_area_lights()
    assert (s0.meshes[1].face_light == -1).all() and all(l.mesh == 0 for l in s0.lights)
    s0.meshes[1].face_light[2] = 0
    n_meshes, mesh = len(s0.meshes), 2
    A = api.DeviceScene(s0, device=0)
    before, graph, frame0 = A.geometry(), A.scene_graph(), render_all(A, p)

    def untouched(word):
        same_geometry(A.geometry(), before, word)
        for x, y in zip(A.scene_graph(), graph):
            assert np.array_equal(raw(x), raw(y)), word
        same_render(render_all(A, p), frame0, f"after the refusal: {word}")

    good = patch(5, 3, 1)
    arrays = lambda m: [np.ascontiguousarray(a) for a in (m.positions, m.normals, m.tangents, m.uvs, m.faces)]

    def refused(meshes, word, **kw):
        with pytest.raises(api.YartError, match=word) as e:
            A.replace_meshes(meshes, **kw)
        assert e.value.code == api.YART_E_INVALID
        untouched(word)

    refused({}, "n_meshes")
    refused({n_meshes: good}, "out of range")
    refused({0: good}, "a light of the scene is on this mesh")
    refused({1: good}, "the mesh has a face_light entry")     # no light names mesh 1, its triLight has an entry
    light = copy.deepcopy(good)
    light.face_light[3] = 0
    refused({mesh: light}, "face_light has an entry other than -1")
    for k, word in enumerate(("position", "normal", "tangent", "uv")):
        for bad in (np.nan, np.inf, -np.inf):
            a = arrays(good)
            a[k] = a[k].copy()
            a[k].reshape(-1)[5] = bad
            refused({mesh: tuple(a)}, f"{word} word is not finite")
    a = arrays(good)
    a[4] = a[4].copy(); a[4][7, 1] = len(good.positions)
    refused({mesh: tuple(a)}, "vertex index out of range")
    a = arrays(good)
    a[4] = a[4].copy(); a[4][2, 3] = len(s0.materials)
    refused({mesh: tuple(a)}, "material index out of range")
    refused({0: good, mesh: tuple(a)}, "material index out of range")          # the second of two (the faces are looked at before the lights)
    # through the C ABI: counts that are wrong with arrays that are never read, null arrays, listed twice, flags, structs
    g = arrays(good)
    desc = lambda nv, nf, ptrs=None: api.MeshDesc(nv, nf, *(ptrs if ptrs is not None else [vp(x) for x in g]), None)
    size = ctypes.sizeof(api.SceneMeshReplace)
    nv, nf = len(g[0]), len(g[4])
    one = api.MeshReplace(mesh, desc(nv, nf))
    cases = [((api.MeshReplace * 1)(api.MeshReplace(mesh, desc(nv, 0))), b"n_faces is 0"),
             ((api.MeshReplace * 1)(api.MeshReplace(mesh, desc(nv, 1 << 25))), b"2^25"),
             ((api.MeshReplace * 1)(api.MeshReplace(mesh, desc(0, nf))), b"n_vertices is 0")]
    for k in range(5):
        ptrs = [vp(x) for x in g]
        ptrs[k] = None
        cases.append(((api.MeshReplace * 1)(api.MeshReplace(mesh, desc(nv, nf, ptrs))), b"pointer is null"))
    for md, word in cases:
        up = api.SceneMeshReplace(size, 1, md, 0)
        assert L.yart_hip_scene_replace_meshes(A.handle, ctypes.byref(up), None, None) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
        untouched(word)
    twice = (api.MeshReplace * 2)(one, one)
    many = (api.MeshReplace * (n_meshes + 1))(*([one] * (n_meshes + 1)))
    small_stats = api.SceneUpdateStats(4)
    for up, stats, word in ((api.SceneMeshReplace(size, 2, twice, 0), None, b"listed twice"), (api.SceneMeshReplace(size, n_meshes + 1, many, 0), None, b"n_meshes"),
                            (api.SceneMeshReplace(size, 1, twice, 4), None, b"flags"), (api.SceneMeshReplace(size, 1, twice, 3), None, b"exclude"),
                            (api.SceneMeshReplace(16, 1, twice, 0), None, b"struct_size"), (api.SceneMeshReplace(size, 1, None, 0), None, b"null"),
                            (api.SceneMeshReplace(size, 1, twice, 0), ctypes.byref(small_stats), b"stats")):
        assert L.yart_hip_scene_replace_meshes(A.handle, ctypes.byref(up), None, stats) == api.YART_E_INVALID
        assert word in L.yart_hip_last_error(), L.yart_hip_last_error()
        untouched(word)
    # ... and the scene still takes a replacement
    s1 = copy.deepcopy(s0)
    s1.meshes[mesh] = good
    A.replace_meshes({mesh: good})
    compare_with_fresh(api, A, s1, p, [mesh], "after the refused replacements")
    A.close()
    # a mesh that is not listed whose vertex box is not finite (an unused vertex at +inf): the scene is created, and cannot be updated
    s2, p2 = room([cube(1), cube(2), one_triangle(3)])
    m = s2.meshes[0]
    m.positions = np.concatenate([m.positions, np.array([[np.inf, 0.0, 0.0]], np.float32)])
    m.normals, m.tangents, m.uvs = (np.concatenate([x, x[-1:]]) for x in (m.normals, m.tangents, m.uvs))
    C2 = api.DeviceScene(s2, device=0)
    g2, graph2, frame2 = C2.geometry(), C2.scene_graph(), render_all(C2, p2)
    with pytest.raises(api.YartError, match="vertex box is not finite") as e:
        C2.replace_meshes({1: good})
    assert e.value.code == api.YART_E_INVALID
    same_geometry(C2.geometry(), g2, "vertex box")
    for x, y in zip(C2.scene_graph(), graph2):
        assert np.array_equal(raw(x), raw(y)), "vertex box"
    same_render(render_all(C2, p2), frame2, "after the refusal: vertex box")
    C2.replace_meshes({0: cube(1)})                           # (listing the mesh replaces the box: accepted)
    C2.close()
