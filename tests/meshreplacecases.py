"""The cases tests/test_mesh_replace_host.py (the host simulator) and tests/test_mesh_replace.py (the device) share: per case a list of
states of one scene — same materials, textures, nodes and mesh count — that differ in whole meshes: faces, vertex counts, uvs.
Frames of 48 x 32 at 4 spp. A mesh that differs between two states is what a step lists (`listed`).

  grow_first     three meshes under a sky; mesh 0 goes from a 12-triangle cube to a 44-triangle patch (36 vertices for 24): every
                 later mesh moves up, the triIdx delta is +32
  shrink_middle  the middle mesh of three goes from 80 triangles to 12: delta -68, source and destination ranges overlap forwards
  last           only the last of three meshes changes (12 -> 30 triangles): no record of another mesh moves, the tail records stay
  same_counts    a 4 x 4 patch re-triangulated along the other diagonal, a material per face: equal triangle, vertex AND node counts
  two            four meshes; mesh 0 grows by 24 triangles and 14 vertices, mesh 2 shrinks by as many: mesh 1 between them moves
                 (delta +24), mesh 3 behind both has delta 0
  single_leaf    four cubes; mesh 1 becomes one triangle and a cube again, then the last mesh does: nNodes = 1, the nodes[1] / nodes[2]
                 reads of its walk land in the next mesh's pad record and root, or in the two tail records; every later base moves
  lod            the height field of test_mesh_update_host.wave_scene at 24^2, 48^2, 12^2, 24^2 (1152, 4608, 288 triangles: across
                 devbvh::kBigSpan = 2048); two meshes (the room, which is emissive and never listed, and the field)
  alpha          scenes.alpha_instances with its glass pane (2 triangles, no alpha-tested material) replaced by 24 leaf cards
  instances      scenes.instances(70, 4): the instanced cube replaced by a 40-triangle patch
  deep           scenes.deep_tree's scene: chain_mesh(80) (stack need 80) replaced by a flat row of 50 triangles and back"""
import copy

import numpy as np

from tests.test_scene_update_host import SIZE, SPP

CASES = ["grow_first", "shrink_middle", "last", "same_counts", "two", "single_leaf", "lod", "alpha", "instances", "deep"]
WHITE, BLUE, RED, GREEN = 0, 1, 2, 3


def cube(mat, h=0.6):
    from yart_amd import scenes
    b = scenes.MeshBuilder()
    b.box((-h, 0.0, -h), (h, 2.0 * h, h), mat)
    return b.build()


def patch(nu, nv, mat, bump=0.3, flip_diagonals=False, per_face_materials=None):
    """a wavy (nu x nv)-quad patch of 2 nu nv triangles over [-0.8, 0.8]^2, uvs scaled by (2, 3)"""
    from yart_amd import scenes
    b = scenes.MeshBuilder()
    b.grid(lambda U, V: ((U - 0.5) * 1.6, 0.4 + bump * np.sin(5.0 * U) * np.cos(4.0 * V), (V - 0.5) * 1.6), nu, nv, mat, uv_scale=(2.0, 3.0), flip=True)
    m = b.build()
    if flip_diagonals:                                        # (a, c, b), (a, d, c) -> (a, d, b), (b, d, c): the quad's other diagonal
        f = m.faces.reshape(-1, 2, 4).copy()
        a, c, bb, d = f[:, 0, 0].copy(), f[:, 0, 1].copy(), f[:, 0, 2].copy(), f[:, 1, 1].copy()
        f[:, 0, :3] = np.stack([a, d, bb], -1)
        f[:, 1, :3] = np.stack([bb, d, c], -1)
        m.faces = np.ascontiguousarray(f.reshape(-1, 4))
    if per_face_materials is not None:
        m.faces[:, 3] = np.resize(np.asarray(per_face_materials, np.uint32), len(m.faces))
    return m


def one_triangle(mat):
    from yart_amd.yscn import Mesh
    p = np.array([[-0.5, 0.1, 0.0], [0.5, 0.1, 0.0], [0.0, 1.2, 0.2]], np.float32)
    n = np.tile(np.array([0.0, -0.18, 0.98], np.float32), (3, 1))
    t = np.tile(np.array([1.0, 0.0, 0.0, 1.0], np.float32), (3, 1))
    uv = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]], np.float32)
    return Mesh(p, n, t, uv, np.array([[0, 1, 2, mat]], np.uint32))


def room(meshes):
    """the meshes side by side on a floor-less stage under a uniform sky: no mesh is emissive, every mesh can be replaced"""
    from yart_amd import yscn
    from yart_amd.yscn import Material, Light, LIGHT_UNIFORM_INF
    s = yscn.Scene()
    for base, rough in (((0.73, 0.73, 0.73), 1.0), ((0.2, 0.3, 0.8), 0.5), ((0.7, 0.1, 0.1), 0.9), ((0.1, 0.5, 0.2), 0.3)):
        s.add_material(Material(base=base, roughness=rough))
    for k, m in enumerate(meshes):
        f, i = yscn.trs(translation=((k - (len(meshes) - 1) / 2.0) * 1.9, 0.0, 0.0), axis=(0, 1, 0), angle=0.3 * k)
        s.add_node(s.add_mesh(m), 0, f, i)
    s.lights.append(Light(LIGHT_UNIFORM_INF, radius=100.0, emission=(0.8, 0.85, 1.0)))
    p = dict(size=SIZE, spp=SPP, depth=4, focal=35.0, fnumber=0.0, eye=(0.0, 2.0, 7.0), target=(0.0, 0.6, 0.0), up=(0.0, 1.0, 0.0),
             exposure=0.0, background=(0.0, 0.0, 0.0))
    return s, p


def with_mesh(s, mesh, m):
    s1 = copy.deepcopy(s)
    s1.meshes[mesh] = copy.deepcopy(m)
    return s1


def listed(s0, s1):
    """the meshes a step from s0 to s1 lists: those whose description differs"""
    out = []
    for i, (a, b) in enumerate(zip(s0.meshes, s1.meshes)):
        same = all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))) for k in ("positions", "normals", "tangents", "uvs", "faces"))
        if not same:
            out.append(i)
    return out


def replacement(s, meshes):
    """the argument of DeviceScene.replace_meshes for state s"""
    return {m: s.meshes[m] for m in meshes}


def row_mesh(n, mat):
    """n small triangles with vertices of their own, side by side along x (tests/test_mesh_update_host.row_of_triangles)"""
    from yart_amd.yscn import Mesh
    from tests.test_mesh_update_host import row_of_triangles
    p = row_of_triangles(n)
    nrm = np.tile(np.array([0.0, -0.15, 0.99], np.float32), (3 * n, 1))
    tan = np.tile(np.array([1.0, 0.0, 0.0, 1.0], np.float32), (3 * n, 1))
    uv = np.tile(np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]], np.float32), (n, 1))
    f = np.concatenate([np.arange(3 * n, dtype=np.uint32).reshape(n, 3), np.full((n, 1), mat, np.uint32)], 1)
    return Mesh(p, nrm, tan, uv, f)


def build_case(name):
    """-> (states, params): the way back to states[0] is a step of its own in the tests"""
    from yart_amd import scenes
    if name == "grow_first":
        s0, p = room([cube(BLUE), cube(RED), patch(5, 3, GREEN)])
        return [s0, with_mesh(s0, 0, patch(11, 2, BLUE))], p
    if name == "shrink_middle":
        s0, p = room([patch(6, 6, WHITE), patch(8, 5, RED), cube(GREEN)])
        return [s0, with_mesh(s0, 1, cube(RED, 0.5))], p
    if name == "last":
        s0, p = room([cube(BLUE), patch(4, 3, RED), cube(GREEN)])
        return [s0, with_mesh(s0, 2, patch(5, 3, GREEN))], p
    if name == "same_counts":
        s0, p = room([cube(BLUE), patch(4, 4, RED, bump=0.0), cube(GREEN)])
        return [s0, with_mesh(s0, 1, patch(4, 4, RED, bump=0.0, flip_diagonals=True, per_face_materials=(RED, WHITE, GREEN)))], p
    if name == "two":
        s0, p = room([patch(6, 4, WHITE), cube(RED), patch(6, 6, GREEN), cube(BLUE)])
        s1 = with_mesh(with_mesh(s0, 0, patch(6, 6, WHITE, bump=0.2)), 2, patch(6, 4, GREEN, bump=0.2))
        return [s0, s1], p
    if name == "single_leaf":
        s0, p = room([cube(BLUE), cube(RED), cube(GREEN), cube(WHITE)])
        return [s0, with_mesh(s0, 1, one_triangle(RED)), s0, with_mesh(s0, 3, one_triangle(WHITE))], p
    if name == "lod":
        from tests.test_mesh_update_host import wave_scene
        made = [wave_scene(n, 0.0) for n in (24, 48, 12)]
        for s, _ in made:                                     # (the field is not emissive: its face_light is all -1)
            assert (s.meshes[1].face_light == -1).all() and all(l.mesh == 0 for l in s.lights)
        return [s for s, _ in made] + [made[0][0]], made[0][1]
    if name == "alpha":
        s0, p = scenes.alpha_instances(SIZE[0], SIZE[1], SPP, 5)
        pane = next(i for i, m in enumerate(s0.meshes) if len(m.faces) == 2)
        leaf = next(i for i, m in enumerate(s0.materials) if m.tex_base >= 0)
        cards = patch(4, 3, leaf, bump=0.1)
        cards.positions = np.ascontiguousarray(cards.positions * np.float32(0.6))
        return [s0, with_mesh(s0, pane, cards)], p
    if name == "instances":
        s0, p = scenes.instances(SIZE[0], SIZE[1], SPP, 4, n_instances=70, groups=4)
        assert len(s0.nodes) >= 64
        c = len(s0.meshes) - 1
        m = patch(5, 4, int(s0.meshes[c].faces[0, 3]), bump=0.4)
        m.positions = np.ascontiguousarray(m.positions - np.float32([0.0, 0.4, 0.0]))
        return [s0, with_mesh(s0, c, m)], p
    if name == "deep":
        s0, p = scenes.deep_tree(8, width=SIZE[0], height=SIZE[1], spp=SPP)
        chain = len(s0.meshes) - 1
        mats = sorted({int(f[3]) for f in s0.meshes[chain].faces})
        s0.meshes[chain] = scenes.chain_mesh(80, mats, ratio=21.0)
        assert (s0.meshes[chain].face_light == -1).all() and all(l.mesh != chain for l in s0.lights)
        return [s0, with_mesh(s0, chain, row_mesh(50, mats[0]))], p
    raise KeyError(name)
