"""Temporal accumulation of deforming meshes: the scene remembers a previous frame (yart_hip_scene_keep_previous), says per pixel
where its surface point was in that frame (yart_hip_scene_pixel_motion_*), and the accumulator takes those records
(yart_hip_temporal_set_pixel_motion; PER-PIXEL MOTION in the header comments of include/yart_hip.h).

yart_amd/scene_motion.py `scene_motion_reference` and yart_amd/temporal.py `temporal_reference` / `temporal_moments_reference` with
`pixel_motion=` state the definitions in NumPy and are the reference of every comparison here, on bits: csrc/scene_motion.hpp and
csrc/temporal.hpp compiled for the host (tests/scenemotionsim) and the device kernels k_sm_node_chains, k_sm_pixels and
k_tp_accumulate<., true, true> through api.DeviceScene.keep_previous / pixel_motion / pixel_motion_into,
api.TemporalAccumulator.accumulate / accumulate_into(pixel_motion=) and DeviceScene.render_denoised(temporal=, pixel_motion=True).

The MIXED scene has every kind of pixel, seen from (0, 0, 5) down -z, four patches in the image's quadrants and nothing behind them:
  node 1   static, the rigid mesh 0                                   node 2   under the root, no mesh, MOVES
  node 3   under node 2 (chain depth 2), mesh 0, its own fwd unchanged: moves rigidly with its parent
  node 4   static, mesh 1, which DEFORMS except for the three vertices of its triangle 0
  node 5   moves, mesh 2, which deforms
The SHEET of the feature conditions is the issue's: one node with fwd = translate(0, 0, 1) carrying an 8 x 8-cell grid over
[-3.2, 3.2]^2 at z = 0, two triangles per cell, flat normals, deformed per frame k = 0 .. 3, the colour linear in the rest
coordinates of the hit point."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_temporal as tt
from tests import test_temporal_motion as tm
from tests.conftest import ROOT
from tests.test_temporal import assert_same, bits

CPU_SIZES = [(1, 1), (5, 3), (37, 23)]
GPU_SIZES = [(5, 3), (37, 23), (131, 67)]
FEATURE_SIZES = [(37, 23), (131, 67)]
FRAMES = 4
EXTENT, CELLS = 3.2, 8


# ---------------------------------------------------------------------------------------------------------------------
# the mixed scene
# ---------------------------------------------------------------------------------------------------------------------
def patch(cells, k, keep_first_triangle=False, deform=True):
    """a grid over [-0.9, 0.9] x [-0.6, 0.6] at z = 0 facing +z; frame k: x' = x + 0.1 k (1 - (x / 0.9)^2), z' = 0.12 k cos(2.5 x)"""
    from yart_amd import scenes
    b = scenes.MeshBuilder()
    b.grid(lambda U, V: ((U - 0.5) * 1.8, (V - 0.5) * 1.2, 0.0 * U), cells, cells, 0)
    m = b.build()
    if deform and k:
        p = m.positions.astype(np.float64)
        x = p[:, 0].copy()
        moved = np.ones(len(p), bool)
        if keep_first_triangle:
            moved[m.faces[0, :3].astype(np.int64)] = False
        p[:, 0] = np.where(moved, x + 0.1 * k * (1.0 - (x / 0.9) ** 2) + 0.02 * k, x)
        p[:, 2] = np.where(moved, 0.12 * k * np.cos(2.5 * x), 0.0)
        m.positions = p.astype(np.float32)
    return m


def mixed_scene(k):
    from yart_amd.yscn import LIGHT_UNIFORM_INF, Light, Material, Scene, trs
    s = Scene()
    s.add_material(Material(base=(0.6, 0.6, 0.6), roughness=1.0))
    s.add_mesh(patch(3, k, deform=False))
    s.add_mesh(patch(4, k, keep_first_triangle=True))
    s.add_mesh(patch(4, k))
    s.add_node(0, 0, *trs((-1.1, 0.7, 0.0), (0, 0, 1), 0.2))
    s.add_node(-1, 0, *trs((1.1 + 0.15 * k, 0.7, 0.1 * k), (0, 1, 0), 0.1 * k))
    s.add_node(0, 2, *trs((0.0, 0.0, 0.2), (0, 0, 1), -0.3))
    s.add_node(1, 0, *trs((-1.1, -0.7, 0.0)))
    s.add_node(2, 0, *trs((1.1 - 0.1 * k, -0.7 + 0.05 * k, 0.2 * k), (1, 0, 0), 0.15 * k, 1.0 + 0.1 * k))
    s.lights.append(Light(LIGHT_UNIFORM_INF, radius=100.0, emission=(1.0, 1.0, 1.0)))
    return s


def mixed_params(w, h, spp=4):
    return dict(size=(w, h), spp=spp, depth=2, focal=35.0, fnumber=0.0, sensor=(36.0, 24.0), eye=(0.0, 0.0, 5.0),
                target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), exposure=0.0, background=(0.0, 0.0, 0.0))


def world64(nodes, k):
    m = np.eye(4)
    while k >= 0:
        m = np.asarray(nodes[k].fwd, np.float64).reshape(4, 4) @ m
        k = nodes[k].parent
    return m


_mixed = {}


def mixed_buffers(w, h):
    """Feature buffers for the mixed scene's frame 1 that need no renderer: per pixel a seeded random mesh node and triangle, a point
    of that triangle (or a little beyond it) through the node's float64 chain, a normal near the triangle's; and among them
    coverage < 1, non-finite P and n, ids of -1, a node without a mesh, and nodes and triangles out of range."""
    if (w, h) not in _mixed:
        s = mixed_scene(1)
        rng = np.random.RandomState(77 * w + h)
        n = w * h
        mesh_nodes = [i for i, nd in enumerate(s.nodes) if nd.mesh >= 0]
        node = rng.choice(mesh_nodes, n)
        if n >= 4:
            node[:4] = mesh_nodes                        # every kind of pixel at every size but 1 x 1
        P, nrm, tri = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int64)
        for i in range(n):
            m = s.meshes[s.nodes[node[i]].mesh]
            tri[i] = rng.randint(len(m.faces)) if i >= 10 else 0
            a, b, c = m.positions[m.faces[tri[i], :3].astype(np.int64)].astype(np.float64)
            u, v = rng.uniform(-0.1, 0.6, 2)
            W = world64(s.nodes, node[i])
            P[i] = W[:3, :3] @ (a + u * (b - a) + v * (c - a)) + W[:3, 3]
            g = W[:3, :3] @ np.cross(b - a, c - a)
            nrm[i] = g / np.linalg.norm(g) + rng.normal(0, 0.05, 3)
        ids = np.stack([node, [s.nodes[i].mesh for i in node], np.zeros(n, np.int64), tri], -1).astype(np.int32)
        cov = np.ones(n, np.float32)
        P, nrm = P.astype(np.float32), nrm.astype(np.float32)
        if n >= 15:
            if n >= 100:
                cov[4:][rng.rand(n - 4) < 0.05] = 0.75
            i = bad_pixels(n)
            cov[i[0]] = 0.0
            P[i[1], 0] = np.inf
            P[i[2], 2] = np.nan
            nrm[i[3], 1] = np.nan
            nrm[i[4], 0] = -np.inf
            ids[i[5]] = -1
            ids[i[6], 0] = 2                             # a node without a mesh
            ids[i[7], 0] = len(s.nodes)                  # the first node out of range
            ids[i[8], 0] = 0x7fffffff
            ids[i[9], 3] = len(s.meshes[s.nodes[ids[i[9], 0]].mesh].faces)      # the first triangle out of range
            ids[i[10], 3] = -1
            cov[i[11]] = 1.0
            ids[i[11], 1] = 7                            # ids[1] is not looked at
        out = dict(position=P.reshape(h, w, 3), normal=nrm.reshape(h, w, 3), coverage=cov.reshape(h, w), ids=ids.reshape(h, w, 4))
        for v in out.values():
            v.setflags(write=False)
        _mixed[(w, h)] = out
    return _mixed[(w, h)]


def bad_pixels(n):
    """eleven pixels that mixed_buffers spoils, one way each, and a twelfth whose ids[1] is wrong (which spoils nothing)"""
    return list(range(4, 15)) + [1] if n < 100 else [n // 2, n // 3, n // 3 + 1, n // 4, n // 4 + 1, n // 5, n // 5 + 1, n // 5 + 2, n // 5 + 3,
                                                n // 6, n // 6 + 1, n // 6 + 2]


def statement_of_scenes(s0, s1, buf):
    from yart_amd.scene_motion import scene_motion_reference
    return scene_motion_reference(s0.nodes, s1.nodes, s1.meshes, [m.positions for m in s0.meshes], [m.positions for m in s1.meshes],
                                  buf["position"], buf["normal"], buf["coverage"], buf["ids"])


def kinds(rec):
    return np.ascontiguousarray(rec).view(np.uint32)[..., 3]


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_and_argument_errors(built, tmp_path):
    """The four new entries are exported and listed in api.EXPORTS, the ABI is still 3, YartTemporalPixelMotion has the same size in
    ctypes and for a C++ compiler (which also sees DeviceScene::keepPrevious / pixelMotion and Temporal::setPixelMotion), and every
    refusal that needs no scene is YART_E_INVALID with a telling message — no device is touched (the scene handle is never
    dereferenced; the refusal of a scene without a kept frame is test_device_refusals)."""
    from yart_amd import api
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in ("yart_hip_scene_keep_previous", "yart_hip_scene_pixel_motion_device", "yart_hip_scene_pixel_motion_host",
                 "yart_hip_temporal_set_pixel_motion"):
        assert hasattr(raw, name) and name in api.EXPORTS, name
    assert L.yart_hip_abi_version() == 3
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu\\n\", sizeof(YartTemporalPixelMotion));\n"
                "  void (yart::hip::DeviceScene::*keep)(void*) = &yart::hip::DeviceScene::keepPrevious;\n"
                "  std::vector<float> (yart::hip::DeviceScene::*pm)(const YartAovBuffers&, uint32_t, uint32_t) = &yart::hip::DeviceScene::pixelMotion;\n"
                "  yart::hip::Temporal t(4, 4);\n"
                "  std::vector<float> rec(4 * 4 * 8, 0.0f);\n"
                "  t.setPixelMotion(rec.data()); t.setPixelMotion(nullptr);\n"
                "  return keep && pm ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.TemporalPixelMotion)] == [8 + ctypes.sizeof(ctypes.c_void_p)]

    # the scene entries
    assert L.yart_hip_scene_keep_previous(None, None) == api.YART_E_INVALID and b"null" in L.yart_hip_last_error()
    fake = ctypes.c_void_p(0x1000)                       # a handle that is never dereferenced: the other arguments are checked first
    n = 4 * 4
    bufs = dict(position=np.zeros(n * 3, np.float32), normal=np.zeros(n * 3, np.float32), coverage=np.zeros(n, np.float32),
                ids=np.zeros(n * 4, np.int32), depth=np.zeros(n, np.float32))
    rec = np.zeros(n * 8 + 4, np.float32)
    aligned = rec.ctypes.data + (-rec.ctypes.data) % 16

    def aovs(names=("position", "normal", "coverage", "ids"), null=(), struct_size=None, extra_mask=0):
        ab = api.AovBuffers()
        ab.struct_size = ctypes.sizeof(api.AovBuffers) if struct_size is None else struct_size
        ab.mask = extra_mask
        for name in names:
            ab.mask |= api.AOVS[name][0]
            if name not in null:
                setattr(ab, name, bufs[name].ctypes.data_as(ctypes.c_void_p))
        return ab

    def device(scene=fake, ab=None, null_aovs=False, w=4, h=4, records=aligned):
        ab = aovs() if ab is None else ab
        return L.yart_hip_scene_pixel_motion_device(scene, None if null_aovs else ctypes.byref(ab), w, h, ctypes.c_void_p(records), None)

    def host(scene=fake, ab=None, null_aovs=False, w=4, h=4, records=aligned):
        ab = aovs() if ab is None else ab
        return L.yart_hip_scene_pixel_motion_host(scene, None if null_aovs else ctypes.byref(ab), w, h, ctypes.c_void_p(records))
    cases = [(dict(scene=None), b"scene pointer"), (dict(null_aovs=True), b"aovs"), (dict(records=None), b"records"),
             (dict(w=0), b"0"), (dict(h=0), b"0"), (dict(w=1 << 14, h=(1 << 14) + 1), b"2^28"), (dict(w=0xffffffff, h=0xffffffff), b"2^28"),
             (dict(ab=aovs(struct_size=4)), b"struct_size"), (dict(ab=aovs(extra_mask=0x80)), b"mask")]
    for missing, word in (("position", b"position"), ("normal", b"normal"), ("coverage", b"coverage"), ("ids", b"ids")):
        rest = tuple(k for k in ("position", "normal", "coverage", "ids") if k != missing)
        cases.append((dict(ab=aovs(rest)), word))                            # not in the mask
        cases.append((dict(ab=aovs(null=(missing,))), word))                 # in the mask, NULL
    cases.append((dict(ab=aovs(struct_size=api.AovBuffers.ids.offset)), b"ids"))      # in the mask, beyond struct_size
    for fn in (device, host):
        for kw, word in cases:
            assert fn(**kw) == api.YART_E_INVALID, (fn.__name__, kw)
            assert word in L.yart_hip_last_error(), (fn.__name__, kw, L.yart_hip_last_error())
    for off in (4, 8, 12):
        assert device(records=aligned + off) == api.YART_E_INVALID and b"aligned" in L.yart_hip_last_error()

    # the setter
    h = ctypes.c_void_p()
    assert L.yart_hip_temporal_create(4, 4, 0, ctypes.byref(h)) == api.YART_OK and h.value

    def setter(handle=h, struct_size=None, records=aligned, null_motion=False):
        pm = api.TemporalPixelMotion(ctypes.sizeof(api.TemporalPixelMotion) if struct_size is None else struct_size, ctypes.c_void_p(records))
        return L.yart_hip_temporal_set_pixel_motion(handle, None if null_motion else ctypes.byref(pm))
    for kw, word in ((dict(handle=None), b"handle"), (dict(struct_size=8), b"struct_size"), (dict(struct_size=0), b"struct_size"),
                     (dict(records=None), b"records")):
        assert setter(**kw) == api.YART_E_INVALID, kw
        assert word in L.yart_hip_last_error(), (kw, L.yart_hip_last_error())
    assert setter() == api.YART_OK and setter(struct_size=64) == api.YART_OK and setter(records=aligned + 4) == api.YART_OK
    assert setter(null_motion=True) == api.YART_OK and setter(null_motion=True) == api.YART_OK
    assert setter() == api.YART_OK and L.yart_hip_temporal_reset(h) == api.YART_OK
    L.yart_hip_temporal_destroy(h)
    # the Python surface
    acc = api.TemporalAccumulator(4, 4)
    acc.set_pixel_motion(np.zeros((4, 4, 8), np.float32))
    acc.set_pixel_motion(None)
    with pytest.raises(AssertionError):
        acc.set_pixel_motion(np.zeros((4, 4, 8), np.float64))
    with pytest.raises(AssertionError):
        acc.set_pixel_motion(np.zeros((4, 4, 7), np.float32))
    acc.close()


def _build_sim(path, extra=()):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-o", path,
                           os.path.join(ROOT, "tests", "scenemotionsim", "scenemotionsim.cpp"),
                           os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def sim(built, tmp_path_factory):
    """tests/scenemotionsim/scenemotionsim.cpp: csrc/scene_motion.hpp and csrc/temporal.hpp with a per-pixel Motion, for the host"""
    exe = str(tmp_path_factory.mktemp("scenemotionsim") / "scenemotionsim")
    r = _build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_motion_sim(exe, tmp, s0, s1, buf):
    """the records csrc/scene_motion.hpp gives on the host for the scene s0 -> s1 (yscn.Scene; the same topology) and the buffers"""
    from yart_amd import api
    h, w = buf["coverage"].shape
    nodes = []
    for s in (s0, s1):
        nd = np.zeros(len(s.nodes), api.NODE_DTYPE)
        for i, node in enumerate(s.nodes):
            nd[i]["fwd"], nd[i]["inv"] = np.asarray(node.fwd, np.float32).reshape(16), np.asarray(node.inv, np.float32).reshape(16)
            nd[i]["mesh"], nd[i]["parent"] = node.mesh, node.parent
        nodes.append(nd)
    md = np.zeros(len(s1.meshes), api.MESH_DTYPE)
    tris, cur, prev = [], [], []
    for i, (m0, m1) in enumerate(zip(s0.meshes, s1.meshes)):
        md[i]["tri_offset"], md[i]["vert_offset"] = sum(len(t) for t in tris), sum(len(v) for v in cur)
        md[i]["n_tris"], md[i]["n_verts"] = len(m1.faces), len(m1.positions)
        tris.append(np.asarray(m1.faces, np.uint32).reshape(-1, 4))
        for dst, m in ((cur, m1), (prev, m0)):
            v = np.zeros((len(m.positions), 4), np.float32)
            v[:, :3] = m.positions
            dst.append(v)
    tris, cur, prev = np.concatenate(tris), np.concatenate(cur), np.concatenate(prev)
    fin, fout = os.path.join(tmp, "sm.in"), os.path.join(tmp, "sm.out")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(s1.nodes), len(md), len(tris), len(cur)], np.uint32).tobytes())
        for a in (nodes[0], nodes[1], md, tris, cur, prev, buf["position"], buf["normal"], buf["coverage"], buf["ids"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, "motion", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(fout, np.float32).reshape(h, w, 8)


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_scene_motion_equals_the_numpy_statement_on_bits(sim, tmp_path, w, h):
    """csrc/scene_motion.hpp on the host == scene_motion_reference, bit for bit, on the mixed scene's frames 0 -> 1 with
    mixed_buffers; and (from 5 x 3 on) the records are of the kinds the scene was made for: static on nodes 1, on triangle 0 of node
    4's mesh and wherever a buffer says so, moved on nodes 3, 4 and 5."""
    s0, s1, buf = mixed_scene(0), mixed_scene(1), mixed_buffers(w, h)
    want = statement_of_scenes(s0, s1, buf)
    got = run_motion_sim(sim, str(tmp_path), s0, s1, buf)
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{int(diff.sum())} words differ, first at {np.argwhere(diff)[0].tolist()}"
    kind, node, tri = kinds(want).reshape(-1), buf["ids"][..., 0].reshape(-1), buf["ids"][..., 3].reshape(-1)
    assert not bits(want).reshape(-1, 8)[kind == 0].any()
    if w * h >= 15:
        assert kind[:4].tolist() == [0, 1, 0, 1] and node[:4].tolist() == [1, 3, 4, 5] and not tri[:4].any()
        n = w * h
        good = np.ones(n, bool)
        for i in bad_pixels(n)[:11]:
            assert kind[i] == 0, i
            good[i] = False
        good &= buf["coverage"].reshape(-1) == 1.0
        i = bad_pixels(n)[11]
        assert good[i] and kind[i] == (0 if (node[i] == 1 or (node[i] == 4 and tri[i] == 0)) else 1)
        assert not kind[good & (node == 1)].any() and not kind[good & (node == 4) & (tri == 0)].any()
        assert kind[good & (node == 3)].all() and kind[good & (node == 5)].all() and kind[good & (node == 4) & (tri != 0)].all()
        assert np.isfinite(want.reshape(-1, 8)[kind == 1]).all()


def test_nothing_moved_is_all_static(sim, tmp_path):
    """the scene against itself: every record is all zero, in the statement and on the host"""
    s1, buf = mixed_scene(1), mixed_buffers(37, 23)
    assert not bits(statement_of_scenes(s1, s1, buf)).any()
    assert not bits(run_motion_sim(sim, str(tmp_path), s1, s1, buf)).any()


def test_sanitized_sim_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading), once, on the mixed scene."""
    exe = os.path.join(tmp_path, "scenemotionsim_san")
    r = _build_sim(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert r.returncode == 0, r.stderr[-3000:]
    s0, s1, buf = mixed_scene(0), mixed_scene(1), mixed_buffers(37, 23)
    assert np.array_equal(bits(run_motion_sim(exe, str(tmp_path), s0, s1, buf)), bits(statement_of_scenes(s0, s1, buf)))


# -- the accumulator ---------------------------------------------------------------------------------------------------
_records = {}


def records_of(w, h):
    """Per-pixel records for the four frames of test_temporal_motion's `mixed` sequence (None in frame 0): on node 1, which moves
    there, what its per-node record gives (P' = M P, n' = Nm n in float32, the statement's own operations), kind 1; and seeded
    among all pixels: kind-1 records with another P' and n', kind-1 records with a NaN or infinite word, kind-0 and kind-2 records
    whose other words are garbage."""
    if (w, h) not in _records:
        from yart_amd.temporal import _dot
        out = []
        for k, fr in enumerate(tm.frames_of(w, h, "mixed")):
            if fr["motion"] is None:
                out.append(None)
                continue
            rng = np.random.RandomState(9000 + 100 * w + 10 * h + k)
            m = fr["motion"][1]
            P, n = fr["position"], fr["normal"]
            rec = np.zeros((h, w, 8), np.float32)
            with np.errstate(all="ignore"):
                for i in range(3):
                    rec[..., i] = _dot(m[4 * i:4 * i + 3], P) + m[4 * i + 3]
                    rec[..., 4 + i] = _dot(m[12 + 4 * i:15 + 4 * i], n)
            kind = (fr["ids"][..., 0] == 1).astype(np.uint32)
            rec[kind == 0] = 0
            flat, kf = rec.reshape(-1, 8), kind.reshape(-1)
            npx = w * h
            for i in rng.choice(npx, max(npx // 12, 1), replace=False):
                case = rng.randint(5)
                if case == 0:                            # moved, to somewhere else
                    flat[i, :3] = P.reshape(-1, 3)[i] + rng.normal(0, 0.05, 3).astype(np.float32)
                    flat[i, 4:7] = n.reshape(-1, 3)[i]
                    kf[i] = 1
                elif case == 1:                          # moved, a word not finite
                    flat[i, rng.choice([0, 1, 2, 4, 5, 6])] = rng.choice([np.nan, np.inf, -np.inf])
                    kf[i] = 1
                elif case == 2:                          # static, garbage words
                    flat[i] = rng.normal(0, 3, 8)
                    flat[i, 1] = np.nan
                    kf[i] = 0
                elif case == 3:                          # kind 2 is not 1
                    flat[i] = rng.normal(0, 3, 8)
                    kf[i] = 2
                else:                                    # 1.0f is not the integer 1
                    kf[i] = 0x3f800000
            rec.view(np.uint32)[..., 3] = kind
            rec.setflags(write=False)
            out.append(rec)
        _records[(w, h)] = out
    return _records[(w, h)]


_accumulated = {}


def accumulated(w, h, demodulate, moments, with_records=True):
    """the NumPy statement over the `mixed` sequence with the records -> [(frame, variance, length)] per frame, computed once"""
    from yart_amd.temporal import TemporalHistory
    key = (w, h, demodulate, moments, with_records)
    if key not in _accumulated:
        hist, prm = TemporalHistory(w, h), tm.params_of(moments)
        fn = statement_pm
        _accumulated[key] = [fn(hist, f, demodulate, moments, prm, r if with_records else None)
                             for f, r in zip(tm.frames_of(w, h, "mixed"), records_of(w, h))]
    return _accumulated[key]


def statement_pm(hist, f, demodulate, moments, prm, records):
    from yart_amd.temporal import temporal_moments_reference, temporal_reference
    fn = temporal_moments_reference if moments else temporal_reference
    r = fn(hist, f["camera"], f["rgba"], f["variance"], f["position"], f["normal"], f["depth"], f["coverage"], f["ids"],
           f["albedo"] if demodulate else None, demodulate=demodulate, pixel_motion=records, **prm)
    for v in r:
        v.setflags(write=False)
    return r


def run_temporal_sim(exe, tmp, frames, records, demodulate, moments, in_place):
    """tests/test_temporal_motion.run_sim with this module's program (its temporal mode): a frame's motion is its w * h records"""
    return tm.run_sim(exe, tmp, frames, [None if r is None else r.reshape(-1, 8) for r in records], demodulate, moments, in_place)


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_accumulate_equals_the_numpy_statement_on_bits(sim, tmp_path, w, h):
    """csrc/temporal.hpp on the host, with a per-pixel Motion, == the NumPy statement with pixel_motion=, bit for bit: the `mixed`
    sequence of test_temporal_motion (seeded random buffers with non-finite entries, a moving camera) at its PARAMS with
    records_of's records (non-finite words among them), both forms, demodulation on and off, out of place and in place, every
    frame. From 37 x 23 on the records matter: the last frame differs from the one without them."""
    frames, records = tm.frames_of(w, h, "mixed"), records_of(w, h)
    for moments in (False, True):
        for dm in (False, True):
            want = accumulated(w, h, dm, moments)
            for in_place in (False, True):
                got = run_temporal_sim(sim, str(tmp_path), frames, records, dm, moments, in_place)
                for k in range(FRAMES):
                    assert_same(got[k], want[k], f"{w}x{h} moments {moments} demodulate {dm} in_place {in_place} frame {k}")
            if w * h > 100:
                without = accumulated(w, h, dm, moments, with_records=False)
                assert (bits(want[-1][0]) != bits(without[-1][0])).any() and (want[-1][2] != without[-1][2]).any()


@pytest.mark.parametrize("moments", [False, True])
def test_kind_0_pixels_give_the_bits_of_a_run_without_a_motion(sim, tmp_path, moments):
    """Records whose kind is not 1 — 0, 2, the bits of 1.0f — with arbitrary other words, NaN among them, give the bits of
    pixel_motion=None on the `mixed` sequence at 37 x 23: the NumPy statement against its own result without a motion, and the host
    statement against that."""
    from yart_amd.temporal import TemporalHistory
    w, h = 37, 23
    rng = np.random.RandomState(3)
    frames = tm.frames_of(w, h, "mixed")
    records = []
    for k in range(FRAMES):
        rec = rng.normal(0, 3, (h, w, 8)).astype(np.float32)
        rec[rng.rand(h, w) < 0.2, 0] = np.nan
        rec.view(np.uint32)[..., 3] = rng.choice(np.array([0, 0, 2, 0x3f800000, 0xffffffff], np.uint32), (h, w))
        records.append(rec)
    prm = tm.params_of(moments)
    for dm in (False, True):
        want = accumulated(w, h, dm, moments, with_records=False)
        assert (want[-1][2] > 1).mean() > 0.1
        hist = TemporalHistory(w, h)
        for k, f in enumerate(frames):
            assert_same(statement_pm(hist, f, dm, moments, prm, records[k]), want[k], f"numpy demodulate {dm} frame {k}")
        got = run_temporal_sim(sim, str(tmp_path), frames, records, dm, moments, False)
        for k in range(FRAMES):
            assert_same(got[k], want[k], f"host demodulate {dm} frame {k}")


def test_one_motion_at_a_time():
    from yart_amd.temporal import TemporalHistory, temporal_reference
    w, h = 5, 3
    f = tm.frames_of(w, h, "mixed")[1]
    with pytest.raises(AssertionError, match="one motion"):
        temporal_reference(TemporalHistory(w, h), f["camera"], f["rgba"], f["variance"], f["position"], f["normal"], f["depth"],
                           f["coverage"], f["ids"], motion=f["motion"], pixel_motion=records_of(w, h)[1])


def test_a_rigid_scene_agrees_with_the_per_node_path():
    """test_temporal_motion's three-node scene and its `inplane`, `normal` and `turn` moves at 37 x 23 and 131 x 67, frames 1 .. 3.
    Node 1 carries the sheet's 8 x 8-cell grid here, scaled to cover what the camera sees of its plane (out to 2.5, and to 6 when
    the plane is turned) — triangles a quarter of the range wide, as the feature conditions' are: the barycentric step's rounding
    error grows with the triangle's edge, and a single triangle as wide as the whole range is no mesh this is for.
    Where node_motion says `moving`, the per-pixel record is kind 1 and its P' is node_motion's M P within 4 ulp of the coordinate
    range — the largest |coordinate| among P, P' and the grid's vertices — (bit equality is not required: node_motion inverts the
    composed matrix, the per-pixel path composes the nodes' own inverses and goes through the triangle's plane), n' within 1e-5;
    where it says static the record is all zero.
    Measured: the largest |P' - M P| is 1.50 ulp of the range (3.6e-7 at a range of 2.5; 5.2e-7 = 1.09 ulp at 6); n' equals Nm n."""
    from yart_amd.scene_motion import scene_motion_reference
    from yart_amd.temporal import _dot
    rest, faces = sheet_rest()
    worst_p = worst_n = 0.0
    for w, h in FEATURE_SIZES:
        for seq in ("inplane", "normal", "turn"):
            fr = tm.frames_of(w, h, seq)
            big = 6.0 if seq == "turn" else 2.5          # the turned plane is seen out to |x_obj| = 5.3, the others to 1.9
            quad = (rest * (big / EXTENT)).astype(np.float32)
            cell = 2.0 * big / CELLS
            for k in range(1, FRAMES):
                f, prev = fr[k], fr[k - 1]
                P, n = f["position"], f["normal"]
                # which triangle of the quad a point of node 1 lies in: below or above the diagonal of its object space
                obj = (P.astype(np.float64) - np.asarray(f["nodes"][1].fwd, np.float64)[:3, 3]) @ np.asarray(f["nodes"][1].fwd, np.float64)[:3, :3]
                ids = f["ids"].copy()
                g = (obj[..., :2] + big) / cell
                ci = np.clip(np.floor(g).astype(np.int64), 0, CELLS - 1)
                upper = (g[..., 1] - ci[..., 1]) > (g[..., 0] - ci[..., 0])        # (a, b, c) lies below the cell's diagonal, (a, c, d) above
                ids[..., 3] = 2 * (ci[..., 1] * CELLS + ci[..., 0]) + np.where(upper, 1, 0)
                assert np.abs(obj[f["ids"][..., 0] == 1][:, :2]).max() < big
                rec = scene_motion_reference(prev["nodes"], f["nodes"], [faces, faces], [quad, quad], [quad, quad], P, n, f["coverage"], ids)
                m = f["motion"][1]
                moving = f["ids"][..., 0] == 1
                assert np.array_equal(kinds(rec) == 1, moving) and not bits(rec)[~moving].any()
                want_p = np.stack([_dot(m[4 * i:4 * i + 3], P) + m[4 * i + 3] for i in range(3)], -1)
                want_n = np.stack([_dot(m[12 + 4 * i:15 + 4 * i], n) for i in range(3)], -1)
                scale = max(float(np.abs(want_p[moving]).max()), float(np.abs(P[moving]).max()), big)
                ulp = float(np.spacing(np.float32(scale)))
                err_p = float(np.abs(rec[..., :3].astype(np.float64) - want_p)[moving].max())
                err_n = float(np.abs(rec[..., 4:7].astype(np.float64) - want_n)[moving].max())
                print(f"{w}x{h} {seq} frame {k}: |P' - M P| <= {err_p:.2e} = {err_p / ulp:.2f} ulp of {scale:.2f}; |n' - Nm n| <= {err_n:.2e}")
                assert err_p <= 4 * ulp, (seq, k, err_p, ulp)
                assert err_n <= 1e-5, (seq, k, err_n)
                worst_p, worst_n = max(worst_p, err_p / ulp), max(worst_n, err_n)
    print(f"largest: {worst_p:.2f} ulp, {worst_n:.2e}")


# -- the feature conditions --------------------------------------------------------------------------------------------
def sheet_rest():
    """rest positions (81, 3) float64 and faces (128, 3) of the sheet: vertex (i, j) at (-3.2 + 0.8 i, -3.2 + 0.8 j, 0), per cell
    the triangles (a, b, c) and (a, c, d), counter-clockwise seen from +z"""
    g = np.linspace(-EXTENT, EXTENT, CELLS + 1)
    X, Y = np.meshgrid(g, g, indexing="xy")
    rest = np.stack([X, Y, np.zeros_like(X)], -1).reshape(-1, 3)
    idx = np.arange((CELLS + 1) ** 2).reshape(CELLS + 1, CELLS + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:], idx[1:, :-1]
    faces = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], -2).reshape(-1, 3)
    return rest, faces


def sheet_vertices(seq, k):
    """the sheet's vertices of frame k, rounded to binary32"""
    rest, _ = sheet_rest()
    x, y = rest[:, 0], rest[:, 1]
    s = x / EXTENT
    p = rest.copy()
    if seq == "stretch":
        p[:, 0] = x + 0.25 * k * (1.0 - s * s) * (1.0 + 0.5 * y / EXTENT)
    elif seq == "wave":
        p[:, 2] = 0.25 * k * np.cos(1.3 * s) * (1.0 + 0.3 * y / EXTENT)
    else:
        assert seq == "both"
        p[:, 0] = x + 0.25 * k * (1.0 - s * s)
        p[:, 2] = 0.25 * k * np.cos(1.3 * s)
    return p.astype(np.float32)


def sheet_nodes():
    from yart_amd.yscn import Node, trs
    return [Node(-1, -1), Node(0, 0, *trs(translation=(0.0, 0.0, 1.0)))]


def sheet_see(cam, verts):
    """what every pixel centre sees of the sheet (vertices in object space, the node translates by (0, 0, 1)): t, triangle, P, the
    flat normal and the rest coordinates of the hit point, float64; every pixel hits"""
    w, h = cam["size"]
    rest, faces = sheet_rest()
    eye, tl, du, dv = tt.camera64(cam)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = (tl + xs[..., None] * du + ys[..., None] * dv - eye).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    v = verts.astype(np.float64) + np.array([0.0, 0.0, 1.0])
    a, e1, e2 = v[faces[:, 0]], v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    with np.errstate(all="ignore"):                      # Moeller-Trumbore, rays x triangles
        pv = np.cross(d[:, None, :], e2[None])
        det = (e1[None] * pv).sum(-1)
        tv = eye - a
        bu = (tv[None] * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        bv = (d[:, None, :] * qv[None]).sum(-1) / det
        t = (e2 * qv).sum(-1)[None] / det
        hit = (bu >= -1e-12) & (bv >= -1e-12) & (bu + bv <= 1 + 1e-12) & (t > 0) & np.isfinite(t)
        t = np.where(hit, t, np.inf)
    tri = t.argmin(1)
    r = np.arange(len(d))
    best = t[r, tri]
    assert np.isfinite(best).all()
    P = eye + best[:, None] * d
    nrm = np.cross(e1[tri], e2[tri])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    ra = rest[faces[tri, 0]]
    uv = ra + bu[r, tri][:, None] * (rest[faces[tri, 1]] - ra) + bv[r, tri][:, None] * (rest[faces[tri, 2]] - ra)
    shape = (h, w)
    return best.reshape(shape), tri.reshape(shape), P.reshape(h, w, 3), nrm.reshape(h, w, 3), uv[:, :2].reshape(h, w, 2)


_sheet = {}


def sheet_sequence(w, h, seq):
    """-> per frame dict(camera, rgba, variance, position, normal, depth, coverage, ids, records (None in frame 0)), and the last
    frames of the statement at the default parameters with the records and without them"""
    from yart_amd.scene_motion import scene_motion_reference
    from yart_amd.temporal import TemporalHistory, temporal_reference
    if (w, h, seq) not in _sheet:
        cam = tm.base_camera(w, h)
        _, faces = sheet_rest()
        nodes = sheet_nodes()
        frames, prev = [], None
        for k in range(FRAMES):
            verts = sheet_vertices(seq, k)
            t, tri, P, nrm, uv = sheet_see(cam, verts)
            rgba = np.ones((h, w, 4), np.float32)
            rgba[..., :3] = tm.COLOUR[:, 0] + uv[..., :1] * tm.COLOUR[:, 1] + uv[..., 1:] * tm.COLOUR[:, 2]
            ids = np.stack([np.ones_like(tri), np.zeros_like(tri), np.zeros_like(tri), tri], -1).astype(np.int32)
            f = dict(camera=cam, rgba=rgba, variance=np.zeros((h, w), np.float32), position=P.astype(np.float32),
                     normal=nrm.astype(np.float32), depth=t.astype(np.float32), coverage=np.ones((h, w), np.float32), ids=ids, records=None)
            if prev is not None:
                f["records"] = scene_motion_reference(nodes, nodes, [faces], [prev], [verts], f["position"], f["normal"], f["coverage"], ids)
            prev = verts
            frames.append(f)
        last = []
        for with_records in (True, False):
            hist = TemporalHistory(w, h)
            for f in frames:
                r = temporal_reference(hist, f["camera"], f["rgba"], f["variance"], f["position"], f["normal"], f["depth"], f["coverage"],
                                       f["ids"], pixel_motion=f["records"] if with_records else None)
            last.append(r)
        _sheet[(w, h, seq)] = (frames, last[0], last[1])
    return _sheet[(w, h, seq)]


def inner(w, h):
    m = np.zeros((h, w), bool)
    m[4:h - 4, 4:w - 4] = True
    return m


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_a_sheet_stretching_in_its_plane_does_not_ghost(w, h):
    """`stretch`, default parameters, the inner pixels (the image eroded by 4 pixels) of frame 3, errors relative to the colour
    range of that frame: with the records the largest error is at most 0.5 % and no inner pixel has length 1; without them the mean
    error is at least 3 % — another point's history, silently.
    This statement gives: with the records max 0.0008 (37 x 23) and 0.0015 (131 x 67); without them mean 0.049 and 0.049, max
    0.064 and 0.068."""
    frames, with_, without = sheet_sequence(w, h, "stretch")
    c = frames[-1]["rgba"][..., :3].astype(np.float64)
    rng_c = c.max() - c.min()
    m = inner(w, h)
    assert (kinds(frames[-1]["records"]) == 1).all()
    err = [np.abs(r[0][..., :3].astype(np.float64) - c).max(-1)[m] / rng_c for r in (with_, without)]
    print(f"stretch {w}x{h}: with the records max {err[0].max():.4f}; without mean {err[1].mean():.4f} max {err[1].max():.4f}; "
          f"length 1 with the records at {(with_[2][m] == 1).sum()} of {m.sum()} inner pixels")
    assert err[0].max() <= 0.005
    assert not (with_[2][m] == 1).any()
    assert err[1].mean() >= 0.03


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_a_sheet_waving_out_of_its_plane_keeps_its_history(w, h):
    """`wave`, default parameters, the inner pixels of frame 3: length 4 on at least 95 % of them with the records, length 1 on all
    of them without (the plane test rejects every tap).
    This statement gives 100 % and 100 % at both sizes."""
    frames, with_, without = sheet_sequence(w, h, "wave")
    m = inner(w, h)
    share, share0 = (with_[2][m] == 4).mean(), (without[2][m] == 1).mean()
    print(f"wave {w}x{h}: length 4 with the records at {share:.4f}, length 1 without at {share0:.4f} of {m.sum()} inner pixels")
    assert share >= 0.95
    assert share0 == 1.0


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_a_sheet_doing_both_keeps_its_history(w, h):
    """`both`, default parameters, the inner pixels of frame 3: length 4 on at least 90 % with the records; length 1 on all without.
    This statement gives 100 % (37 x 23) and 97.6 % (131 x 67) with the records, 100 % without."""
    frames, with_, without = sheet_sequence(w, h, "both")
    m = inner(w, h)
    share, share0 = (with_[2][m] == 4).mean(), (without[2][m] == 1).mean()
    print(f"both {w}x{h}: length 4 with the records at {share:.4f}, length 1 without at {share0:.4f} of {m.sum()} inner pixels")
    assert share >= 0.90
    assert share0 == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


PM_AOVS = ("position", "normal", "coverage", "ids")


def device_state(scene, n_meshes):
    """the scene's own node array and vertex positions, read back"""
    nodes, _, _ = scene.scene_graph()
    return nodes, [scene.mesh_records(m)["positions"] for m in range(n_meshes)]


def animate(api, w, h, order, spp=4):
    """The mixed scene created at frame 0 and rendered, keep_previous, update and update_meshes in `order`, rendered again ->
    (scene, the second frame's feature buffers, the statement's records from the device's own node arrays, positions and buffers)"""
    from yart_amd.scene_motion import scene_motion_reference
    s0, s1, p = mixed_scene(0), mixed_scene(1), mixed_params(w, h, spp)
    scene = api.DeviceScene(s0, device=0)
    scene.render_aovs(p, PM_AOVS)
    before = device_state(scene, len(s0.meshes))
    scene.keep_previous()
    steps = {"nodes": lambda: scene.update(s1.nodes), "meshes": lambda: scene.update_meshes({1: s1.meshes[1].positions, 2: s1.meshes[2].positions})}
    for step in order:
        steps[step]()
    after = device_state(scene, len(s0.meshes))
    _, buf, _ = scene.render_aovs(p, PM_AOVS)
    want = scene_motion_reference(before[0], after[0], s1.meshes, before[1], after[1], buf["position"], buf["normal"], buf["coverage"], buf["ids"])
    return scene, buf, want


def assert_same_records(got, want, tag):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{tag}: {int(diff.sum())} words differ, first at {np.argwhere(diff)[0].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_pixel_motion_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_sm_node_chains and k_sm_pixels through DeviceScene.pixel_motion (the host entry) == scene_motion_reference fed the device's
    own node arrays, vertex positions and feature buffers (4 spp), bit for bit, with update and update_meshes in both orders; from
    37 x 23 on all five mesh nodes are seen, static and moved records both occur, and some pixels miss everything."""
    for order in (("nodes", "meshes"), ("meshes", "nodes")):
        scene, buf, want = animate(gpu_api, w, h, order)
        got = scene.pixel_motion(buf)
        scene.close()
        assert got.shape == (h, w, 8) and got.dtype == np.float32
        assert_same_records(got, want, f"pixel_motion {w}x{h} {order}")
        if w * h > 100:
            node, kind = buf["ids"][..., 0], kinds(want)
            assert {-1, 1, 3, 4, 5} <= set(np.unique(node).tolist())
            assert not kind[node == 1].any() and not kind[node == -1].any()
            full = buf["coverage"] == 1.0
            assert kind[full & (node == 3)].all() and kind[full & (node == 5)].all() and kind[full & (node == 4)].any()
            assert (kind == 1).mean() > 0.1 and (kind == 0).mean() > 0.1


@pytest.mark.gpu
def test_device_refusals(gpu_api):
    """A scene on which keep_previous was never called is refused with YART_E_INVALID by both entries; after keep_previous and no
    update every record is static."""
    api = gpu_api
    w, h = 37, 23
    scene = api.DeviceScene(mixed_scene(0), device=0)
    _, buf, _ = scene.render_aovs(mixed_params(w, h), PM_AOVS)
    with pytest.raises(api.YartError, match="keep_previous"):
        scene.pixel_motion(buf)
    scene.keep_previous()
    assert not bits(scene.pixel_motion(buf)).any()
    scene.close()


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_pixel_motion as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_into():
    import torch
    from yart_amd import api
    # pixel_motion_into on a non-default stream == the host entry == the statement
    for w, h in GPU_SIZES:
        scene, buf, want = animate(api, w, h, ("nodes", "meshes"))
        host = scene.pixel_motion(buf)
        t = {name: torch.from_numpy(buf[name].copy()).cuda() for name in buf}
        rec = torch.full((h, w, 8), 7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            scene.pixel_motion_into(rec, t)
        got = rec.cpu().numpy()
        scene.close()
        assert_same_records(host, want, f"host entry {w}x{h}")
        assert got.tobytes() == host.tobytes(), f"pixel_motion_into {w}x{h}"
        for name in t:
            assert np.array_equal(bits(t[name].cpu().numpy()), bits(buf[name])), name + " was written"
    # accumulate_into(pixel_motion=a device tensor) == the statement
    for w, h in GPU_SIZES:
        for moments in (False, True):
            dm = moments
            want = accumulated(w, h, dm, moments)
            dev = tm.accumulator(api, w, h, moments)
            side = torch.cuda.Stream()
            for k, (fr, rec) in enumerate(zip(tm.frames_of(w, h, "mixed"), records_of(w, h))):
                t = {name: torch.from_numpy(fr[name].copy()).cuda() for name in fr if isinstance(fr[name], np.ndarray) and name != "motion"}
                rt = None if rec is None else torch.from_numpy(rec.copy()).cuda()
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    out, var = torch.zeros_like(t["rgba"]), torch.zeros_like(t["variance"])
                    ln = torch.zeros((h, w), dtype=torch.int32, device="cuda")
                    dev.accumulate_into(out, var, ln, fr["camera"], t["rgba"], t["variance"], tm.aovs_of(t, dm), demodulate=dm, pixel_motion=rt)
                    got = (out.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy().view(np.uint32))
                assert_same(got, want[k], f"accumulate_into {w}x{h} moments {moments} frame {k}")
                if rt is not None:
                    assert np.array_equal(bits(rt.cpu().numpy()), bits(rec)), "the records were written"
            dev.close()


@pytest.mark.gpu
def test_device_entries_on_torch_tensors(gpu_api):
    """In a fresh child process, on a non-default stream: DeviceScene.pixel_motion_into gives the bytes of the host entry, which are
    the statement's, at every size; TemporalAccumulator.accumulate_into(pixel_motion=device tensor) gives the statement's bits over
    the four-frame `mixed` sequence in both forms; inputs and records are not written."""
    run_torch_child("child_into()")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_accumulate_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_tp_accumulate<., true, true> through api.TemporalAccumulator.accumulate(pixel_motion=) — the host entries — == the NumPy
    statement, bit for bit: frame, variance and length of all four frames of the `mixed` sequence, both forms, demodulation on and
    off, and with the outputs aliasing the inputs."""
    for moments in (False, True):
        for dm, in_place in ((False, False), (True, False), (True, True)):
            want = accumulated(w, h, dm, moments)
            acc = tm.accumulator(gpu_api, w, h, moments)
            for k, (fr, rec) in enumerate(zip(tm.frames_of(w, h, "mixed"), records_of(w, h))):
                got = tm.device_frame(acc, fr, dm, in_place, pixel_motion=rec)
                assert_same(got, want[k], f"pixel motion {w}x{h} moments {moments} demodulate {dm} in_place {in_place} frame {k}")
            acc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [False, True])
def test_the_pixel_motion_is_consumed(gpu_api, moments):
    """`mixed` at 37 x 23: frame 1 is accumulated with its records, frame 2 without a setter call: frame 2 equals the statement with
    pixel_motion=None for it, and not the one with frame 2's records. One motion is pending at a time: set_motion then
    set_pixel_motion runs with the records alone, set_pixel_motion then set_motion with the per-node motion alone. reset and
    set_pixel_motion(None) clear; a refused accumulate call does not consume."""
    from yart_amd.temporal import TemporalHistory
    api = gpu_api
    w, h = 37, 23
    fr, rec = tm.frames_of(w, h, "mixed"), records_of(w, h)
    prm = tm.params_of(moments)

    def states(motions, start=0):
        """motions: per frame None, ("pixel", records) or ("node", records)"""
        hist = TemporalHistory(w, h)
        out = []
        for f, m in zip(fr[start:], motions):
            if m is not None and m[0] == "node":
                out.append(tm.statement(hist, f, False, moments, prm, m[1]))
            else:
                out.append(statement_pm(hist, f, False, moments, prm, None if m is None else m[1]))
        return out
    want = states([None, ("pixel", rec[1]), None])
    assert (bits(want[2][0]) != bits(states([None, ("pixel", rec[1]), ("pixel", rec[2])])[2][0])).any()
    acc = tm.accumulator(api, w, h, moments)
    tm.device_frame(acc, fr[0], False)
    assert_same(tm.device_frame(acc, fr[1], False, pixel_motion=rec[1]), want[1], "frame 1, with its records")
    assert_same(tm.device_frame(acc, fr[2], False), want[2], "frame 2, no setter call")
    # the later setter replaces the earlier one, both ways
    with_pixel, with_node = states([None, ("pixel", rec[2])], start=1)[1], states([None, ("node", fr[2]["motion"])], start=1)[1]
    assert (bits(with_pixel[0]) != bits(with_node[0])).any()
    for first, want2 in (("node", with_pixel), ("pixel", with_node)):
        acc.reset()
        tm.device_frame(acc, fr[1], False)
        keep = rec[2].copy()
        if first == "node":
            acc.set_motion(fr[2]["motion"])
            acc.set_pixel_motion(keep)
        else:
            acc.set_pixel_motion(keep)
            acc.set_motion(fr[2]["motion"])
        assert_same(tm.device_frame(acc, fr[2], False), want2, f"{first} first")
    # set, then reset / cleared with None: the next frames have no motion
    plain = states([None, None], start=1)
    assert (bits(plain[1][0]) != bits(with_pixel[0])).any()
    keep = rec[2].copy()
    acc.set_pixel_motion(keep)
    acc.reset()
    assert_same(tm.device_frame(acc, fr[1], False), plain[0], "first frame after the reset")
    assert_same(tm.device_frame(acc, fr[2], False), plain[1], "second frame after the reset")
    acc.reset()
    tm.device_frame(acc, fr[1], False)
    acc.set_pixel_motion(keep)
    acc.set_pixel_motion(None)
    assert_same(tm.device_frame(acc, fr[2], False), plain[1], "after set_pixel_motion(None)")
    # a refused accumulate call does not consume
    acc.reset()
    tm.device_frame(acc, fr[1], False)
    acc.set_pixel_motion(keep)
    with pytest.raises(api.YartError, match="alpha_min"):
        tm.device_frame(acc, fr[2], False, alpha_min=2.0)
    assert_same(tm.device_frame(acc, fr[2], False), with_pixel, "after a refused accumulate call")
    acc.close()


def wave_normals(k):
    """the `wave` surface's unit normals at the sheet's vertices: (-dz/dx, -dz/dy, 1) normalised"""
    rest, _ = sheet_rest()
    s, y = rest[:, 0] / EXTENT, rest[:, 1]
    dzdx = -0.25 * k * (1.3 / EXTENT) * np.sin(1.3 * s) * (1.0 + 0.3 * y / EXTENT)
    dzdy = 0.25 * k * np.cos(1.3 * s) * (0.3 / EXTENT)
    n = np.stack([-dzdx, -dzdy, np.ones_like(s)], -1)
    return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)


def sheet_scene(seq, k):
    from yart_amd.yscn import LIGHT_UNIFORM_INF, Light, Material, Mesh, Scene, trs
    _, faces = sheet_rest()
    v = sheet_vertices(seq, k)
    s = Scene()
    mat = s.add_material(Material(base=(0.7, 0.7, 0.7), roughness=1.0))
    f4 = np.concatenate([faces.astype(np.uint32), np.full((len(faces), 1), mat, np.uint32)], 1)
    s.add_mesh(Mesh(v, np.broadcast_to(np.array([0.0, 0.0, 1.0], np.float32), v.shape).copy(), None, np.zeros((len(v), 2), np.float32), f4))
    s.add_node(0, 0, *trs(translation=(0.0, 0.0, 1.0)))
    s.lights.append(Light(LIGHT_UNIFORM_INF, radius=100.0, emission=(1.0, 1.0, 1.0)))
    return s


def child_end_to_end():
    from yart_amd import api
    w, h = 37, 23
    p = dict(mixed_params(w, h, spp=1), depth=3)
    m = inner(w, h)
    lengths = {}
    for flag in (True, False):
        scene = api.DeviceScene(sheet_scene("wave", 0), device=0)
        acc = api.TemporalAccumulator(w, h, device=0)
        for k in range(FRAMES):
            if k:
                scene.keep_previous()
                scene.update_meshes({0: (sheet_vertices("wave", k), wave_normals(k))})
            _, _, g = scene.render_denoised(p, temporal=acc, pixel_motion=flag and k > 0)
            assert ("pixel_motion" in g) == (flag and k > 0)
        lengths[flag] = g["length"].cpu().numpy().view(np.uint32)
        if flag:
            assert (g["pixel_motion"].cpu().numpy().view(np.uint32)[..., 3][m] == 1).all()
        acc.close()
        scene.close()
    share, share0 = (lengths[True][m] == 4).mean(), (lengths[False][m] == 1).mean()
    print(f"end to end: length 4 with pixel_motion=True at {share:.4f}, length 1 without at {share0:.4f} of {m.sum()} inner pixels")
    assert share >= 0.95 and share0 == 1.0
    try:
        scene = api.DeviceScene(sheet_scene("wave", 0), device=0)
        scene.render_denoised(p, temporal=api.TemporalAccumulator(w, h, device=0), motion=np.zeros((2, 24), np.float32), pixel_motion=True)
    except AssertionError:
        pass
    else:
        raise SystemExit("motion= together with pixel_motion=True was not refused")


@pytest.mark.gpu
def test_render_denoised_with_pixel_motion(gpu_api):
    """End to end: the `wave` sheet rendered by the path tracer under a uniform environment light at 1 spp and 37 x 23, four frames,
    the scene deformed in place (keep_previous, update_meshes); DeviceScene.render_denoised(temporal=acc, pixel_motion=True) reaches
    length 4 on at least 95 % of the inner pixels, the same sequence without the flag stays at length 1 on all of them (the length
    depends on the geometry buffers only: noise does not enter). motion= together with pixel_motion=True is refused."""
    run_torch_child("child_end_to_end()")
