"""Scene graphs nested to any depth (the reference's testNode and processNode recurse without a limit:
src/cpu/ray-integrator.cpp:20-54, src/gltf/gltf.cpp:272-317).

Depth counts levels with the root at depth 0: a 9-level graph has a node at depth 8, the first depth at which the node walk
applies a chain in more than one window (traverse.hpp::objectRay) and a node has no world-space pre-cull box
(host_scene.hpp). Every frame is compared with the compiled reference bit for bit.

CPU: the device headers on the host (tests/hostsim, and hostsim_lean with the lean kernels' hand-over logic) on chains and
trees of 9 to 64 levels; the reference's known-answer vectors on the ill-conditioned 24-level graph; a harness that checks
the world-space pre-cull against the exact object-space test on random and edge-aimed rays; the glTF importer on a
40-level TRS chain (node and light transforms against the reference's float4x4 algebra), a 700-level chain, a cycle and a
shared child; the Python scene model on a 3000-level chain.
GPU: the same scenes through every pipeline, a long chain, a deep glTF asset, tiled / progressive renders and a seeded fuzz
of deep graphs."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import gltf_assets as ga
from tests.conftest import REF_BIN, bit_identical_or_drift

needs_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/yart_ref not built here")

# (depth, branching, pad_nodes, ill_conditioned): chains and trees; (24, 3) has 111 nodes, (64, 2, 70) 258
CPU_CASES = [(9, 1, 0, True), (9, 2, 0, False), (12, 1, 0, True), (12, 3, 0, False), (24, 1, 0, True), (24, 3, 0, True),
             (24, 1, 0, False), (64, 1, 0, True), (64, 2, 70, False)]


def _deep(depth, branching=1, pad=0, ill=True, **kw):
    from yart_amd import scenes
    return scenes.deep_instances(depth, branching, pad_nodes=pad, ill_conditioned=ill, **kw)


def _reference(tmp_path, s, p, tag="s", **params):
    from yart_amd import scenes
    sp, pp, ref = str(tmp_path / f"{tag}.yscn"), str(tmp_path / f"{tag}.txt"), str(tmp_path / f"{tag}.ref.f32")
    s.save(sp)
    scenes.write_params(pp, p, threads=1, **params)
    subprocess.run([REF_BIN, "render", sp, pp, ref], check=True, capture_output=True, text=True)
    return sp, pp, np.fromfile(ref, np.uint32)


def _depths(s):
    d = [0] * len(s.nodes)
    for i, n in enumerate(s.nodes):
        if n.parent >= 0:
            d[i] = d[n.parent] + 1
    return d


def test_deep_instances_shapes():
    """The generator builds what the tests assume: `depth` levels, pre-order, area lights under deep chains."""
    for depth, branching, pad, ill in CPU_CASES:
        s, _ = _deep(depth, branching, pad, ill)
        d = _depths(s)
        assert max(d) == depth - 1, (depth, branching)
        assert all(0 <= n.parent < i for i, n in enumerate(s.nodes) if i), "pre-order"
        lit = {l.mesh for l in s.lights if l.type == 0}
        assert any(d[i] >= 8 and n.mesh in lit for i, n in enumerate(s.nodes)), "an area light below depth 8"
    assert len(_deep(24, 3)[0].nodes) > 64 and len(_deep(64, 2, 70)[0].nodes) > 64


@needs_ref
@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: f"d{c[0]}b{c[1]}p{c[2]}{'ill' if c[3] else 'trs'}")
def test_deep_graphs_on_host(hostsim, hostsim_lean, tmp_path, case):
    s, p = _deep(*case, width=40, height=32, spp=4)
    sp, pp, ref = _reference(tmp_path, s, p)
    got = str(tmp_path / "got.f32")
    for exe in (hostsim, hostsim_lean):
        r = subprocess.run([exe, "render", sp, pp, got], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        assert "differs" not in r.stderr, f"{case}: the lean walk kept a ray the general walk treats differently\n{r.stderr[:2000]}"
        g = np.fromfile(got, np.uint32)
        assert np.array_equal(ref, g), f"{case} / {os.path.basename(exe)}: {(ref != g).sum()} words differ"
    assert np.any(ref.view(np.float32).reshape(-1, 4)[:, :3] > 0)


@needs_ref
def test_deep_graph_known_answers(hostsim, tmp_path):
    """Hit records and per-sample radiance of probe pixels on the ill-conditioned 24-level chain: every vector equal."""
    from yart_amd import scenes
    from tests import katlib
    s, p = _deep(24, 1, 0, True, width=48, height=48, spp=4)
    rng = np.random.RandomState(24)
    probes = [(int(rng.randint(14, 34)), int(rng.randint(14, 34))) for _ in range(6)]
    sp, pp = str(tmp_path / "s.yscn"), str(tmp_path / "p.txt")
    s.save(sp); scenes.write_params(pp, p, threads=1, probe_pixels=probes)
    kats = {}
    for name, exe in (("ref", REF_BIN), ("device headers", hostsim)):
        out = str(tmp_path / (name.split()[0] + ".json"))
        subprocess.run([exe, "kat", sp, pp, out], check=True, stdout=subprocess.DEVNULL)
        kats[name] = katlib.load(out)
    res = katlib.compare(kats["ref"], kats["device headers"], [k for k in kats["ref"] if k != "ggxGlassEavg"])
    bad = {k: v for k, v in res.items() if v["mismatches"]}
    assert not bad, bad


# The world-space pre-cull (host_scene.hpp: padded nodeWorld boxes, tested before the reference's object-space test by
# traverseScene and the lean walks) may only skip what the exact test skips. The harness draws rays (origins around the
# scene's geometry, directions at random or aimed at corners / edge points of a node's box mapped to world space, tMax at random,
# some just short of / past the aimed point) and checks: every (ray, node) the exact per-level test accepts, the padded
# world box accepts too.
PRECULL_HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
#include "host_scene.hpp"
#include "scene_file.hpp"
#include "traverse.hpp"
using namespace yart_hip;
int main(int argc, char** argv) {
  auto loaded = loadSceneFile(argv[1]);
  HostImage im = buildHostImage(loaded->desc);
  const SceneDev sc = im.view();
  const uint64_t nRays = std::strtoull(argv[2], nullptr, 10);
  std::mt19937_64 rng(std::strtoull(argv[3], nullptr, 10));
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  // ray origins: around the scene's geometry (the finite world boxes of its leaf mesh nodes), where cameras and the surfaces
  // rays leave from are (an inner node's box can be far larger: bounds of rotated bounds grow with every level, as the
  // reference's do)
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (uint32_t i = 0; i < sc.nNodes; i++) {
    const f4 a = sc.nodeWorld[2u * i], b = sc.nodeWorld[2u * i + 1u];
    if (sc.nodes[i].mesh < 0 || sc.nodes[i].skip != i + 1u || !std::isfinite(a.x)) continue;
    lo[0] = std::min(lo[0], double(a.x)); lo[1] = std::min(lo[1], double(a.y)); lo[2] = std::min(lo[2], double(a.z));
    hi[0] = std::max(hi[0], double(b.x)); hi[1] = std::max(hi[1], double(b.y)); hi[2] = std::max(hi[2], double(b.z));
  }
  for (int c = 0; c < 3; c++) { const double e = hi[c] - lo[c]; lo[c] -= 0.5 * e; hi[c] += 0.5 * e; }
  uint64_t pairs = 0, exact = 0, deepExact = 0, shallowExact = 0, bad = 0;
  for (uint64_t r = 0; r < nRays; r++) {
    const uint32_t i = 1u + uint32_t(U(rng) * (sc.nNodes - 1)) % (sc.nNodes - 1);
    const NodeDev& nd = sc.nodes[i];
    if (nd.pad[0] & 1u) continue;
    double o[3], d[3];
    for (int c = 0; c < 3; c++) o[c] = lo[c] + U(rng) * (hi[c] - lo[c]);
    double tAim = -1.0;
    if (U(rng) < 0.5) { for (int c = 0; c < 3; c++) d[c] = N(rng); }
    else {
      // a corner (or a point on an edge) of the node's local box, through the forward chain in double, plus a tiny jitter
      double p[3];
      const int edgeAxis = int(U(rng) * 4.0) - 1;                 // -1: corner
      for (int c = 0; c < 3; c++) p[c] = c == edgeAxis ? nd.bmin[c] + U(rng) * (nd.bmax[c] - nd.bmin[c]) : (U(rng) < 0.5 ? nd.bmin[c] : nd.bmax[c]);
      for (int32_t a = int32_t(i); a >= 0; a = sc.nodes[a].parent) {
        const float* m = sc.nodes[a].xf.fwd;
        double q[3];
        for (int k = 0; k < 3; k++) q[k] = double(m[4 * k]) * p[0] + double(m[4 * k + 1]) * p[1] + double(m[4 * k + 2]) * p[2] + double(m[4 * k + 3]);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
      }
      double len = 0.0;
      for (int c = 0; c < 3; c++) { d[c] = p[c] - o[c]; len += d[c] * d[c]; }
      len = std::sqrt(len);
      for (int c = 0; c < 3; c++) d[c] = d[c] / len + 1e-6 * N(rng);
      tAim = len;
    }
    double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const f3 wo = mk3(float(o[0]), float(o[1]), float(o[2]));
    const f3 wd = mk3(float(d[0] / dl), float(d[1] / dl), float(d[2] / dl));
    const double sel = U(rng);
    const float tMax = tAim > 0.0 && sel < 0.5 ? float(tAim * (0.97 + 0.06 * U(rng))) : sel < 0.75 ? 1e30f : float(1.0 + 100.0 * U(rng));
    const float tMin = 1e-4f;
    f3 oo, od;
    objectRay(sc, i, wo, wd, oo, od);
    const RayO ray = makeRay(oo, od);
    float dd;
    pairs++;
    if (!testBox(ray, tMin, tMax, nd.bmin, nd.bmax, dd) || tMax < dd) continue;
    exact++;
    (nd.depth >= kMaxNodeDepth ? deepExact : shallowExact)++;
    const RayO world = makeRay(wo + 0.0f, wd + 0.0f);
    const f4 wlo = sc.nodeWorld[2u * i], whi = sc.nodeWorld[2u * i + 1u];
    const float wmin[3] = {wlo.x, wlo.y, wlo.z}, wmax[3] = {whi.x, whi.y, whi.z};
    float dw;
    if (!testBox(world, 0.0f, tMax + (fabsf(tMax) * 1e-4f + 1e-3f), wmin, wmax, dw)) {
      if (bad++ < 5) std::fprintf(stderr, "node %u depth %u: exact test accepts, world box rejects\n", i, nd.depth);
    }
  }
  std::printf("{\"pairs\": %llu, \"exact\": %llu, \"shallow\": %llu, \"deep\": %llu, \"bad\": %llu}\n",
              (unsigned long long) pairs, (unsigned long long) exact, (unsigned long long) shallowExact, (unsigned long long) deepExact,
              (unsigned long long) bad);
  return 0;
}
"""


@pytest.mark.parametrize("case", [(24, 1, 0, True), (24, 3, 0, True), (64, 2, 70, False), (64, 1, 0, True)],
                         ids=["d24", "d24b3", "d64b2p70", "d64"])
def test_world_precull_is_conservative_at_depth(built, tmp_path, case):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "precull.cpp", str(tmp_path / "precull")
    src.write_text(PRECULL_HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "yart_amd", "csrc"), "-I",
                    os.path.join(root, "include"), "-o", exe, str(src), os.path.join(root, "yart_amd", "csrc", "_gen", "lut_data.cpp"),
                    "-lpthread"], check=True)
    s, _ = _deep(*case)
    sp = str(tmp_path / "s.yscn")
    s.save(sp)
    out = subprocess.run([exe, sp, "1000000", str(case[0])], check=True, capture_output=True, text=True)
    res = json.loads(out.stdout)
    print(case, res)
    assert res["bad"] == 0, out.stderr
    assert res["shallow"] > 1000 and res["deep"] > 1000, res


# ------------------------------------------------------------------------------------------------------------- glTF
def _triangle_mesh(b, material):
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    n = np.tile(np.array([0, 0, 1], np.float32), (3, 1))
    return b.mesh([{"attributes": {"POSITION": b.accessor(p, "VEC3"), "NORMAL": b.accessor(n, "VEC3"),
                                   "TEXCOORD_0": b.accessor(p[:, :2].copy(), "VEC2")}, "material": material}])


def _chain_rows(n, seed=40):
    """n TRS rows "tx ty tz qx qy qz qw sx sy sz parent", each the child of the previous one (yart_ref xform's input)."""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        q = ga.quat_axis_angle(ax, float(rng.uniform(-1.5, 1.5)))
        sc = rng.uniform(0.6, 1.6, 3) if i % 2 == 0 else 1.0 / np.asarray(rows[-1][7:10])
        rows.append([float(np.float32(v)) for v in (*rng.uniform(-0.5, 0.5, 3), *q, *sc)] + [i - 1])
    return rows


def _chain_glb(path, rows, lit=lambda i: True):
    """A glTF chain of len(rows) nodes (node i the child of node i - 1), a one-triangle mesh on every node that `lit`
    selects (emissive: one area light per such node). Returns {row: mesh index}."""
    b = ga.GltfBuilder()
    glow = b.material(emissiveFactor=[1.0, 1.0, 1.0])
    meshes = {}
    # glTF node k holds row k; children are referenced by index, so the file can list them root first
    for i, r in enumerate(rows):
        mesh = None
        if lit(i):
            mesh = meshes[i] = _triangle_mesh(b, glow)
        b.node(mesh, translation=r[0:3], rotation=r[3:7], scale=r[7:10], children=[i + 1] if i + 1 < len(rows) else (), root=(i == 0))
    b.write_glb(path)
    return meshes


def _load(api, path, tmp_path):
    from yart_amd import yscn
    out = os.path.join(tmp_path, "out.yscn")
    api.gltf_to_yscn(path, out)
    return yscn.Scene.load(out)


@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    return api


@needs_ref
def test_gltf_40_level_chain_transforms_equal_reference(api, tmp_path):
    """A 40-level TRS chain with an emissive mesh on every node: node fwd / inv and area-light transforms (the product
    node.transform * globalTransform along the chain, gltf.cpp:293) equal the reference's float4x4 / Transform algebra."""
    rows = _chain_rows(40)
    txt, binp = str(tmp_path / "x.txt"), str(tmp_path / "x.bin")
    with open(txt, "w") as f:
        f.write("\n".join(" ".join(repr(v) for v in r) for r in rows) + "\n")
    subprocess.run([REF_BIN, "xform", txt, binp], check=True, capture_output=True)
    want = np.fromfile(binp, np.float32).reshape(len(rows), 4, 4, 4)
    glb = str(tmp_path / "c.glb")
    meshes = _chain_glb(glb, rows)
    s = _load(api, glb, tmp_path)
    by_mesh = {n.mesh: n for n in s.nodes if n.mesh >= 0}
    light_by_mesh = {l.mesh: l for l in s.lights}
    assert len(s.nodes) == 41 and max(_depths(s)) == 40
    # pre-order, children's lights first: the deepest node's light comes first
    assert [l.mesh for l in s.lights] == [meshes[i] for i in reversed(range(40))]
    for i in range(40):
        n, l = by_mesh[meshes[i]], light_by_mesh[meshes[i]]
        assert np.array_equal(n.fwd, want[i, 0]), i
        assert np.array_equal(n.inv, want[i, 1]), i
        assert np.array_equal(l.fwd, want[i, 2]), i
        assert np.array_equal(l.inv, want[i, 3]), i


def test_gltf_700_level_chain_imports(api, tmp_path):
    rows = _chain_rows(700, seed=7)
    glb = str(tmp_path / "c.glb")
    meshes = _chain_glb(glb, rows, lit=lambda i: i % 100 == 99)
    s = _load(api, glb, tmp_path)
    assert len(s.nodes) == 701
    assert [n.parent for n in s.nodes] == list(range(-1, 700))
    assert [l.mesh for l in s.lights] == [meshes[i] for i in (699, 599, 499, 399, 299, 199, 99)]


def test_gltf_cycle_is_refused(api, tmp_path):
    b = ga.GltfBuilder()
    m = _triangle_mesh(b, b.material())
    b.node(m, children=[1], root=True)
    b.node(None, children=[2])
    b.node(m, children=[1])                       # node 2 -> node 1: node 1 is its own ancestor
    glb = str(tmp_path / "cyc.glb")
    b.write_glb(glb)
    with pytest.raises(api.YartError) as e:
        api.gltf_to_yscn(glb, str(tmp_path / "out.yscn"))
    assert e.value.code == api.YART_E_IO and "cycle" in str(e.value) and "node 1" in str(e.value)


def test_gltf_shared_child_is_instanced_per_path(api, tmp_path):
    """A node reachable from two parents: one node record per path (the reference's recursion visits it twice)."""
    b = ga.GltfBuilder()
    m = _triangle_mesh(b, b.material(emissiveFactor=[1.0, 0.5, 0.25]))
    b.node(m, translation=[0.5, 0, 0])                               # node 0: shared
    b.node(None, translation=[1, 0, 0], children=[0], root=True)     # node 1
    b.node(None, translation=[0, 2, 0], children=[0], root=True)     # node 2
    glb = str(tmp_path / "shared.glb")
    b.write_glb(glb)
    s = _load(api, glb, tmp_path)
    assert [n.parent for n in s.nodes] == [-1, 0, 1, 0, 3]
    assert [n.mesh for n in s.nodes] == [-1, -1, m, -1, m]
    assert len(s.lights) == 2
    assert [float(l.fwd[0][3]) for l in s.lights] == [1.5, 0.5] and [float(l.fwd[1][3]) for l in s.lights] == [0.0, 2.0]


# ----------------------------------------------------------------------------------------------------------- Python
def _lights_recursive(s):
    """create_area_lights as it was written before (recursive): the order to keep."""
    children = {i: [] for i in range(len(s.nodes))}
    for i, n in enumerate(s.nodes):
        if n.parent >= 0: children[n.parent].append(i)
    out = []

    def visit(i):
        for c in children[i]: visit(c)
        n = s.nodes[i]
        if n.mesh < 0: return
        for t in range(len(s.meshes[n.mesh].faces)):
            if s.materials[int(s.meshes[n.mesh].faces[t, 3])].is_emissive:
                out.append((n.mesh, t, i))
    visit(0)
    return out


def test_create_area_lights_order_unchanged():
    from yart_amd import scenes
    for s, _ in (scenes.instances(n_instances=12), _deep(12, 3), scenes.material_test()):
        want = _lights_recursive(s)
        s.create_area_lights()
        got = [(l.mesh, l.tri) for l in s.lights if l.type == 0]
        assert got == [(m, t) for m, t, _ in want]
        for l, (_, _, node) in zip(s.lights, want):
            fwd, inv = s._global(node)
            assert np.array_equal(l.fwd, fwd) and np.array_equal(l.inv, inv)


def test_create_area_lights_3000_level_chain():
    from yart_amd import scenes
    from yart_amd.yscn import Material
    s, _ = scenes.cornell(16, 16, 1, 2)
    glow = s.add_material(Material(base=(0.5, 0.5, 0.5), emission=(2.0, 2.0, 2.0)))
    b = scenes.MeshBuilder()
    b.box((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1), glow)
    lamp = s.add_mesh(b.build())
    parent = 0
    for level in range(1, 3000):
        parent = s.add_node(lamp if level in (1500, 2999) else -1, parent, *scenes.trs(translation=(0, 1e-3, 0)))
    s.create_area_lights()
    area = [l for l in s.lights if l.type == 0]
    assert len(area) == 2 + 2 * 12        # the Cornell quad light (2 triangles), then 12 triangles per lamp... in post-order
    assert [l.mesh for l in area[2:]] == [lamp] * 24
    # children before their parent: the deepest lamp's lights come first, the Cornell mesh (a child of the root) before both
    assert area[0].mesh == 0
    assert np.isclose(area[2].fwd[1][3], 2999e-3, rtol=1e-3) and np.isclose(area[-1].fwd[1][3], 1500e-3, rtol=1e-3)


# -------------------------------------------------------------------------------------------------------------- GPU
GPU_CASES = [(12, 1, 0, True), (12, 3, 0, False), (24, 1, 0, True), (24, 3, 0, True)]
FUZZ_DEEP_SEEDS = list(range(100))


@pytest.mark.gpu
@pytest.mark.usefixtures("ref_bin")
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: f"d{c[0]}b{c[1]}{'ill' if c[3] else 'trs'}")
def test_deep_graphs_every_pipeline(api, tmp_path, case):
    from tests.test_gpu_parity import PIPELINE_FLAGS
    s, p = _deep(*case, width=48, height=40, spp=4)
    _, _, ref = _reference(tmp_path, s, p)
    ds = api.DeviceScene(s, device=0)
    for name, flags in PIPELINE_FLAGS.items():
        img, _ = ds.render(p, flags=flags)
        bit_identical_or_drift(img, ref.view(np.float32).reshape(img.shape), f"{case}/{name}")
    ds.close()


@pytest.mark.gpu
@pytest.mark.usefixtures("ref_bin")
@pytest.mark.parametrize("case", [(64, 1, 0, True), (64, 2, 70, False), (1000, 1, 0, True)], ids=["d64", "d64b2p70", "chain1000"])
def test_long_chains_fuzz_pipelines(api, tmp_path, case):
    from tests.test_fuzz_scenes import FUZZ_PIPELINES
    small = case[0] > 64
    s, p = _deep(*case, width=16 if small else 32, height=16 if small else 24, spp=1 if small else 2, bounces=2 if small else 4,
                 mesh_every=50 if small else 3, light_every=75 if small else 5)
    _, _, ref = _reference(tmp_path, s, p)
    ds = api.DeviceScene(s, device=0)
    for name, flags in FUZZ_PIPELINES.items():
        img, _ = ds.render(p, flags=flags)
        bit_identical_or_drift(img, ref.view(np.float32).reshape(img.shape), f"{case}/{name}")
    ds.close()


@pytest.mark.gpu
@pytest.mark.usefixtures("ref_bin")
def test_deep_gltf_renders_like_reference(api, tmp_path):
    """The 40-level chain asset through DeviceScene(path) against the reference's render of the .yscn the importer writes."""
    from yart_amd import scenes
    rows = _chain_rows(40)
    glb = str(tmp_path / "c.glb")
    _chain_glb(glb, rows, lit=lambda i: i % 4 == 3)
    sp = str(tmp_path / "c.yscn")
    api.gltf_to_yscn(glb, sp, uniform_env=(0.3, 0.3, 0.35))
    p = dict(size=(40, 32), spp=4, depth=3, focal=35.0, fnumber=0.0, eye=(0.0, 0.0, 12.0), target=(0.0, 0.0, 0.0),
             up=(0.0, 1.0, 0.0), exposure=0.0, background=(0.0, 0.0, 0.0))
    pp, ref = str(tmp_path / "c.txt"), str(tmp_path / "c.ref.f32")
    scenes.write_params(pp, p, threads=1)
    subprocess.run([REF_BIN, "render", sp, pp, ref], check=True, capture_output=True)
    ds = api.DeviceScene(glb, device=0, uniform_env=(0.3, 0.3, 0.35))
    img, _ = ds.render(p)
    bit_identical_or_drift(img, np.fromfile(ref, np.float32).reshape(img.shape), "gltf chain 40")
    ds.close()


@pytest.mark.gpu
@pytest.mark.usefixtures("ref_bin")
def test_deep_graph_tiles_and_waves(api, tmp_path):
    """Progressive waves and tiles of a 24-level tree: the same frame as the reference's."""
    s, p = _deep(24, 2, 0, True, width=80, height=72, spp=8)
    p["first_wave"], p["max_wave"], p["tile"] = 2, 4, 32
    _, _, ref = _reference(tmp_path, s, p)
    ds = api.DeviceScene(s, device=0)
    tiles, waves = [], []
    img, _, aborted = ds.render_tiles(p, on_tile=lambda f, t: tiles.append(t) and False, on_wave=lambda f, w: waves.append(w) and False)
    assert not aborted and tiles and len(waves) >= 2
    bit_identical_or_drift(img, ref.view(np.float32).reshape(img.shape), "deep tiles")
    img, _, aborted = ds.render_waves(p, on_wave=lambda f, w: False)
    assert not aborted
    bit_identical_or_drift(img, ref.view(np.float32).reshape(img.shape), "deep waves")
    ds.close()


@pytest.mark.gpu
@pytest.mark.usefixtures("ref_bin")
def test_fuzz_deep_graphs(api, tmp_path):
    from yart_amd import scenes
    from tests.test_fuzz_scenes import FUZZ_PIPELINES
    bad = []
    for seed in FUZZ_DEEP_SEEDS:
        s, p = scenes.fuzz_deep_case(seed)
        _, _, ref = _reference(tmp_path, s, p, tag=str(seed))
        ds = api.DeviceScene(s, device=0)
        for name, flags in FUZZ_PIPELINES.items():
            img, _ = ds.render(p, flags=flags)
            g = np.ascontiguousarray(img, np.float32).view(np.uint32).ravel()
            if not np.array_equal(ref, g):
                bad.append(f"seed {seed} / {name}: {(ref != g).sum()} words differ")
        ds.close()
    assert not bad, "\n".join(bad[:40])
