"""What a mesh with new faces and new counts costs in place, next to what callers did before (profiles/mesh_replace.txt).

Two scenes, each measured in one run:
  heightfield(n=256)          the field (mesh 1, 131072 triangles) re-tessellated to n = 192 (73728) and to n = 320 (204800)
  material_test(tex=1024)     the instanced mesh (mesh 1, 156 triangles; 7.3 M texels of textures stay on the device) swapped for one of
                              twice its faces (312)
and for each:
  re-create        yart_hip_scene_destroy + yart_hip_scene_create of the scene with the new mesh: what callers did before
  replace_meshes   yart_hip_scene_replace_meshes to the new mesh. Before every timed call an untimed one puts the scene's own mesh back,
                   so every timed call changes the counts and repacks; the first call (which allocates the second arrays) is shown
  floor            yart_hip_scene_update_meshes of the scene's own mesh (positions, normals, tangents): the rebuild at equal counts
  fast path        yart_hip_scene_replace_meshes with the scene's own mesh: equal counts, nothing is repacked
One warm-up, then the median of 5 calls each: the wall time of the C call, its device time, its launches.

    python tools/mesh_replace_bench.py [--out profiles/mesh_replace.txt]"""
import argparse
import copy
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from yart_amd import api, scenes  # noqa: E402
from update_trace_common import recreate_ms, update_stats  # noqa: E402


def replace_struct(mesh, m):
    """-> (YartSceneMeshReplace for one mesh, what has to outlive its use)"""
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (m.positions, m.normals, m.tangents, m.uvs)] + [np.ascontiguousarray(m.faces, np.uint32)]
    one = (api.MeshReplace * 1)(api.MeshReplace(mesh, api.MeshDesc(len(arrays[0]), len(arrays[4]), *(vp(a) for a in arrays), None)))
    return api.SceneMeshReplace(C.sizeof(api.SceneMeshReplace), 1, one, 0), (one, arrays)


def measure(name, s, mesh, variants, out):
    """variants: {what: the mesh that replaces s.meshes[mesh]}"""
    L = api.lib()
    desc, keep = api.describe_scene(s)
    h = C.c_void_p()
    api._check(L.yart_hip_scene_create(C.byref(desc), 0, C.byref(h)), L)
    own, keep_own = replace_struct(mesh, s.meshes[mesh])
    tris = sum(len(m.faces) for m in s.meshes)
    texels = sum(t.width * t.height for t in s.textures)
    lines = [f"{name}: {tris} tris, {texels / 1e6:.2f} M texels, mesh {mesh} ({len(s.meshes[mesh].faces)} tris) is replaced"]

    def replace(up):
        st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
        api._check(L.yart_hip_scene_replace_meshes(h, C.byref(up), None, C.byref(st)), L)
        return st
    for what, m in variants.items():
        changed = copy.copy(s)
        changed.meshes = list(s.meshes)
        changed.meshes[mesh] = m
        create, hc = recreate_ms(changed)
        L.yart_hip_scene_destroy(hc)
        up, keep_up = replace_struct(mesh, m)

        def change(k):
            replace(own)
            return replace(up)
        total, device, launches = update_stats(change)
        ms = statistics.median(total[1:])
        verdict = f"re-create / replace {create / ms:.1f}" if ms < create else f"NOT faster than the re-creation ({create / ms:.2f})"
        lines.append(f"{name}: {what:<24} ({len(m.faces)} tris) | destroy+create {create:>9.3f} ms | replace_meshes: total {ms:.3f} ms, device "
                     f"{statistics.median(device[1:]):.3f} ms, {launches[-1]} launches (first call {total[0]:.3f} ms) | {verdict}")
    replace(own)
    pos, nrm, tan = (np.ascontiguousarray(a, np.float32) for a in (s.meshes[mesh].positions, s.meshes[mesh].normals, s.meshes[mesh].tangents))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    one = (api.MeshUpdate * 1)(api.MeshUpdate(mesh, len(pos), vp(pos), vp(nrm), vp(tan)))
    mu = api.SceneMeshUpdate(C.sizeof(api.SceneMeshUpdate), 1, one, 0)

    def floor(k):
        st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
        api._check(L.yart_hip_scene_update_meshes(h, C.byref(mu), None, C.byref(st)), L)
        return st
    total, device, launches = update_stats(floor)
    floor_ms = statistics.median(total[1:])
    lines.append(f"{name}: floor, update_meshes at equal counts: total {floor_ms:.3f} ms, device {statistics.median(device[1:]):.3f} ms, {launches[-1]} launches")
    total, device, launches = update_stats(lambda k: replace(own))
    ms = statistics.median(total[1:])
    lines.append(f"{name}: fast path, replace_meshes at equal counts: total {ms:.3f} ms, device {statistics.median(device[1:]):.3f} ms, {launches[-1]} launches "
                 f"| {ms / floor_ms:.2f} x the floor")
    L.yart_hip_scene_destroy(h)
    for line in lines:
        print(line, flush=True)
    out += lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# tools/mesh_replace_bench.py: median of 5 calls after one warm-up; wall time of the C call (total) and its device time",
           "# every timed replace_meshes call starts from the scene's own mesh (put back by an untimed call) and changes the counts"]
    s, _ = scenes.heightfield(96, 96, 1, 4, n=256)
    measure("heightfield(n=256)", s, 1, {f"re-tessellated to n={n}": scenes.heightfield(96, 96, 1, 4, n=n)[0].meshes[1] for n in (192, 320)}, out)
    s, _ = scenes.material_test(96, 64, 1, 4, tex=1024)
    inst = s.meshes[1]
    mats = sorted(set(int(m) for m in inst.faces[:, 3]))
    b = scenes.MeshBuilder()
    b.box((-0.5, 0, -0.5), (0.5, 1, 0.5), mats[0])
    b.sphere((0, 1.4, 0), 0.4, mats[-1], nu=25, nv=6)
    twice = b.build()
    assert len(twice.faces) == 2 * len(inst.faces), (len(twice.faces), len(inst.faces))
    measure("material_test(tex=1024)", s, 1, {"twice its faces": twice}, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
