"""Wall time of yart_hip_scene_update_meshes against re-creating the device scene (profiles/mesh_update.txt).

Two scenes: scenes.heightfield(n=256) — the 131 k-triangle height field deforms, so nearly all of the scene is rebuilt either way —
and scenes.material_test(tex=1024) — a textured scene (eight 1024^2 maps and their footprint records) in which the small instanced
mesh deforms. For each: yart_hip_scene_destroy + yart_hip_scene_create of the same description (the C calls alone: the description is
marshalled once; what a caller without the update has to do per frame), and the update with the mesh's vertices scaled a little, two
sets of vertices in turn, with the device build and with the host builder (YART_HOST_BVH) — one warm-up, then the median of 5 runs
each. (destroy + create builds on the device in both rows.)

    python tools/mesh_update_trace.py [--out profiles/mesh_update.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api, scenes  # noqa: E402
from update_trace_common import recreate_ms, update_stats  # noqa: E402

def measure(name, s, mesh, out):
    L = api.lib()
    create, h = recreate_ms(s)
    m = s.meshes[mesh]
    base = np.ascontiguousarray(m.positions, np.float32)
    sets = [np.ascontiguousarray(base * np.float32(1.0 + 0.03 * (k + 1))) for k in range(2)]
    nrm, tan = np.ascontiguousarray(m.normals, np.float32), np.ascontiguousarray(m.tangents, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = {}
    for tag in ("device", "host"):                  # the builder: the device build, and the host builder the library takes under YART_HOST_BVH
        if tag == "host":
            os.environ["YART_HOST_BVH"] = "1"
        def update(k):
            one = (api.MeshUpdate * 1)(api.MeshUpdate(mesh, len(base), vp(sets[k % 2]), vp(nrm), vp(tan)))
            up = api.SceneMeshUpdate(C.sizeof(api.SceneMeshUpdate), 1, one, 0)
            st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
            api._check(L.yart_hip_scene_update_meshes(h, C.byref(up), None, C.byref(st)), L)
            return st
        total, device, launches = update_stats(update)
        os.environ.pop("YART_HOST_BVH", None)
        rows[tag] = (statistics.median(total[1:]), statistics.median(device[1:]), launches[-1], total[0])
    total, device, launches = [rows["device"][3], rows["device"][0]], [0.0, rows["device"][1]], rows["device"][2]
    L.yart_hip_scene_destroy(h)
    tris = sum(len(x.faces) for x in s.meshes)
    texels = sum(t.width * t.height for t in s.textures)
    line = (f"{name:<24} {tris:>8} tris, {texels / 1e6:6.2f} M texels, mesh {mesh} deforms ({len(m.faces)} tris) | destroy+create "
            f"{create:>9.3f} ms | update_meshes: total {statistics.median(total[1:]):.3f} ms, device "
            f"{statistics.median(device[1:]):.3f} ms, {launches} launches (first call {total[0]:.3f} ms) | with the host builder "
            f"(YART_HOST_BVH): total {rows['host'][0]:.3f} ms, {rows['host'][2]} launches")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# tools/mesh_update_trace.py: median of 5 runs after one warm-up; wall time of the C calls; positions, normals and tangents of one mesh passed"]
    s, _ = scenes.heightfield(n=256)
    measure("heightfield(n=256)", s, 1, out)
    s, _ = scenes.material_test(tex=1024)
    measure("material_test(tex=1024)", s, 1, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
