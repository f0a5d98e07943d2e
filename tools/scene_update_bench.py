"""Wall time of re-creating a device scene against yart_hip_scene_update (profiles/scene_update.txt).

For each scene: yart_hip_scene_destroy + yart_hip_scene_create of the same description (the C calls alone: the description is
marshalled once), and yart_hip_scene_update with every node moved (a small translation composed onto its transform), refit and
YART_UPDATE_REBUILD_TOP — one warm-up, then the median of 5 runs each.

    python tools/scene_update_bench.py [--out profiles/scene_update.txt] [--skip-sponza]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api, scenes  # noqa: E402
from update_trace_common import recreate_ms, update_stats  # noqa: E402

def node_array(nodes, shift):
    nd = (api.NodeDesc * len(nodes))()
    for i, n in enumerate(nodes):
        f = np.array(n.fwd, np.float64)
        if i > 0:
            f[:3, 3] += shift
        f32 = f.astype(np.float32)
        nd[i] = api.NodeDesc(n.parent, n.mesh, api._f(f32, 16), api._f(np.linalg.inv(f32.astype(np.float64)).astype(np.float32), 16))
    return nd


def measure(name, s, out):
    L = api.lib()
    create, h = recreate_ms(s)
    arrays = [node_array(s.nodes, 0.01 * (k + 1)) for k in range(2)]
    rows = {}
    for tag, flags in (("refit", 0), ("rebuild", api.UPDATE_REBUILD_TOP)):
        def update(k):
            up = api.SceneUpdate(C.sizeof(api.SceneUpdate), len(s.nodes), arrays[k % 2], 0, None, flags)
            st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
            api._check(L.yart_hip_scene_update(h, C.byref(up), None, C.byref(st)), L)
            return st
        total, device, launches = update_stats(update)
        rows[tag] = (statistics.median(total[1:]), statistics.median(device[1:]), launches[-1], total[0])
    L.yart_hip_scene_destroy(h)
    tris = sum(len(m.faces) for m in s.meshes)
    # (first call: the scene's first update, which builds its topology tables — the refit runs come first on a fresh handle; the
    # rebuild runs follow on the same handle, so their warm-up is no first call and is not reported)
    line = (f"{name:<22} {len(s.nodes):>7} nodes {tris:>8} tris | destroy+create {create:>10.3f} ms | "
            f"update refit: total {rows['refit'][0]:.3f} ms, device {rows['refit'][1]:.3f} ms, {rows['refit'][2]} launches "
            f"(first call {rows['refit'][3]:.3f} ms) | "
            f"update rebuild: total {rows['rebuild'][0]:.3f} ms, device {rows['rebuild'][1]:.3f} ms, {rows['rebuild'][2]} launches")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-sponza", action="store_true")
    a = ap.parse_args()
    out = ["# tools/scene_update_bench.py: median of 5 runs after one warm-up; wall time of the C calls; every node but the root moved; tris: of the meshes, before instancing"]
    for n in (70, 4096, 65536):
        t0 = time.perf_counter()
        s, _ = scenes.instances(n_instances=n, groups=4)
        print(f"# instances({n}): described in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(f"instances({n})", s, out)
    if not a.skip_sponza:
        t0 = time.perf_counter()
        s, _ = scenes.sponza_class(detail=1.0)
        print(f"# sponza_class: described in {time.perf_counter() - t0:.1f} s", flush=True)
        measure("sponza_class(1.0)", s, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
