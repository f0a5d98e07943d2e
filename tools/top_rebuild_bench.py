"""What the top-level hierarchy costs an update, three ways, and when a fresh tree pays (profiles/top_rebuild.txt).

For instances(4096), instances(16000) and instances(65536): yart_hip_scene_update with every node but the root moved (a small
translation composed onto its transform) — refit (flags 0), YART_UPDATE_REBUILD_TOP (host) and YART_UPDATE_REBUILD_TOP_DEVICE in the
same run, one warm-up, then the median of 5 calls each: the wall time of the C call, its device time, its launches.

For the 4096- and 16000-instance scenes also the wall time of one small frame (96 x 96, 1 spp; median of 5 after a warm-up) in two
states: the instances' transforms permuted among themselves and the tree refitted, and the same state with the tree rebuilt on the
device.

    python tools/top_rebuild_bench.py [--out profiles/top_rebuild.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from yart_amd import api, scenes  # noqa: E402
from scene_update_bench import node_array  # noqa: E402
from update_trace_common import median_ms, scene_over, update_stats  # noqa: E402

WAYS = (("refit", 0), ("host rebuild", api.UPDATE_REBUILD_TOP), ("device rebuild", api.UPDATE_REBUILD_TOP_DEVICE))


def permuted_array(nodes, seed=3):
    """the node records with the instances' transforms (mesh nodes below a group) permuted among themselves"""
    nd = node_array(nodes, 0.0)
    inst = [i for i, n in enumerate(nodes) if n.mesh >= 0 and n.parent > 0]
    perm = np.random.default_rng(seed).permutation(len(inst))
    src = [(bytes(nd[i].fwd), bytes(nd[i].inv)) for i in inst]
    for i, j in zip(inst, perm):
        C.memmove(nd[i].fwd, src[j][0], 64)
        C.memmove(nd[i].inv, src[j][1], 64)
    return nd


def measure(name, s, p, render, out):
    L = api.lib()
    desc, keep = api.describe_scene(s)
    h = C.c_void_p()
    api._check(L.yart_hip_scene_create(C.byref(desc), 0, C.byref(h)), L)
    arrays = [node_array(s.nodes, 0.01 * (k + 1)) for k in range(2)]

    def update_with(nd, flags):
        up = api.SceneUpdate(C.sizeof(api.SceneUpdate), len(s.nodes), nd, 0, None, flags)
        st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
        api._check(L.yart_hip_scene_update(h, C.byref(up), None, C.byref(st)), L)
        return st
    update_with(arrays[0], 0)                       # the scene's first update builds its tables: not part of any row
    update_with(arrays[0], api.UPDATE_REBUILD_TOP_DEVICE)
    cells = []
    for tag, flags in WAYS:
        total, device, launches = update_stats(lambda k: update_with(arrays[k % 2], flags))
        cells.append(f"{tag}: total {statistics.median(total[1:]):.3f} ms, device {statistics.median(device[1:]):.3f} ms, {launches[-1]} launches")
    line = f"{name:<18} {len(s.nodes):>7} nodes | " + " | ".join(cells)
    print(line, flush=True)
    out.append(line)
    if render:
        scene = scene_over(h)
        nd = permuted_array(s.nodes)
        for tag, flags in (("permuted, refitted", 0), ("permuted, rebuilt on the device", api.UPDATE_REBUILD_TOP_DEVICE)):
            update_with(nd, flags)
            ms = median_ms(lambda: scene.render(p))
            line = f"{name:<18} render {p['size'][0]} x {p['size'][1]} x {p['spp']} spp, {tag}: {ms:.3f} ms"
            print(line, flush=True)
            out.append(line)
        scene._h = C.c_void_p()                     # (the handle is this function's: the wrapper must not destroy it a second time)
    L.yart_hip_scene_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# tools/top_rebuild_bench.py: median of 5 calls after one warm-up; wall time of the C call (total) and its device time; every node but the root moved",
           "# render lines: wall time of yart_hip_render of one small frame, median of 5 after one warm-up"]
    for n in (4096, 16000, 65536):
        t0 = time.perf_counter()
        s, p = scenes.instances(96, 96, 1, 4, n_instances=n, groups=4)
        print(f"# instances({n}): described in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(f"instances({n})", s, p, n <= 16000, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
