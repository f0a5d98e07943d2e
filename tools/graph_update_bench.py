"""What a changed node list costs in place, next to what callers did before (profiles/graph_update.txt).

For instances(4096), instances(16000) and instances(65536), in one run per scene:
  update_graph     yart_hip_scene_update_graph from the scene's list to one with 1 % more nodes (instances appended as children of the
                   root), to one with 1 % fewer (the last instances removed) and to one in which 1 % of the instances have another mesh
                   of the scene — with the top-level hierarchy built on the device (flags 0) and on the host (YART_UPDATE_REBUILD_TOP).
                   Before every timed call an untimed one puts the scene's own list back, so every timed call makes the change.
  floor            yart_hip_scene_update(YART_UPDATE_REBUILD_TOP_DEVICE) with the scene's own list: the chain the graph update adds
                   its topology work to
  re-create        yart_hip_scene_destroy + yart_hip_scene_create of the scene with the appended list: what callers did before
One warm-up, then the median of 5 calls each: the wall time of the C call, its device time, its launches.

    python tools/graph_update_bench.py [--out profiles/graph_update.txt]"""
import argparse
import copy
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from yart_amd import api, scenes  # noqa: E402
from update_trace_common import recreate_ms, update_stats  # noqa: E402

WAYS = (("device", 0), ("host", api.UPDATE_REBUILD_TOP))


def desc_array(nodes):
    nd = (api.NodeDesc * len(nodes))()
    for i, n in enumerate(nodes):
        nd[i] = api.NodeDesc(n.parent, n.mesh, api._f(n.fwd, 16), api._f(n.inv, 16))
    return nd


def variants(s):
    """-> {name: node list}: 1 % of the instances appended, removed, re-meshed"""
    inst = [i for i, n in enumerate(s.nodes) if n.mesh >= 0 and n.parent > 0]
    k = max(len(inst) // 100, 1)
    other = next(m for m in range(len(s.meshes)) if m != s.nodes[inst[0]].mesh)
    appended = list(s.nodes)
    for i in inst[:k]:                                  # copies of the first instances, as children of the root
        n = copy.copy(s.nodes[i])
        n.parent = 0
        appended.append(n)
    assert all(s.nodes[i].mesh >= 0 for i in range(len(s.nodes) - k, len(s.nodes))), "the list ends in instances: leaves"
    remeshed = list(s.nodes)
    for i in inst[::len(inst) // k][:k]:
        remeshed[i] = copy.copy(s.nodes[i])
        remeshed[i].mesh = other
    return {"append 1 %": appended, "remove 1 %": list(s.nodes[:-k]), "re-mesh 1 %": remeshed}


def measure(name, s, out):
    L = api.lib()
    lists = variants(s)
    appended = copy.copy(s)
    appended.nodes = lists["append 1 %"]
    create, h = recreate_ms(appended)
    L.yart_hip_scene_destroy(h)
    desc, keep = api.describe_scene(s)
    h = C.c_void_p()
    api._check(L.yart_hip_scene_create(C.byref(desc), 0, C.byref(h)), L)
    own = desc_array(s.nodes)

    def graph(nd, flags):
        up = api.SceneGraphUpdate(C.sizeof(api.SceneGraphUpdate), len(nd), nd, 0, None, flags)
        st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
        api._check(L.yart_hip_scene_update_graph(h, C.byref(up), None, C.byref(st)), L)
        return st

    def floor(k):
        up = api.SceneUpdate(C.sizeof(api.SceneUpdate), len(own), own, 0, None, api.UPDATE_REBUILD_TOP_DEVICE)
        st = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
        api._check(L.yart_hip_scene_update(h, C.byref(up), None, C.byref(st)), L)
        return st
    lines = [f"{name}: {len(s.nodes)} nodes; re-create (destroy + create of the appended list): {create:.3f} ms"]
    total, device, launches = update_stats(floor)
    floor_ms = statistics.median(total[1:])
    lines.append(f"{name}: floor, yart_hip_scene_update(REBUILD_TOP_DEVICE): total {floor_ms:.3f} ms, device {statistics.median(device[1:]):.3f} ms, "
                 f"{launches[-1]} launches")
    for what, nodes in lists.items():
        nd = desc_array(nodes)
        for tag, flags in WAYS:
            def change(k):
                graph(own, flags)
                return graph(nd, flags)
            total, device, launches = update_stats(change)
            ms = statistics.median(total[1:])
            lines.append(f"{name}: update_graph {what:<11} ({len(nodes)} nodes), {tag:<6} build: total {ms:.3f} ms, device {statistics.median(device[1:]):.3f} ms, "
                         f"{launches[-1]} launches | {ms / floor_ms:.2f} x the floor, re-create / update {create / ms:.1f}")
    L.yart_hip_scene_destroy(h)
    for line in lines:
        print(line, flush=True)
    out += lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# tools/graph_update_bench.py: median of 5 calls after one warm-up; wall time of the C call (total) and its device time",
           "# every timed update_graph call starts from the scene's own list (put back by an untimed call) and makes the change named"]
    for n in (4096, 16000, 65536):
        t0 = time.perf_counter()
        s, _ = scenes.instances(96, 96, 1, 4, n_instances=n, groups=4)
        print(f"# instances({n}): described in {time.perf_counter() - t0:.1f} s", flush=True)
        measure(f"instances({n})", s, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
