"""What the tools that time the in-place scene updates share (scene_update_bench.py, mesh_update_trace.py, lighting_update_trace.py,
texture_update_trace.py): one warm-up and the median of RUNS calls, re-creation of the device scene timed that way, and the
statistics of RUNS + 1 update calls."""
import ctypes as C
import statistics
import time

from yart_amd import api

RUNS = 5


def median_ms(fn, runs=RUNS):
    """wall time of fn() in ms: one warm-up, then the median of `runs` calls"""
    t = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t[1:])


def recreate_ms(s):
    """-> (median_ms of yart_hip_scene_destroy + yart_hip_scene_create of s — the C calls alone: the description is marshalled once —,
    the handle of the scene the last call made: the caller's to destroy)"""
    L = api.lib()
    desc, keep = api.describe_scene(s)
    h = C.c_void_p()
    api._check(L.yart_hip_scene_create(C.byref(desc), 0, C.byref(h)), L)

    def recreate():
        nonlocal h
        L.yart_hip_scene_destroy(h)
        h = C.c_void_p()
        api._check(L.yart_hip_scene_create(C.byref(desc), 0, C.byref(h)), L)
    return median_ms(recreate), h


def scene_over(h):
    """the binding's marshalling (DeviceScene.update_*) over a handle made with the C calls; the handle stays the caller's"""
    scene = api.DeviceScene.__new__(api.DeviceScene)
    scene._h, scene._L, scene._keep, scene.last_update = h, api.lib(), [], None
    return scene


def update_stats(update, runs=RUNS):
    """update(k) makes the k-th of runs + 1 update calls and returns its statistics (a SceneUpdateStats or DeviceScene.last_update)
    -> the calls' [ms_total], [ms_device], [launches]; the first call is the warm-up"""
    rows = []
    for k in range(runs + 1):
        st = update(k)
        rows.append((st["ms_total"], st["ms_device"], st["launches"]) if isinstance(st, dict) else (st.ms_total, st.ms_device, st.launches))
    return [list(column) for column in zip(*rows)]
