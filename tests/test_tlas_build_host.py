"""The level-wise build of the top-level hierarchy on the host: csrc/tlas_build.hpp::tlasBuildLevelwise — the statement the kernels of
csrc/tlas_build_kernels.inc restate — against host_scene.hpp::buildTopLevel, byte for byte, on the aimed inputs of tests/tlassuite.py
(tests/tlassim/tlassim.cpp); the constants of the contract for a C compiler; and the argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tlassuite, updatesim
from tests.conftest import ROOT

SIM_SOURCES = ["tlassim/tlassim.cpp"]


def _cap():
    from yart_amd import api
    return api.TLAS_LOCAL_LEAVES


def run_suite(exe, tmp_path, cases):
    path = os.path.join(tmp_path, "suite.bin")
    tlassuite.save(cases, path)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-2000:]
    assert "DIFFERENT" not in r.stdout
    lines = re.findall(r"^EQUAL case (\d+) kind (\d+) leaves (\d+) nodes (\d+) records (\d+) height (\d+)$", r.stdout, re.M)
    assert len(lines) == len(cases)
    for (kind, leaves, mesh, _), line in zip(cases, lines):
        k, kd, lv, nn, rec, height = (int(v) for v in line)
        assert (kd, lv, nn, rec) == (tlassuite.KINDS.index(kind), leaves, len(mesh), 2 * leaves - 1)
        assert height == int(np.ceil(np.log2(leaves))) if leaves > 1 else height == 0


def test_suite_covers_its_kinds_and_keeps_the_zero_rule(built):
    cap = _cap()
    cases = tlassuite.suite(cap)
    assert all(n >= 8 for n in tlassuite.counts(cases).values()), tlassuite.counts(cases)
    counts = tlassuite.leaf_counts(cap)
    assert counts[:8] == [1, 2, 3, 4, 5, 63, 64, 65] and max(counts) >= 8 * cap + 5
    assert {cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap, 2 * cap + 1, 4 * cap + 3} <= set(counts)
    tlassuite.check_signed_zero_rule(cases)


def test_levelwise_build_equals_the_recursive_one_on_bytes(built, tmp_path):
    """Every case of the suite: tlasBuildLevelwise == buildTopLevel, records and height."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "tlassim"), SIM_SOURCES)
    run_suite(exe, str(tmp_path), tlassuite.suite(_cap()))


def test_sanitized_build_runs_clean(built, tmp_path):
    """The same program under -fsanitize=address,undefined (a stand-alone program: no preloading) on the sizes up to 2 cap + 1."""
    exe = updatesim.build_sim(os.path.join(tmp_path, "tlassim_san"), SIM_SOURCES, sanitized=True)
    run_suite(exe, str(tmp_path), tlassuite.suite(_cap(), max_leaves=2 * _cap() + 1))


def test_constants_for_a_c_compiler(built, tmp_path):
    """YART_UPDATE_REBUILD_TOP_DEVICE == 2 and kTlasLocalLeaves as the binding has them; the C++ mirror's overloads exist."""
    from yart_amd import api
    src = os.path.join(tmp_path, "c.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include "../yart_amd/csrc/tlas_build.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%u %u %u\\n\", YART_UPDATE_REBUILD_TOP_DEVICE, yart_hip::kTlasLocalLeaves,"
                " unsigned(yart::hip::DeviceScene::TopLevel::RebuildDevice));\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fn)(const std::vector<YartNodeDesc>&, const std::vector<YartLightDesc>&,"
                " yart::hip::DeviceScene::TopLevel, void*) = &yart::hip::DeviceScene::update;\n"
                "  YartSceneUpdateStats (yart::hip::DeviceScene::*fm)(const std::vector<YartMeshUpdate>&, yart::hip::DeviceScene::TopLevel, void*)"
                " = &yart::hip::DeviceScene::updateMeshes;\n"
                "  return fn && fm ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "c")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [api.UPDATE_REBUILD_TOP_DEVICE, api.TLAS_LOCAL_LEAVES, 2] and api.UPDATE_REBUILD_TOP_DEVICE == 2


def test_argument_errors_without_a_device(built):
    """The flag pair 1 | 2, the new flag on a handle that is no scene, NULL pointers and n_nodes >= 2^20 are refused with YART_E_INVALID before
    a scene or a device is looked at; the entries are exported and bound; the host entry builds, and fewer than 64 nodes give no records."""
    from yart_amd import api
    L = api.lib()
    assert {"yart_hip_tlas_build_device", "yart_hip_tlas_build_host"} <= set(api.EXPORTS)
    fake = ctypes.c_void_p(0x1000)                   # a handle that is never dereferenced: the update itself is checked first
    nodes = (api.NodeDesc * 1)()
    up = api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, nodes, 0, None, 3)
    assert L.yart_hip_scene_update(fake, ctypes.byref(up), None, None) == api.YART_E_INVALID
    assert b"flags" in L.yart_hip_last_error() and b"exclude each other" in L.yart_hip_last_error()
    one = (api.MeshUpdate * 1)()
    mu = api.SceneMeshUpdate(ctypes.sizeof(api.SceneMeshUpdate), 1, one, 3)
    assert L.yart_hip_scene_update_meshes(fake, ctypes.byref(mu), None, None) == api.YART_E_INVALID
    assert b"flags" in L.yart_hip_last_error() and b"exclude each other" in L.yart_hip_last_error()
    # the new flag alone on such a handle: still an error return that names the flags (its value was an unknown flag before)
    for entry, upd in ((L.yart_hip_scene_update, api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, nodes, 0, None, 2)),
                       (L.yart_hip_scene_update_meshes, api.SceneMeshUpdate(ctypes.sizeof(api.SceneMeshUpdate), 1, one, 2))):
        assert entry(fake, ctypes.byref(upd), None, None) == api.YART_E_INVALID
        assert b"flags: YART_UPDATE_REBUILD_TOP_DEVICE" in L.yart_hip_last_error()
    for bad in (4, 6, 7, 0x80000002):
        up = api.SceneUpdate(ctypes.sizeof(api.SceneUpdate), 1, nodes, 0, None, bad)
        assert L.yart_hip_scene_update(fake, ctypes.byref(up), None, None) == api.YART_E_INVALID
        assert b"unknown flags" in L.yart_hip_last_error()
    world = np.zeros((70, 8), np.float32)
    mesh = np.zeros(70, np.int32)
    tlas = np.zeros(139, api.TLAS_DTYPE)
    n, h = ctypes.c_uint32(9), ctypes.c_uint32(9)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for entry, head in ((L.yart_hip_tlas_build_host, ()), (L.yart_hip_tlas_build_device, (0,))):
        for args in ((None, vp(mesh), 70, vp(tlas), ctypes.byref(n), ctypes.byref(h)), (vp(world), None, 70, vp(tlas), ctypes.byref(n), ctypes.byref(h)),
                     (vp(world), vp(mesh), 70, None, ctypes.byref(n), ctypes.byref(h)), (vp(world), vp(mesh), 70, vp(tlas), None, ctypes.byref(h)),
                     (vp(world), vp(mesh), 70, vp(tlas), ctypes.byref(n), None)):
            assert entry(*head, *args) == api.YART_E_INVALID
            assert b"null" in L.yart_hip_last_error()
        for count in (1 << 20, (1 << 20) + 5, 0xffffffff):
            assert entry(*head, vp(world), vp(mesh), count, vp(tlas), ctypes.byref(n), ctypes.byref(h)) == api.YART_E_INVALID
            assert b"2^20" in L.yart_hip_last_error()
    with pytest.raises(api.YartError):
        api.DeviceScene.update(None, [], rebuild_top="gpu")
    with pytest.raises(api.YartError):
        api.DeviceScene.update_meshes(None, {}, rebuild_top=2)
    # the host entry: 70 boxes on a line; 63 nodes: no tree
    world[:, 0] = np.arange(70)
    world[:, 4] = world[:, 0] + 0.5
    world[:, 5:7] = 1.0
    got, height = api.tlas_build(world, mesh, device=None)
    assert len(got) == 139 and height == 7 and int(got["b"].sum()) == 70 and sorted(got["a"][got["b"] == 1]) == list(range(70))
    assert got["lo"][0, 0] == 0.0 and got["hi"][0, 0] == 69.5
    assert len(api.tlas_build(world[:63], mesh[:63], device=None)[0]) == 0
    assert len(api.tlas_build(world, np.full(70, -1, np.int32), device=None)[0]) == 0
