"""First-hit feature buffers (include/yart_hip.h: YartAovBuffers, yart_hip_render_aovs[_device], yart_hip_probe_camera_rays).

The definition is the reference's `Hit` of bounce 0 of every (pixel, sample) of the frame, reduced per pixel by a float32 sum in
ascending sample order and one division (api.reduce_aov_samples). The GPU tests hold the buffers to it on bits, through pieces
that are pinned to the compiled reference elsewhere: the sampler (probe_sampler vs the KATs), cameraRay of csrc/integrator.hpp
(the `camera_rays` KAT section), the device traversal's hit records (probe_hits vs the reference's testNode), and — where the
walk needs the sampler (stochastic alpha) or the material lookup — the product's device headers compiled for the host
(tests/aovsim), which the host KAT tests and the bit-exact host frames pin."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def _camera_and_params(api, **over):
    p = dict(size=(16, 8), spp=8, depth=3, eye=(0, 0, 5), target=(0, 0, 0))
    p.update(over)
    return api.make_camera(p), api.make_params(p)


def test_aov_abi_and_argument_errors(built, tmp_path):
    """The new symbols exist, the ABI version is still 3, YartAovBuffers has the declared layout, the C++ mirror compiles, and
    every argument error is YART_E_INVALID with a message — decided before any device is touched (there is no scene here)."""
    from yart_amd import api
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in ("yart_hip_render_aovs", "yart_hip_render_aovs_device", "yart_hip_probe_camera_rays"):
        assert hasattr(raw, name), name
        assert name in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    assert ctypes.sizeof(api.AovBuffers) == 8 + 7 * ctypes.sizeof(ctypes.c_void_p)
    assert api.AovBuffers.albedo.offset == 8 and api.AovBuffers.rays.offset == 8 + 6 * ctypes.sizeof(ctypes.c_void_p)
    # sizeof / constants as the C compiler sees them, and the C++ mirror (DeviceScene::renderAovs)
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %u %u\\n\", sizeof(YartAovBuffers), YART_AOV_ALL,\n"
                "    YART_AOV_ALBEDO | YART_AOV_NORMAL | YART_AOV_POSITION | YART_AOV_DEPTH | YART_AOV_COVERAGE | YART_AOV_IDS | YART_AOV_RAYS);\n"
                "  yart::hip::AovFrame (yart::hip::DeviceScene::*fn)(const YartCameraDesc&, const YartRenderParams&, uint32_t, YartStats*) = &yart::hip::DeviceScene::renderAovs;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.AovBuffers), 127, 127]

    cam, rp = _camera_and_params(api)
    frame = np.zeros((8, 16, 4), np.float32)
    buf = np.zeros((8, 16, 4), np.float32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    fp = frame.ctypes.data_as(ctypes.c_void_p)

    def call(ab, rp=rp, device=False):
        if device:
            return L.yart_hip_render_aovs_device(None, ctypes.byref(cam), ctypes.byref(rp), fp, ctypes.byref(ab), None, None)
        return L.yart_hip_render_aovs(None, ctypes.byref(cam), ctypes.byref(rp), fp, ctypes.byref(ab), None)

    def buffers(mask, size=ctypes.sizeof(api.AovBuffers), **ptrs):
        ab = api.AovBuffers()
        ab.struct_size, ab.mask = size, mask
        for k, v in ptrs.items():
            setattr(ab, k, v)
        return ab

    for device in (False, True):
        # a requested buffer is NULL
        assert call(buffers(1 | 2, albedo=ptr), device=device) == api.YART_E_INVALID
        assert b"normal is null" in L.yart_hip_last_error()
        # unknown mask bits
        assert call(buffers(128, albedo=ptr), device=device) == api.YART_E_INVALID
        assert b"mask" in L.yart_hip_last_error()
        # struct_size ends before a requested field (rays is the last one)
        assert call(buffers(64, size=ctypes.sizeof(api.AovBuffers) - 8, rays=ptr), device=device) == api.YART_E_INVALID
        assert b"struct_size" in L.yart_hip_last_error()
        assert call(buffers(1, size=4, albedo=ptr), device=device) == api.YART_E_INVALID
        assert b"struct_size" in L.yart_hip_last_error()
        # partial sample ranges
        for over in (dict(start_sample=4), dict(stop_sample=4)):
            _, part = _camera_and_params(api, first_wave=4, max_wave=4, **over)
            assert call(buffers(8, depth=ptr), rp=part, device=device) == api.YART_E_INVALID
            assert b"full sample range" in L.yart_hip_last_error()
        # well-formed buffers, no scene: still refused, for that reason
        assert call(buffers(8, depth=ptr), device=device) == api.YART_E_INVALID
        assert b"scene" in L.yart_hip_last_error()
    assert L.yart_hip_probe_camera_rays(None, ctypes.byref(cam), ctypes.byref(rp), 1, ptr, ptr) == api.YART_E_INVALID


def test_numpy_statement_of_the_reduction():
    """api.reduce_aov_samples / reduce_aov_coverage — the definition the GPU tests compare against — on hand-made samples:
    ascending-s float32 sums (the order matters), misses skipped, one division; a pixel without hits, one with all hits."""
    from yart_amd import api
    f = np.float32
    big, one = f(2.0 ** 24), f(1.0)
    # pixel 0: no hit; pixel 1: every sample hits; pixel 2: order-sensitive values; pixel 3: misses carry garbage that must not count
    vals = np.zeros((4, 4, 2), f)
    hit = np.zeros((4, 4), bool)
    vals[1] = [[1, 10], [2, 20], [3, 30], [4, 40]]; hit[1] = True
    vals[2, :, 0] = [big, one, one, -big]; vals[2, :, 1] = [one, one, big, -big]; hit[2] = True
    vals[3] = [[5, 5], [np.nan, np.inf], [7, 7], [1e30, -1e30]]; hit[3] = [True, False, True, False]
    got = api.reduce_aov_samples(vals, hit)
    assert got.dtype == np.float32 and got.shape == (4, 2)
    assert np.array_equal(got[0], [0, 0])
    assert np.array_equal(got[1], [f(10) / f(4), f(100) / f(4)])
    # ((2^24 + 1) + 1) - 2^24 = 0 in float32 (each + 1 is rounded away); ((1 + 1) + 2^24) - 2^24 = 2
    assert np.array_equal(got[2], [f(0), f(2) / f(4)])
    assert np.array_equal(got[3], [f(12) / f(4), f(12) / f(4)])
    exp = np.zeros(2, f)
    for s in range(4):          # the same thing as an explicit scalar loop
        exp = (exp + vals[2, s]).astype(f)
    assert np.array_equal(got[2].view(np.uint32), (exp / f(4)).view(np.uint32))
    cov = api.reduce_aov_coverage(hit)
    assert cov.dtype == np.float32 and np.array_equal(cov, [0, 1, 1, 0.5])
    # `samples` is the divisor when the values cover the whole range by construction (3 samples: 1/3 is not exact)
    assert api.reduce_aov_coverage(np.array([[True, False, True]]))[0] == f(2) / f(3)
    assert api.reduce_aov_samples(np.ones((1, 3, 1), f), np.ones((1, 3), bool))[0, 0] == f(3) / f(3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


@pytest.fixture(scope="module")
def aovsim(built, tmp_path_factory):
    """tests/aovsim/aovsim.cpp: the product's device headers compiled for the host (as build() compiles tests/hostsim)."""
    exe = str(tmp_path_factory.mktemp("aovsim") / "aovsim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "aovsim", "aovsim.cpp"),
                    os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
    return exe


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4, what
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ (first at {np.argwhere(diff)[0].tolist()})"


def _triples(w, h, spp, x0=0, y0=0, W=None, H=None):
    """(x, y, s) of every sample of the window, pixel-major (row-major pixels), samples ascending."""
    ys, xs, ss = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(spp), indexing="ij")
    return np.stack([xs, ys, ss], -1).reshape(-1, 3).astype(np.uint32)


def _save(tmp_path, s, p, tag):
    from yart_amd import scenes
    sp, pp = tmp_path / f"{tag}.yscn", tmp_path / f"{tag}.txt"
    s.save(sp)
    scenes.write_params(pp, p)
    return str(sp), str(pp)


def _host_hits(aovsim, tmp_path, sp, pp, triples):
    """tests/aovsim `hits`: dict of per-(pixel, sample) arrays of bounce 0 from the host-compiled device headers."""
    fin, fout = str(tmp_path / "hits.in"), str(tmp_path / "hits.out")
    np.ascontiguousarray(triples, np.uint32).tofile(fin)
    subprocess.run([aovsim, "hits", sp, pp, fin, fout], check=True)
    w = np.fromfile(fout, np.uint32).reshape(-1, 22)
    assert len(w) == len(triples)
    f = w.view(np.float32)
    return dict(ray=f[:, 0:6], hit=w[:, 6] == 1, t=f[:, 7:8], p=f[:, 8:11], n=f[:, 11:14], albedo=f[:, 14:17],
                ids=w[:, 17:21].view(np.int32))


def _expected(api, per, h, w, spp):
    """The buffers the definition gives for per-sample values `per` (dict as _host_hits returns; pixel-major, h x w x spp)."""
    hit = per["hit"].reshape(h, w, spp)
    exp = {}
    for name, key in (("albedo", "albedo"), ("normal", "n"), ("position", "p"), ("depth", "t")):
        if key in per:
            v = api.reduce_aov_samples(per[key].reshape(h, w, spp, -1), hit)
            exp[name] = v[..., 0] if name == "depth" else v
    exp["coverage"] = api.reduce_aov_coverage(hit)
    if "ids" in per:
        ids = per["ids"].reshape(h, w, spp, 4)[:, :, 0, :]
        exp["ids"] = np.where(hit[:, :, 0, None], ids, -1).astype(np.int32)
    return exp


CAMERA_SCENES = {"cornell": lambda sc: sc.cornell(128, 128, 16, 4), "material": lambda sc: sc.material_test(96, 64, 16, 6)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CAMERA_SCENES))
def test_probe_camera_rays_is_sampler_then_camera(gpu_api, aovsim, tmp_path, case):
    """probe_camera_rays == (the sampler's film and lens draws of (x, y, s), probe_sampler: pinned to the reference's draws)
    through (cameraRay of csrc/integrator.hpp compiled for the host: pinned to the reference's Camera::getRay by the
    camera_rays KAT), bit for bit; `material` has a hexagonal aperture at f/2.8 (the lens draw matters). The wave schedule
    starts with 2 samples: most of the samples checked lie beyond the first wave."""
    from yart_amd import scenes
    s, p = CAMERA_SCENES[case](scenes)
    p = dict(p, first_wave=2, max_wave=8)
    sp, pp = _save(tmp_path, s, p, case)
    w, h = p["size"]
    rng = np.random.RandomState(3)
    n = 600
    tri = np.stack([rng.randint(0, w, n), rng.randint(0, h, n), rng.randint(0, p["spp"], n)], -1).astype(np.uint32)
    tri[:4] = [[0, 0, 0], [w - 1, h - 1, p["spp"] - 1], [w - 1, 0, 1], [0, h - 1, 2]]
    assert len(tri) >= 256 and (tri[:, 2] >= 2).sum() >= 256
    scene = gpu_api.DeviceScene(s, device=0)
    got = scene.probe_camera_rays(p, tri)
    draws = scene.probe_sampler(p["spp"], p.get("tile", 64), tri, [2, 2])
    scene.close()
    rec = np.zeros((n, 6), np.uint32)
    rec[:, 0:2] = tri[:, 0:2]
    rec[:, 2:6] = bits(draws.astype(np.float32))
    fin, fout = str(tmp_path / "cam.in"), str(tmp_path / "cam.out")
    rec.tofile(fin)
    subprocess.run([aovsim, "camrays", sp, pp, fin, fout], check=True)
    exp = np.fromfile(fout, np.float32).reshape(n, 6)
    same_bits(got, exp, f"{case}: camera rays")
    if case == "material":
        assert len(np.unique(bits(got[:, 0]))) > n // 2, "depth of field: the ray origins must move over the aperture"


def _chain_scenes(sc):
    return {"cornell": sc.cornell(128, 128, 16, 4), "material": sc.material_test(96, 64, 16, 6), "two_skies": sc.two_skies(),
            "deep_instances": sc.deep_instances(depth=12, branching=2, width=48, height=48, spp=4)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell", "material", "two_skies", "deep_instances"])
def test_buffers_vs_camera_rays_and_hit_records(gpu_api, aovsim, tmp_path, case):
    """Every pixel of the frame (>= 900): per-sample camera rays (probe_camera_rays) -> probe_hits (the reference's testNode
    Hit, pinned by the hit-record KAT) -> the numpy reduction == normal, position, depth, coverage and the triangle id.
    Albedo and the other ids come from the host-compiled device headers (tests/aovsim: matBase of csrc/bsdf.hpp at the hit's
    uv), whose rays, t, p, n and triangle are checked against the device chain sample by sample; where a pixel's hits
    all have untextured materials, the albedo must also be the reduction of the materials' plain base colours.
    `material` and `two_skies` have an alpha cut-out card: probe_hits has no sampler state, so for the samples whose camera ray meets
    the card its hit is not the path's (they are shown to be exactly those); pixels with such a sample are held to the host
    walk with the sampler instead — as every pixel is — and the device chain is asserted on all the others."""
    from yart_amd import scenes
    api = gpu_api
    s, p = _chain_scenes(scenes)[case]
    alpha_mats = [i for i, m in enumerate(s.materials) if m.tex_base >= 0 and not s.textures[m.tex_base].is_float
                  and s.textures[m.tex_base].channels == 4 and (s.textures[m.tex_base].data[..., 3] < 255).any()]
    assert case != "deep_instances" or not alpha_mats, "the deep scene graph must have no alpha-tested material"
    w, h = p["size"]
    spp = p["spp"]
    assert w * h >= 900
    tri = _triples(w, h, spp)
    sp, pp = _save(tmp_path, s, p, case)
    scene = api.DeviceScene(s, device=0)
    frame, got, st = scene.render_aovs(p)
    rays = scene.probe_camera_rays(p, tri)
    ph = scene.probe_hits(rays)
    scene.close()
    dev = dict(hit=ph[:, 0] == 1.0, t=ph[:, 1:2], p=ph[:, 4:7], n=ph[:, 7:10])
    # the host statement: same rays as the device chain, and — sample by sample — the same hit wherever no alpha test decides
    host = _host_hits(aovsim, tmp_path, sp, pp, tri)
    same_bits(host["ray"], rays, f"{case}: host camera rays")
    agree = host["hit"] == dev["hit"]
    for k in ("t", "p", "n"):
        agree &= ~dev["hit"] | (bits(host[k]) == bits(dev[k])).all(-1)
    agree &= ~dev["hit"] | (host["ids"][:, 3] == ph[:, 13].astype(np.int32))
    if not alpha_mats:
        assert agree.all(), f"{case}: host walk and probe_hits differ on {int((~agree).sum())} samples"
    else:
        # probe_hits knows nothing of the sampler: its alpha tests draw other numbers than the path's (the issue's item 5). Where
        # the two walks differ, one of them accepted a cut-out candidate the other passed: the path's own hit (host walk, with the
        # sampler) is on the alpha-tested material, or the probe stopped in front of it
        d = ~agree
        on_card = host["hit"] & np.isin(host["ids"][:, 2], alpha_mats)
        probe_nearer = dev["hit"] & (~host["hit"] | (dev["t"][:, 0] < host["t"][:, 0]))
        assert (on_card | probe_nearer)[d].all(), f"{case}: walks differ away from the alpha card"
        print(f"{case}: {int(d.sum())} of {d.size} samples decided by an alpha test")
    clean = agree.reshape(h, w, spp).all(-1)          # pixels whose every sample the device chain reproduces
    assert clean.mean() > 0.75
    exp = _expected(api, dev, h, w, spp)
    for name in ("normal", "position", "depth", "coverage"):
        same_bits(got[name][clean], exp[name][clean], f"{case}: {name} vs camera rays -> probe_hits -> reduction")
    tri0 = np.where(dev["hit"].reshape(h, w, spp)[:, :, 0], ph[:, 13].reshape(h, w, spp)[:, :, 0].astype(np.int32), -1)
    assert np.array_equal(got["ids"][..., 3][clean], tri0[clean]), f"{case}: triangle ids"
    assert 0.0 < float(got["coverage"].mean()) and (case in ("cornell", "deep_instances") or float(got["coverage"].min()) < 1.0)
    # every pixel, every buffer against the host statement (on the clean pixels the same numbers as above, plus albedo and ids)
    hexp = _expected(api, host, h, w, spp)
    for name in ("normal", "position", "depth", "coverage"):
        same_bits(got[name], hexp[name], f"{case}: {name} vs host walk")
    same_bits(got["albedo"], hexp["albedo"], f"{case}: albedo vs matBase at the hits")
    assert np.array_equal(got["ids"], hexp["ids"]), f"{case}: ids"
    # ids against the scene description: the node's mesh, the triangle's material
    ids = got["ids"].reshape(-1, 4)
    for node, mesh, mat, t in ids[ids[:, 0] >= 0][::7]:
        assert s.nodes[node].mesh == mesh and int(s.meshes[mesh].faces[t, 3]) == mat
    # untextured materials: the base colour itself
    base = np.array([m.base for m in s.materials], np.float32)
    textured = np.array([m.tex_base >= 0 for m in s.materials])
    mat = np.where(host["hit"], host["ids"][:, 2], 0)
    plain = dict(hit=host["hit"], albedo=base[mat])
    pexp = _expected(api, plain, h, w, spp)["albedo"]
    untex = ~(textured[mat] & host["hit"]).reshape(h, w, spp).any(-1)
    assert untex.sum() > 0.3 * w * h or case == "material"
    same_bits(got["albedo"][untex], pexp[untex], f"{case}: albedo of untextured materials")
    if case == "material":
        assert (~untex).sum() > 100, "the material scene must show textured base colours"
    assert int(got["rays"].sum()) == st["rays"]


def _all_flags():
    from tests.test_gpu_parity import PIPELINE_FLAGS
    return PIPELINE_FLAGS


@pytest.mark.gpu
def test_alpha_scene_buffers_vs_host_walk_every_pipeline(gpu_api, aovsim, tmp_path):
    """Stochastic alpha: which candidate bounce 0 accepts depends on draws inside the walk, so the per-sample truth is the host
    run of the product's device headers (tests/aovsim `hits`: the general walk with the sampler; csrc/integrator.hpp is
    pinned to the reference on this scene's frames). Every buffer == the reduction of it, and every pipeline gives the
    same buffers and the frame of `render`."""
    from yart_amd import scenes
    api = gpu_api
    s, p = scenes.alpha_instances(n_instances=9)
    w, h = p["size"]
    spp = p["spp"]
    assert w * h >= 900
    sp, pp = _save(tmp_path, s, p, "alpha")
    host = _host_hits(aovsim, tmp_path, sp, pp, _triples(w, h, spp))
    exp = _expected(api, host, h, w, spp)
    scene = api.DeviceScene(s, device=0)
    ref_frame, ref_st = scene.render(p)
    # the scene must exercise the alpha test at bounce 0: some camera rays pass a candidate the plain walk would have taken
    ph = scene.probe_hits(host["ray"])
    passed = (ph[:, 0] == 1.0) & (~host["hit"] | (bits(ph[:, 1]) != bits(host["t"][:, 0])))
    assert passed.sum() > 50, "no camera ray passed through an alpha cut-out"
    for name, flags in _all_flags().items():
        frame, got, st = scene.render_aovs(p, flags=flags)
        same_bits(frame, ref_frame, f"alpha / {name}: frame")
        assert st["rays"] == ref_st["rays"] and int(got["rays"].sum()) == st["rays"]
        for k in ("albedo", "normal", "position", "depth", "coverage"):
            same_bits(got[k], exp[k], f"alpha / {name}: {k}")
        assert np.array_equal(got["ids"], exp["ids"]), f"alpha / {name}: ids"
    scene.close()


@pytest.mark.gpu
def test_buffers_do_not_depend_on_pipeline_batches_waves_estimator(gpu_api):
    """One scene at 64 spp: the full set of buffers is bit-identical across every pipeline flag set, max_batch_paths (one
    batch, 2 batches, >= 5 batches), one wave vs doubling waves, and the four estimators."""
    from yart_amd import scenes
    api = gpu_api
    s, p = scenes.material_test(96, 64, 64, 6)
    npaths = 96 * 64 * 64
    scene = api.DeviceScene(s, device=0)
    frame0, ref, st0 = scene.render_aovs(p)
    assert set(ref) == set(api.AOVS)

    def check(tag, q, flags=0, frame_too=True):
        frame, got, st = scene.render_aovs(q, flags=flags)
        for k in api.AOVS:
            same_bits(got[k], ref[k], f"{tag}: {k}")
        if frame_too:
            same_bits(frame, frame0, f"{tag}: frame")
            assert st["rays"] == st0["rays"]

    for name, flags in _all_flags().items():
        check(name, p, flags)
        for batches, cap in (("2 batches", npaths // 2), ("6 batches", npaths // 6 + 1)):
            if name in ("wavefront", "megakernel", "wavefront+path_pool", "wavefront+no_compaction"):
                check(f"{name} / {batches}", dict(p, max_batch_paths=cap), flags)
    waves = dict(p, first_wave=1, max_wave=16)        # 1, 1, 2, 4, 8, 16, 16, 16: a pixel's samples span eight waves
    for name in ("wavefront", "megakernel", "wavefront+path_pool"):
        # (the blended frame of a multi-wave render is another frame; the feature buffers and the ray counts are not)
        frame, got, st = scene.render_aovs(waves, flags=_all_flags()[name])
        assert st["waves"] == 8 and st["rays"] == st0["rays"]
        for k in api.AOVS:
            same_bits(got[k], ref[k], f"doubling waves / {name}: {k}")
        plain, _ = scene.render(waves, flags=_all_flags()[name])
        same_bits(frame, plain, f"doubling waves / {name}: frame vs render")
    check("doubling waves in 6 batches", dict(waves, max_batch_paths=96 * 64 * 16 // 6 + 1), frame_too=False)
    for est in (api.ESTIMATOR_GMON, api.ESTIMATOR_MEAN, api.ESTIMATOR_MON, api.ESTIMATOR_GMONB):
        check(f"estimator {est}", dict(p, estimator=est), frame_too=False)
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_buffers_add_up_to_the_unsharded_ones(gpu_api, world):
    """rank / world_size: pixels of other ranks are 0 (ids -1); the ranks' buffers (rendered one after the other on device 0)
    are disjoint and add up — ids combine by max — to the unsharded buffers, bit for bit."""
    from yart_amd import scenes
    api = gpu_api
    s, p = scenes.material_test(96, 64, 16, 6)
    p = dict(p, tile=16)
    scene = api.DeviceScene(s, device=0)
    frame, full, st = scene.render_aovs(p)
    acc = {k: (np.full_like(v, -1) if k == "ids" else np.zeros_like(v)) for k, v in full.items()}
    owned = np.zeros((64, 96), np.int32)
    rays = 0
    for r in range(world):
        fr, part, pst = scene.render_aovs(p, rank=r, world_size=world)
        mine = fr[..., 3] == 1.0
        owned += mine
        for k, v in part.items():
            other = v[~mine]
            assert np.all(other == (-1 if k == "ids" else 0)), f"rank {r}: {k} written outside the rank's pixels"
            acc[k] = np.maximum(acc[k], v) if k == "ids" else acc[k] + v
        rays += pst["rays"]
        assert int(part["rays"].sum()) == pst["rays"]
    assert np.all(owned == 1)
    for k in full:
        same_bits(acc[k], full[k], f"world {world}: {k}")
    assert rays == st["rays"]
    scene.close()


@pytest.mark.gpu
def test_frame_unchanged_and_device_tensors(gpu_api, tmp_path):
    """render_aovs' frame and ray count are render's; the rays buffer sums to stats.rays; a subset of buffers and an empty
    mask work; render_aovs_into (torch device tensors) == the host-pointer variant."""
    from yart_amd import scenes
    api = gpu_api
    s, p = scenes.cornell(128, 128, 16, 4)
    scene = api.DeviceScene(s, device=0)
    frame, st = scene.render(p)
    fa, bufs, sa = scene.render_aovs(p)
    same_bits(fa, frame, "frame of render_aovs vs render")
    assert sa["rays"] == st["rays"] and sa["samples"] == st["samples"]
    assert int(bufs["rays"].astype(np.uint64).sum()) == st["rays"]
    f0, none, s0 = scene.render_aovs(p, aovs=())
    same_bits(f0, frame, "empty mask")
    assert none == {} and s0["rays"] == st["rays"]
    f1, some, _ = scene.render_aovs(p, aovs=("normal", "ids"))
    same_bits(some["normal"], bufs["normal"], "subset: normal")
    assert np.array_equal(some["ids"], bufs["ids"])
    scene.close()
    # torch device tensors: in a process of its own that initialises torch's HIP runtime first, as bench.py does
    code = (
        "import sys, numpy as np, torch\n"
        "torch.cuda.set_device(0)\n"
        "from yart_amd import api, scenes\n"
        "s, p = scenes.cornell(128, 128, 16, 4)\n"
        "scene = api.DeviceScene(s, device=0)\n"
        "frame, bufs, st = scene.render_aovs(p)\n"
        "dev = torch.device('cuda:0')\n"
        "t_frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)\n"
        "tens = {k: torch.full((128, 128, ch) if ch > 1 else (128, 128), 7, dtype=torch.float32 if dt == np.float32 else torch.int32, device=dev)\n"
        "        for k, (bit, ch, dt) in api.AOVS.items()}\n"
        "sd = scene.render_aovs_into(t_frame, tens, p, stream=torch.cuda.current_stream().cuda_stream)\n"
        "torch.cuda.synchronize()\n"
        "bad = [] if np.array_equal(t_frame.cpu().numpy().view(np.uint32), frame.view(np.uint32)) else ['frame']\n"
        "bad += [k for k, t in tens.items() if not np.array_equal(t.cpu().numpy().view(np.uint32), bufs[k].view(np.uint32))]\n"
        "bad += [] if sd['rays'] == st['rays'] else ['rays']\n"
        "np.save(sys.argv[1], bufs['depth'])\n"
        "scene.close()\n"
        "print('differ:', bad)\n"
        "sys.exit(1 if bad else 0)\n")
    out = os.path.join(tmp_path, "depth.npy")
    r = subprocess.run([sys.executable, "-c", code, out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    same_bits(np.load(out), bufs["depth"], "the child process rendered the same scene")
