"""Per-pixel sample moments (include/yart_hip.h: YartMomentBuffers, yart_hip_render_moments[_device], yart_hip_probe_moments).

The definition is the header comment; yart_amd/moments.py `moments_reference` states it in NumPy (float32 samples, float64
sums, ascending sample order) and is the reference of every comparison here, all of them on bits: csrc/moments.hpp compiled
for the host (tests/momentsim, also under ASan + UBSan), the kernels alone (api.probe_moments) and the kernels inside a
render, whose per-sample truth is DeviceScene.probe_samples — an independent device path that the golden tests pin."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

EXPOSURE_SCALE = 2.0
PROBE_PIXELS = [1, 63, 64, 65, 257]          # one group of lanes, a block less one pixel / exactly / plus one (16 pixels per
PROBE_SPP = [1, 2, 15, 16, 17, 65]           # block of 256), several blocks; fewer / exactly / more samples than a group's 16 lanes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4, what
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ (first at {np.argwhere(diff)[0].tolist()})"


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the reference, computed once per case and shared by the tests
# ---------------------------------------------------------------------------------------------------------------------
_inputs, _reference = {}, {}


def samples(n, spp):
    """[n, spp, 3] float32, seeded: radiance over [0, 10) with, sprinkled over a tenth of the records, NaN, +Inf, -Inf, negatives,
    -0, 3e38 (its luminance overflows after the exposure scale), 1.5e38 (it does not), denormals and zeros; pixel 0 is a
    clean low-noise pixel, and where there are pixels enough, some have all samples equal and one has none accepted."""
    if (n, spp) not in _inputs:
        rng = np.random.RandomState(100 * n + spp)
        a = rng.uniform(0, 10, (n, spp, 3)).astype(np.float32)
        special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 3e38, 1.5e38, 1e-40, 0.0, -1e-42], np.float32)
        flat = a.reshape(-1)
        hit = rng.rand(flat.size) < 0.1 / 3
        flat[hit] = special[rng.randint(len(special), size=int(hit.sum()))]
        a[0] = (np.float32(1000.0) + rng.uniform(0, 1e-3, (spp, 3))).astype(np.float32)       # S2 - S1^2 / N cancels in float32
        if n >= 8:
            a[1] = np.float32(0.1)                             # all samples equal
            a[2] = np.array([0.3, 7.0, 1e-3], np.float32)      # all equal, channels apart
            a[3] = np.float32(1e-41)                           # all equal, denormal
            a[4] = np.float32(np.nan)                          # nothing accepted
            a[5, 0] = np.float32(1.0)
            a[5, 1:] = np.float32(-2.0)                        # one accepted sample (if spp > 1: variance 0 by N < 2)
        _inputs[(n, spp)] = a
        a.setflags(write=False)
    return _inputs[(n, spp)]


def reference(n, spp):
    from yart_amd.moments import moments_reference
    if (n, spp) not in _reference:
        _reference[(n, spp)] = moments_reference(samples(n, spp), EXPOSURE_SCALE)
    return _reference[(n, spp)]


def doubling_chunks(spp):
    """1, 1, 2, 4, ... cut off where the sum reaches spp: the wave schedule of a render that starts with one sample"""
    out, nxt = [], 1
    while sum(out) < spp:
        out.append(min(nxt, spp - sum(out)))
        nxt = 1 if len(out) == 1 else nxt * 2
    return out


def check_all_equal(n, spp, var, cnt):
    """All samples of a pixel equal: the variance is never negative, exactly 0 where every binary64 operation of the definition
    is exact (N a power of two up to 16: N * y, N * y * y and (N * y)^2 all fit 53 bits), and otherwise no more than the
    roundings of the definition allow: S2 is a sum of N terms (each addition within 2^-53 of S2) and (S1 * S1) / N two more
    roundings of a number of S2's size, so |S2 - S1 * S1 / N| <= (N + 2) * 2^-53 * N * y^2, over (N - 1) * N."""
    from yart_amd.moments import luma
    if n < 8:
        return
    a = samples(n, spp)
    for px in (1, 2, 3):
        y = float(luma((a[px, 0] * np.float32(EXPOSURE_SCALE)).astype(np.float32)))
        assert cnt[px] == spp
        assert var[px] >= 0.0
        if spp in (1, 2, 16):
            assert var[px] == 0.0, (px, spp, var[px])
        else:
            assert float(var[px]) <= 2.0 * (spp + 2) / (spp - 1) * 2.0 ** -53 * y * y, (px, spp, var[px])
    assert cnt[4] == 0 and var[4] == 0
    assert cnt[5] == 1 and var[5] == 0


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def _camera_and_params(api, **over):
    p = dict(size=(16, 8), spp=8, depth=3, eye=(0, 0, 5), target=(0, 0, 0))
    p.update(over)
    return api.make_camera(p), api.make_params(p)


def test_moment_abi_and_argument_errors(built, tmp_path):
    """The new symbols exist and are in api.EXPORTS, the ABI version is still 3, YartMomentBuffers and the constants agree between
    ctypes, a C++ compiler and the C++ mirror (DeviceScene::renderMoments), and every argument error is YART_E_INVALID with a
    message — decided before any device is touched (there is no scene here)."""
    from yart_amd import api
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in ("yart_hip_render_moments", "yart_hip_render_moments_device", "yart_hip_probe_moments"):
        assert hasattr(raw, name), name
        assert name in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    assert ctypes.sizeof(api.MomentBuffers) == 8 + 3 * ctypes.sizeof(ctypes.c_void_p)
    assert api.MomentBuffers.mean.offset == 8 and api.MomentBuffers.count.offset == 8 + 2 * ctypes.sizeof(ctypes.c_void_p)
    assert {k: v[0] for k, v in api.MOMENTS.items()} == {"mean": 1, "variance": 2, "count": 4}
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %u %u %u %u\\n\", sizeof(YartMomentBuffers), YART_MOMENT_MEAN, YART_MOMENT_VARIANCE,\n"
                "    YART_MOMENT_COUNT, YART_MOMENT_ALL);\n"
                "  yart::hip::MomentFrame (yart::hip::DeviceScene::*fn)(const YartCameraDesc&, const YartRenderParams&, uint32_t, uint32_t, YartStats*) = &yart::hip::DeviceScene::renderMoments;\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.MomentBuffers), 1, 2, 4, 7]

    cam, rp = _camera_and_params(api)
    frame = np.zeros((8, 16, 4), np.float32)
    buf = np.zeros((8, 16, 4), np.float32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    fp = frame.ctypes.data_as(ctypes.c_void_p)

    def call(mb, rp=rp, device=False):
        if device:
            return L.yart_hip_render_moments_device(None, ctypes.byref(cam), ctypes.byref(rp), fp, None, ctypes.byref(mb), None, None)
        return L.yart_hip_render_moments(None, ctypes.byref(cam), ctypes.byref(rp), fp, None, ctypes.byref(mb), None)

    def buffers(mask, size=ctypes.sizeof(api.MomentBuffers), **ptrs):
        mb = api.MomentBuffers()
        mb.struct_size, mb.mask = size, mask
        for k, v in ptrs.items():
            setattr(mb, k, v)
        return mb

    for device in (False, True):
        # a requested buffer is NULL
        assert call(buffers(1 | 2, mean=ptr), device=device) == api.YART_E_INVALID
        assert b"variance is null" in L.yart_hip_last_error()
        assert call(buffers(4), device=device) == api.YART_E_INVALID
        assert b"count is null" in L.yart_hip_last_error()
        # unknown mask bits
        assert call(buffers(8, mean=ptr), device=device) == api.YART_E_INVALID
        assert b"mask" in L.yart_hip_last_error()
        # struct_size ends before a requested field (count is the last one)
        assert call(buffers(4, size=ctypes.sizeof(api.MomentBuffers) - 8, count=ptr), device=device) == api.YART_E_INVALID
        assert b"struct_size" in L.yart_hip_last_error()
        assert call(buffers(1, size=4, mean=ptr), device=device) == api.YART_E_INVALID
        assert b"struct_size" in L.yart_hip_last_error()
        # partial sample ranges
        for over in (dict(start_sample=4), dict(stop_sample=4)):
            _, part = _camera_and_params(api, first_wave=4, max_wave=4, **over)
            assert call(buffers(2, variance=ptr), rp=part, device=device) == api.YART_E_INVALID
            assert b"full sample range" in L.yart_hip_last_error()
        # a bad feature-buffer struct next to good moments is still refused
        ab = api.AovBuffers()
        ab.struct_size, ab.mask = ctypes.sizeof(api.AovBuffers), 128
        mb = buffers(2, variance=ptr)
        if device:
            rc = L.yart_hip_render_moments_device(None, ctypes.byref(cam), ctypes.byref(rp), fp, ctypes.byref(ab), ctypes.byref(mb), None, None)
        else:
            rc = L.yart_hip_render_moments(None, ctypes.byref(cam), ctypes.byref(rp), fp, ctypes.byref(ab), ctypes.byref(mb), None)
        assert rc == api.YART_E_INVALID and b"YartAovBuffers.mask" in L.yart_hip_last_error()
        # well-formed buffers, no scene: still refused, for that reason
        assert call(buffers(2, variance=ptr), device=device) == api.YART_E_INVALID
        assert b"scene" in L.yart_hip_last_error()
    # the probe: null pointers, empty sizes, chunks that do not sum to spp
    one = np.array([4], np.uint32).ctypes.data_as(ctypes.c_void_p)
    assert L.yart_hip_probe_moments(None, 1, 4, one, 1, 1.0, ptr, ptr, ptr) == api.YART_E_INVALID
    assert L.yart_hip_probe_moments(ptr, 1, 4, one, 1, 1.0, ptr, None, ptr) == api.YART_E_INVALID
    assert L.yart_hip_probe_moments(ptr, 0, 4, one, 1, 1.0, ptr, ptr, ptr) == api.YART_E_INVALID
    assert L.yart_hip_probe_moments(ptr, 1, 5, one, 1, 1.0, ptr, ptr, ptr) == api.YART_E_INVALID
    assert b"sum" in L.yart_hip_last_error()
    zero = np.array([4, 0], np.uint32).ctypes.data_as(ctypes.c_void_p)
    assert L.yart_hip_probe_moments(ptr, 1, 4, zero, 2, 1.0, ptr, ptr, ptr) == api.YART_E_INVALID


def test_numpy_statement_on_hand_made_samples():
    """moments_reference on samples whose answer is known without running it."""
    from yart_amd.moments import luma, moments_reference
    f = np.float32
    # two samples (1, 1, 1) and (3, 3, 3): mean 2; y = l, 3 l with l = luma(1, 1, 1); variance of the mean = ((y1 - y2)^2 / 2) / 2 = l^2
    l1 = float(luma(np.ones(3, f)))
    mean, var, cnt = moments_reference(np.array([[[1, 1, 1], [3, 3, 3]]], f), 1.0)
    assert cnt[0] == 2 and np.array_equal(mean[0], [2, 2, 2])
    assert abs(float(var[0]) - l1 * l1) <= 2e-7
    assert mean.dtype == np.float32 and var.dtype == np.float32 and cnt.dtype == np.uint32
    # the exposure scale multiplies the samples before anything else: variance scales by its square
    _, var4, _ = moments_reference(np.array([[[1, 1, 1], [3, 3, 3]]], f), 2.0)
    assert var4[0] == f(4) * var[0]
    # rejected samples do not count: NaN, negative, a luminance that overflows; -0 and denormals do
    x = np.array([[[1, 1, 1], [np.nan, 1, 1], [1, -1, 1], [np.inf, 0, 0], [-0.0, 0.0, 1e-42], [3, 3, 3]]], f)
    mean, var, cnt = moments_reference(x, 1.0)
    assert cnt[0] == 3
    big = np.array([[[3e38, 3e38, 3e38], [1, 1, 1]]], f)          # finite as it is, infinite after an exposure scale of 2
    assert moments_reference(big, 1.0)[2][0] == 2 and moments_reference(big, 2.0)[2][0] == 1
    assert np.array_equal(bits(mean[0]), bits((np.array([4, 4, 4 + 1e-42], np.float64) / 3).astype(f)))
    # no accepted sample, one accepted sample
    mean, var, cnt = moments_reference(np.array([[[np.nan] * 3] * 4, [[2, 4, 6]] + [[-1, 0, 0]] * 3], f), 1.0)
    assert list(cnt) == [0, 1] and list(var) == [0, 0] and np.array_equal(mean, [[0, 0, 0], [2, 4, 6]])
    # float64 sums: 1000 + noise of 1e-3 keeps its variance (a float32 S2 - S1^2 / N would return 0 or garbage)
    rng = np.random.RandomState(1)
    y = 1000.0 + rng.uniform(0, 1e-3, 64)
    x = np.repeat(y.astype(f)[None, :, None], 3, -1)
    _, var, _ = moments_reference(x, 1.0)
    yy = luma(x[0]).astype(np.float64)
    # (one-pass sums in float64: N additions into S2 and two roundings of S1 * S1 / N, each within 2^-53 of S2 — against a
    # two-pass variance that is exact to float64 rounding; a float32 S2 of 6.4e7 has a spacing of 4, the signal is 6e-6)
    bound = (64 + 2) * 2.0 ** -53 * float((yy * yy).sum()) / (63 * 64)
    assert bound < 0.1 * yy.var(ddof=1) / 64
    assert abs(float(var[0]) - yy.var(ddof=1) / 64) <= bound + 1e-7 * yy.var(ddof=1) / 64


def _build_sim(path, extra):
    return subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + extra +
                          ["-o", path, os.path.join(ROOT, "tests", "momentsim", "momentsim.cpp"),
                           os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def momentsim(built, tmp_path_factory):
    """tests/momentsim/momentsim.cpp: csrc/moments.hpp (and the path tracer's headers) compiled for the host."""
    exe = str(tmp_path_factory.mktemp("momentsim") / "momentsim")
    r = _build_sim(exe, ["-O2"])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_reduce(exe, tmp, n, spp, env=None):
    a = samples(n, spp)
    rec = np.zeros((n, spp, 4), np.float32)
    rec[..., :3] = a
    fin, fout = os.path.join(tmp, "m.in"), os.path.join(tmp, "m.out")
    with open(fin, "wb") as f:
        f.write(np.array([n, spp], np.uint32).tobytes() + np.array([EXPOSURE_SCALE], np.float32).tobytes() + rec.tobytes())
    r = subprocess.run([exe, "reduce", fin, fout], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        return r, None
    w = np.fromfile(fout, np.uint32).reshape(n, 5)
    return r, (np.ascontiguousarray(w[:, :3]).view(np.float32), np.ascontiguousarray(w[:, 3]).view(np.float32), np.ascontiguousarray(w[:, 4]))


def check_against_reference(got, n, spp, what):
    mean, var, cnt = reference(n, spp)
    assert np.array_equal(got[2], cnt), f"{what}: count"
    same_bits(got[0], mean, f"{what}: mean")
    same_bits(got[1], var, f"{what}: variance")
    check_all_equal(n, spp, got[1], got[2])


@pytest.mark.parametrize("n", [1, 65, 257])
def test_momentsim_equals_the_numpy_statement_on_bits(momentsim, tmp_path, n):
    """csrc/moments.hpp on the host == moments_reference, bit for bit, over the adversarial samples; all-equal samples give a
    variance that is never negative (and 0 where the arithmetic is exact)."""
    for spp in PROBE_SPP:
        r, got = run_reduce(momentsim, str(tmp_path), n, spp)
        assert r.returncode == 0, r.stderr
        check_against_reference(got, n, spp, f"momentsim {n} x {spp}")
    assert (reference(n, 65)[2] < 65).any() or n == 1, "the inputs must contain rejected samples"


def test_momentsim_is_clean_under_asan_and_ubsan(built, tmp_path_factory, tmp_path):
    """The same program with -fsanitize=address,undefined (host code only), once: no report, same bits."""
    exe = str(tmp_path_factory.mktemp("momentsim_san") / "momentsim_san")
    r = _build_sim(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here: " + r.stderr[-200:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r, got = run_reduce(exe, str(tmp_path), 65, 17, env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-800:]
    check_against_reference(got, 65, 17, "momentsim under sanitizers")


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("n", PROBE_PIXELS)
def test_probe_moments_equals_the_numpy_statement_on_bits(gpu_api, n):
    """k_moments_accumulate / k_moments_finish alone (api.probe_moments) == moments_reference, bit for bit, over the
    adversarial samples, as one launch and as launches of 1, 1, 2, 4, ... samples: the chunking changes nothing."""
    for spp in PROBE_SPP:
        whole = gpu_api.probe_moments(samples(n, spp), None, EXPOSURE_SCALE)
        check_against_reference(whole, n, spp, f"probe {n} x {spp}, one chunk")
        chunks = doubling_chunks(spp)
        assert sum(chunks) == spp and (spp < 4 or chunks[:3] == [1, 1, 2])
        parts = gpu_api.probe_moments(samples(n, spp), chunks, EXPOSURE_SCALE)
        check_against_reference(parts, n, spp, f"probe {n} x {spp}, chunks {chunks}")


def _triples(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return np.stack([xs, ys, ss], -1).reshape(-1, 3).astype(np.uint32)


def _scene(case):
    from yart_amd import scenes
    if case == "cornell":
        return scenes.cornell(32, 32, 16, 4)
    s, p = scenes.material_test(32, 24, 16, 6)
    return s, dict(p, exposure=2.0)              # an integer, non-zero exposure override: exposureScale = 4 exactly


_render_truth = {}


def render_truth(api, case):
    """(scene, params, expected moments from probe_samples, render_aovs' frame / buffers / stats), once per case"""
    if case not in _render_truth:
        from yart_amd.moments import moments_reference
        s, p = _scene(case)
        w, h = p["size"]
        scene = api.DeviceScene(s, device=0)
        rad, _ = scene.probe_samples(p, _triples(w, h, p["spp"]))
        scale = np.float32(2.0) ** np.float32(p.get("exposure", 0.0))
        exp = moments_reference(rad.reshape(h, w, p["spp"], 3), scale)
        frame, aovs, st = scene.render_aovs(p)
        _render_truth[case] = (scene, p, dict(mean=exp[0], variance=exp[1], count=exp[2]), frame, aovs, st)
    return _render_truth[case]


def check_moments(got, exp, what):
    assert set(got) == set(exp), what
    assert np.array_equal(got["count"], exp["count"]), f"{what}: count"
    same_bits(got["mean"], exp["mean"], f"{what}: mean")
    same_bits(got["variance"], exp["variance"], f"{what}: variance")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell", "material"])
def test_render_moments_vs_probe_samples_every_pipeline(gpu_api, case):
    """Every pixel: the moments of the render == moments_reference of the per-sample radiance DeviceScene.probe_samples gives
    for all (x, y, s), times float32(2 ** exposure) — for every pipeline flag set the golden tests vary (megakernel and path
    pool included), several batches, a wave schedule of 1, 1, 2, 4, 4, 4 samples, and each estimator. The frame, the ray and
    sample counts and the feature buffers are render_aovs' bits."""
    from tests.test_gpu_parity import PIPELINE_FLAGS
    api = gpu_api
    scene, p, exp, frame0, aovs0, st0 = render_truth(api, case)
    w, h = p["size"]
    assert (exp["count"] == p["spp"]).mean() > 0.9 and float(exp["variance"].max()) > 0.0

    def check(tag, q, flags=0, frame_too=True):
        frame, aovs, moms, st = scene.render_moments(q, aovs=api.AOV_ALL, flags=flags)
        check_moments(moms, exp, f"{case} / {tag}")
        for k in api.AOVS:
            same_bits(aovs[k], aovs0[k], f"{case} / {tag}: feature buffer {k}")
        assert st["rays"] == st0["rays"] and st["samples"] == st0["samples"]
        if frame_too:
            same_bits(frame, frame0, f"{case} / {tag}: frame")
        return st

    npaths = w * h * p["spp"]
    for name, flags in PIPELINE_FLAGS.items():
        check(name, p, flags)
    for name in ("wavefront", "megakernel", "wavefront+path_pool"):
        check(f"{name} / 5 batches", dict(p, max_batch_paths=npaths // 5 + 1), PIPELINE_FLAGS[name])
        # a first wave of one sample: waves of 1, 1, 2, 4, 4, 4 — a pixel's samples span six waves (the blended frame is another)
        st = check(f"{name} / doubling waves", dict(p, first_wave=1, max_wave=4), PIPELINE_FLAGS[name], frame_too=False)
        assert st["waves"] == 6
    check("doubling waves in 3 batches", dict(p, first_wave=1, max_wave=4, max_batch_paths=w * h * 4 // 3 + 1), frame_too=False)
    for est in (api.ESTIMATOR_GMON, api.ESTIMATOR_MEAN, api.ESTIMATOR_MON, api.ESTIMATOR_GMONB):
        check(f"estimator {est}", dict(p, estimator=est), frame_too=False)


@pytest.mark.gpu
def test_ranks_subsets_and_the_empty_mask(gpu_api):
    """rank / world_size 2: pixels of the other rank are 0, the two ranks' buffers add up to the unsharded ones. A subset of the
    moments without feature buffers; an empty mask is render_aovs."""
    api = gpu_api
    scene, p, exp, frame0, aovs0, st0 = render_truth(api, "material")
    p16 = dict(p, tile=16)
    _, _, full, _ = scene.render_moments(p16)        # (the sampler knows the tile size: other samples than `exp`'s, hence `full`)
    assert full["count"].shape == exp["count"].shape and float(full["variance"].max()) > 0.0
    acc = {k: np.zeros_like(v) for k, v in full.items()}
    owned = np.zeros(full["count"].shape, np.int32)
    for r in range(2):
        fr, _, part, _ = scene.render_moments(p16, rank=r, world_size=2)
        mine = fr[..., 3] == 1.0
        owned += mine
        for k, v in part.items():
            assert np.all(bits(v[~mine]) == 0), f"rank {r}: {k} written outside the rank's pixels"
            acc[k] = acc[k] + v
    assert np.all(owned == 1)
    check_moments(acc, full, "ranks 0 + 1")
    frame, none, some, st = scene.render_moments(p, moments=("variance",))
    assert none == {} and set(some) == {"variance"}
    same_bits(some["variance"], exp["variance"], "subset: variance")
    same_bits(frame, frame0, "subset: frame")
    frame, aovs, empty, st = scene.render_moments(p, moments=(), aovs=("normal", "ids"))
    assert empty == {} and st["rays"] == st0["rays"]
    same_bits(frame, frame0, "empty mask: frame")
    same_bits(aovs["normal"], aovs0["normal"], "empty mask: normal")
    assert np.array_equal(aovs["ids"], aovs0["ids"])


def child_render_moments_into():
    import torch
    from yart_amd import api
    s, p = _scene("cornell")
    scene = api.DeviceScene(s, device=0)
    frame, aovs, moms, st = scene.render_moments(p, aovs=("albedo", "depth"))
    dev = torch.device("cuda:0")
    t_frame = torch.zeros((32, 32, 4), dtype=torch.float32, device=dev)
    t_aovs = {"albedo": torch.full((32, 32, 3), 7, dtype=torch.float32, device=dev), "depth": torch.full((32, 32), 7, dtype=torch.float32, device=dev)}
    t_moms = {k: torch.full((32, 32, ch) if ch > 1 else (32, 32), 7, dtype=torch.float32 if dt == np.float32 else torch.int32, device=dev)
              for k, (bit, ch, dt) in api.MOMENTS.items()}
    sd = scene.render_moments_into(t_frame, t_aovs, t_moms, p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(t_frame.cpu().numpy()), bits(frame)), "frame"
    for k, t in t_aovs.items():
        assert np.array_equal(bits(t.cpu().numpy()), bits(aovs[k])), k
    for k, t in t_moms.items():
        assert np.array_equal(bits(t.cpu().numpy()), bits(moms[k])), k
    assert sd["rays"] == st["rays"]
    assert float(moms["variance"].max()) > 0
    scene.close()


@pytest.mark.gpu
def test_render_moments_into_torch_tensors(gpu_api):
    """render_moments_into (device tensors, torch's current stream) == the host-pointer form, bit for bit; in a process of its
    own that initialises torch's HIP runtime first, as bench.py does."""
    code = "import torch\ntorch.cuda.set_device(0)\nfrom tests import test_moments as t\nt.child_render_moments_into()\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
