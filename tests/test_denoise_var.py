"""The variance-guided à-trous filter (include/yart_hip.h: yart_hip_denoise_atrous_var_device / _host, YartDenoiseVarParams).

The definition is the header comment; yart_amd/denoise.py `atrous_var_reference` states it in NumPy float32 and is the
reference of every comparison here, with the machine's libm for expf / logf (tests/libmref.py) where the comparison is on
bits: csrc/denoise.hpp compiled for the host (tests/momentsim `denoisevar`) and the device kernels through api.denoise_var /
api.denoise_var_into / DeviceScene.render_denoised(variance_guided=True). The quality tests hold the default parameters to
"better than not denoising" and to "no worse than the plain filter at its defaults" on the frames of the golden scenes
(tests/golden/denoise/; the variance buffers are written by tools/denoise_var_sweep.py)."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT, bit_identical_or_drift
from tests.libmref import LibmRef
from tests.paramfile import load_params

CPU_SIZES = [(1, 1), (5, 3), (37, 23)]                  # (width, height)
GPU_SIZES = CPU_SIZES + [(131, 67)]                     # + several workgroups in both directions, no multiple of 16, 64 or 4
ITERATIONS = [1, 2, 5]
SIGMAS = dict(sigma_luma=3.0, sigma_normal=0.8, sigma_depth=1.5)       # weights neither all 1 nor all 0 on the random inputs
# a term whose sigma is <= 0 does not exist (run at 37 x 23, 2 iterations, all guides)
SIGMA_VARIANTS = [dict(sigma_luma=0.0, sigma_normal=0.8, sigma_depth=1.5), dict(sigma_luma=3.0, sigma_normal=0.0, sigma_depth=-1.0),
                  dict(sigma_luma=0.0, sigma_normal=0.0, sigma_depth=0.0), dict(sigma_luma=-2.0, sigma_normal=-0.5, sigma_depth=1.5)]
# (albedo, normal, depth, demodulate): every subset of the guides, demodulation on and off where there is an albedo
GUIDE_SETS = [(a, n, d, dm) for a, n, d in itertools.product((False, True), repeat=3) for dm in ((False, True) if a else (False,))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the reference, computed once per case and shared by the tests
# ---------------------------------------------------------------------------------------------------------------------
_inputs, _reference, _libm = {}, {}, []


def libm_fns(tmp_path_factory):
    if not _libm:
        ref = LibmRef(tmp_path_factory.mktemp("libm_dnv"))
        _libm.append((lambda x: ref.eval("expf", x).view(np.float32).reshape(np.shape(x)),
                      lambda x: ref.eval("logf", x).view(np.float32).reshape(np.shape(x))))
    return _libm[0]


def inputs(w, h):
    """The inputs of tests/test_denoise.py (seeded random HDR frame over [0, 50] with 1e4 fireflies, a NaN and an Inf; unit-ish
    normals; depths with zeros; albedo with exact zeros; a random alpha) plus a variance buffer: the variance of a mean of a few
    samples of such values (over [0, 40]), with exact zeros, huge values (1e30), and — where there are pixels enough — a NaN, a
    negative value and an Inf."""
    if (w, h) not in _inputs:
        rng = np.random.RandomState(1000 * w + h)
        n = w * h
        rgba = rng.uniform(0, 50, (h, w, 4)).astype(np.float32)
        rgba[..., 3] = rng.uniform(0, 1, (h, w))
        flat = rgba.reshape(n, 4)
        for k in rng.choice(n, n // 50, replace=False):
            flat[k, rng.randint(3)] = 1e4
        nrm = rng.normal(0, 1, (h, w, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) + rng.normal(0, 0.02, (h, w, 3))).astype(np.float32)
        depth = rng.uniform(0.1, 100, (h, w)).astype(np.float32)
        depth[rng.rand(h, w) < 0.05] = 0.0
        alb = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
        alb[rng.rand(h, w, 3) < 0.05] = 0.0
        var = (rng.uniform(0, 40, (h, w)) * rng.uniform(0, 1, (h, w)) ** 4).astype(np.float32)
        var[rng.rand(h, w) < 0.1] = 0.0
        var[rng.rand(h, w) < 0.03] = 1e30
        if n >= 8:
            flat[n // 3, 1] = np.nan
            flat[(2 * n) // 3, 0] = np.inf
            vf = var.reshape(n)
            vf[n // 5] = np.nan
            vf[(2 * n) // 5] = -1.0
            vf[(3 * n) // 5] = np.inf
            vf[n - 1] = 0.0
        _inputs[(w, h)] = dict(rgba=rgba, variance=var, albedo=alb, normal=nrm, depth=depth)
    return _inputs[(w, h)]


def guides_of(inp, a, n, d):
    return (inp["albedo"] if a else None, inp["normal"] if n else None, inp["depth"] if d else None)


def reference(tmp_path_factory, w, h, iterations, gs, sigmas=None):
    from yart_amd.denoise import atrous_var_reference
    sig = dict(SIGMAS if sigmas is None else sigmas)
    key = (w, h, iterations, gs, tuple(sorted(sig.items())))
    if key not in _reference:
        expf, logf = libm_fns(tmp_path_factory)
        a, n, d, dm = gs
        inp = inputs(w, h)
        out = atrous_var_reference(inp["rgba"], inp["variance"], *guides_of(inp, a, n, d), iterations=iterations, demodulate=dm,
                                   expf=expf, logf=logf, **sig)
        out.setflags(write=False)
        _reference[key] = out
    return _reference[key]


def grid(w, h):
    """(iterations, guide set, sigmas) of the size: the full grid, plus the sigma variants at 37 x 23."""
    cases = [(it, gs, None) for it in ITERATIONS for gs in GUIDE_SETS]
    if (w, h) == (37, 23):
        cases += [(2, (True, True, True, True), v) for v in SIGMA_VARIANTS]
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def test_denoise_var_abi_and_argument_errors(built, tmp_path):
    """Both symbols exist and are in api.EXPORTS, the ABI is still 3, YartDenoiseVarParams and the defaults agree between ctypes,
    yart_amd/denoise.py and a C++ compiler (which also sees yart::hip::denoiseVar), and every argument error is
    YART_E_INVALID with a telling message — no scene, no device."""
    from yart_amd import api, denoise
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in ("yart_hip_denoise_atrous_var_device", "yart_hip_denoise_atrous_var_host"):
        assert hasattr(raw, name), name
        assert name in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %u\\n\", sizeof(YartDenoiseVarParams), YART_DENOISE_VAR_DEFAULT_ITERATIONS);\n"
                "  std::printf(\"%.9g %.9g %.9g\\n\", YART_DENOISE_VAR_DEFAULT_SIGMA_LUMA, YART_DENOISE_VAR_DEFAULT_SIGMA_NORMAL, YART_DENOISE_VAR_DEFAULT_SIGMA_DEPTH);\n"
                "  std::vector<float> (*fn)(const std::vector<float>&, const std::vector<float>&, uint32_t, uint32_t, const yart::hip::DenoiseGuides&, const YartDenoiseVarParams&) = &yart::hip::denoiseVar;\n"
                "  return fn && yart::hip::denoiseVarDefaults().struct_size == sizeof(YartDenoiseVarParams) ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:2]] == [ctypes.sizeof(api.DenoiseVarParams), denoise.DEFAULT_VAR_ITERATIONS]
    assert ctypes.sizeof(api.DenoiseVarParams) == 24
    assert [np.float32(v) for v in out[2:]] == [np.float32(v) for v in (denoise.DEFAULT_VAR_SIGMA_LUMA, denoise.DEFAULT_VAR_SIGMA_NORMAL,
                                                                     denoise.DEFAULT_VAR_SIGMA_DEPTH)]
    # the existing structs are frozen
    assert ctypes.sizeof(api.DenoiseParams) == 24 and ctypes.sizeof(api.AovBuffers) == 8 + 7 * ctypes.sizeof(ctypes.c_void_p)

    buf = np.zeros((4, 4, 4), np.float32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)

    def call(device, rgba=ptr, variance=ptr, albedo=None, out=ptr, w=4, h=4, params=True, **over):
        dp = api.make_denoise_var_params()
        for k, v in over.items():
            setattr(dp, k, v)
        pp = ctypes.byref(dp) if params else None
        if device:
            return L.yart_hip_denoise_atrous_var_device(rgba, variance, albedo, None, None, w, h, pp, out, None)
        return L.yart_hip_denoise_atrous_var_host(rgba, variance, albedo, None, None, w, h, pp, out)

    for device in (False, True):
        for kw, word in ((dict(rgba=None), b"null"), (dict(out=None), b"null"), (dict(variance=None), b"variance"),
                         (dict(params=False), b"params"),
                         (dict(struct_size=20), b"struct_size"), (dict(struct_size=0), b"struct_size"),
                         (dict(iterations=9), b"iterations"), (dict(w=0), b"width"), (dict(h=0), b"height"),
                         (dict(sigma_luma=float("nan")), b"sigma"), (dict(sigma_normal=float("inf")), b"sigma"),
                         (dict(sigma_depth=float("-inf")), b"sigma"), (dict(flags=2), b"flags"), (dict(flags=1 | 0x80000000), b"flags"),
                         (dict(flags=api.FLAG_DEMODULATE), b"albedo")):
            assert call(device, **kw) == api.YART_E_INVALID, (device, kw)
            assert word in L.yart_hip_last_error(), (device, kw, L.yart_hip_last_error())
        if L.yart_hip_device_count() == 0:             # well-formed arguments, no device: that, and nothing else
            assert call(device) == api.YART_E_NO_DEVICE
            assert call(device, albedo=ptr, flags=api.FLAG_DEMODULATE) == api.YART_E_NO_DEVICE


def test_numpy_statement_on_hand_made_inputs():
    """atrous_var_reference on inputs whose answer is known without running it."""
    from yart_amd.denoise import atrous_var_reference
    f = np.float32
    rng = np.random.RandomState(6)
    # iterations = 0: the input bits
    x = rng.uniform(0, 9, (6, 7, 4)).astype(f)
    v = rng.uniform(0, 1, (6, 7)).astype(f)
    assert np.array_equal(bits(atrous_var_reference(x, v, iterations=0)), bits(x))
    # a constant frame stays constant (to rounding), whatever the variance
    c = np.full((9, 11, 4), 2.5, f)
    out = atrous_var_reference(c, v[:1, :1].repeat(9, 0).repeat(11, 1), iterations=3)
    assert np.allclose(out, c, rtol=1e-6)
    # variance 0 everywhere: the colour term is |dl| / 1e-6 — any visible difference closes the weight; the frame is kept
    step = rng.uniform(1, 5, (8, 8, 4)).astype(f)
    out = atrous_var_reference(step, np.zeros((8, 8), f), iterations=3, sigma_luma=4.0)
    assert np.allclose(out[..., :3], step[..., :3], rtol=1e-5)
    # a large variance everywhere opens the colour term: the filter averages (the spread of the frame shrinks)
    out = atrous_var_reference(step, np.full((8, 8), 1e6, f), iterations=3, sigma_luma=4.0)
    assert out[..., :3].std() < 0.5 * step[..., :3].std()
    # a pixel whose variance is NaN or negative is absent: filled from its neighbours, and no tap of anyone's
    vv = np.full((9, 9), 0.5, f)
    img = rng.uniform(1, 5, (9, 9, 4)).astype(f)
    a, b = vv.copy(), vv.copy()
    a[4, 4], b[4, 4] = np.nan, -3.0
    oa, ob = atrous_var_reference(img, a, iterations=3), atrous_var_reference(img, b, iterations=3)
    assert np.isfinite(oa).all() and np.array_equal(bits(oa), bits(ob))
    bad = img.copy()
    bad[4, 4, 1] = np.inf                                 # ... the same as a pixel whose colour is not finite
    assert np.array_equal(bits(atrous_var_reference(bad, vv, iterations=3)), bits(oa))
    assert np.array_equal(oa[..., 3], img[..., 3])


def _build_sim(path, extra):
    return subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + extra +
                          ["-o", path, os.path.join(ROOT, "tests", "momentsim", "momentsim.cpp"),
                           os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def momentsim(built, tmp_path_factory):
    """tests/momentsim/momentsim.cpp: csrc/denoise.hpp's variance-guided statement compiled for the host."""
    exe = str(tmp_path_factory.mktemp("momentsim_dn") / "momentsim")
    r = _build_sim(exe, ["-O2"])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_sim_on(cmd, tmp, inp, w, h, iterations, gs, sigmas3, in_place, env=None):
    """Writes the 9-word header, the frame, inp["variance"] if there is one and the guides of `gs`, runs `cmd <in> <out>`."""
    a, n, d, dm = gs
    head = np.array([w, h, iterations, 1 if dm else 0, (1 if a else 0) | (2 if n else 0) | (4 if d else 0), 1 if in_place else 0], np.uint32)
    fin, fout = os.path.join(tmp, "dn.in"), os.path.join(tmp, "dn.out")
    with open(fin, "wb") as f:
        f.write(head.tobytes())
        f.write(np.array(sigmas3, np.float32).tobytes())
        f.write(inp["rgba"].tobytes())
        if "variance" in inp:
            f.write(inp["variance"].tobytes())
        for g in guides_of(inp, a, n, d):
            if g is not None:
                f.write(g.tobytes())
    r = subprocess.run(cmd + [fin, fout], capture_output=True, text=True, env=env)
    return r, (np.fromfile(fout, np.float32).reshape(h, w, 4) if r.returncode == 0 else None)


def run_sim(exe, tmp, w, h, iterations, gs, sigmas, in_place, env=None):
    sig = dict(SIGMAS if sigmas is None else sigmas)
    return run_sim_on([exe, "denoisevar"], tmp, inputs(w, h), w, h, iterations, gs,
                      [sig["sigma_luma"], sig["sigma_normal"], sig["sigma_depth"]], in_place, env)


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_equals_the_numpy_statement_on_bits(momentsim, tmp_path_factory, tmp_path, w, h):
    """csrc/denoise.hpp (dnPrepare<true> / dnFilterPixel<true>) on the host == atrous_var_reference with libm's expf / logf, bit for
    bit: every iteration count, guide subset, demodulation on / off, out of place and in place; the sigma variants that drop terms."""
    for it, gs, sig in grid(w, h):
        want = reference(tmp_path_factory, w, h, it, gs, sig)
        assert w * h < 8 or np.isfinite(want).all()
        for in_place in (False, True):
            r, got = run_sim(momentsim, str(tmp_path), w, h, it, gs, sig, in_place)
            assert r.returncode == 0, r.stderr
            diff = bits(got) != bits(want)
            assert not diff.any(), (f"{w}x{h} iterations {it} guides {gs} sigmas {sig} in_place {in_place}: {int(diff.sum())} words "
                                    f"differ, first at {np.argwhere(diff)[0].tolist()}")


def test_variance_changes_the_result(tmp_path_factory):
    """The variance buffer is really read: another buffer gives another frame, and the sigma_luma <= 0 variant ignores its values
    (but not which pixels it invalidates)."""
    from yart_amd.denoise import atrous_var_reference
    inp = inputs(37, 23)
    base = reference(tmp_path_factory, 37, 23, 2, (False, False, False, False))
    other = atrous_var_reference(inp["rgba"], np.where(np.isfinite(inp["variance"]) & (inp["variance"] >= 0), inp["variance"] * 9, inp["variance"]),
                                 iterations=2, **SIGMAS)
    assert not np.array_equal(bits(other), bits(base))
    off = dict(SIGMAS, sigma_luma=0.0)
    a = atrous_var_reference(inp["rgba"], inp["variance"], iterations=2, **off)
    b = atrous_var_reference(inp["rgba"], np.where(np.isfinite(inp["variance"]) & (inp["variance"] >= 0), np.float32(1.0), inp["variance"]),
                             iterations=2, **off)
    assert np.array_equal(bits(a), bits(b))


# -- the two forms against each other ------------------------------------------------------------------------------------
# With the colour term off and every variance finite and non-negative, the variance changes neither which pixels are valid nor
# any weight: the plain and the variance-guided filter return the same bits. Every other test holds a form to its own NumPy
# statement; this one holds the two instantiations of the shared body (csrc/denoise.hpp) to each other.
SAME_SIZES = [(5, 3), (37, 23)]
SAME_GUIDES = (True, True, True, True)                  # all three guides, demodulated
SAME_PLAIN = dict(sigma_color=0.0, sigma_normal=0.8, sigma_depth=1.5)
SAME_VAR = dict(sigma_luma=-1.0, sigma_normal=0.8, sigma_depth=1.5)
_same_inputs = {}


def same_inputs(w, h):
    """inputs(w, h) with one NaN in the frame (its Inf made finite) and every variance that is not finite or is negative made an
    exact zero; the albedo keeps its exact zeros."""
    if (w, h) not in _same_inputs:
        inp = {k: v.copy() for k, v in inputs(w, h).items()}
        inp["rgba"][np.isinf(inp["rgba"])] = 7.0
        bad = ~np.isfinite(inp["variance"]) | (inp["variance"] < 0)
        inp["variance"][bad] = 0.0
        assert np.isnan(inp["rgba"]).sum() == 1 and np.isfinite(inp["variance"]).all() and (inp["variance"] >= 0).all()
        assert (inp["variance"] == 0).any() and (inp["variance"] > 0).any() and (inp["albedo"] == 0).any()
        for v in inp.values():
            v.setflags(write=False)
        _same_inputs[(w, h)] = inp
    return _same_inputs[(w, h)]


def assert_same_bits(plain, var, what):
    diff = bits(plain) != bits(var)
    assert not diff.any(), f"{what}: {int(diff.sum())} words differ, first at {np.argwhere(diff)[0].tolist()}"
    assert np.isfinite(plain).all()


@pytest.mark.parametrize("w,h", SAME_SIZES)
def test_forms_agree_without_a_colour_term_numpy(w, h):
    from yart_amd.denoise import atrous_reference, atrous_var_reference
    inp = same_inputs(w, h)
    guides = guides_of(inp, True, True, True)
    for it in ITERATIONS:
        plain = atrous_reference(inp["rgba"], *guides, iterations=it, demodulate=True, **SAME_PLAIN)
        var = atrous_var_reference(inp["rgba"], inp["variance"], *guides, iterations=it, demodulate=True, **SAME_VAR)
        assert_same_bits(plain, var, f"NumPy statements {w}x{h} iterations {it}")
        assert not np.array_equal(bits(plain), bits(inp["rgba"]))


@pytest.fixture(scope="module")
def denoisesim(tmp_path_factory):
    """tests/denoisesim/denoisesim.cpp: csrc/denoise.hpp's plain statement compiled for the host."""
    exe = str(tmp_path_factory.mktemp("denoisesim_dnv") / "denoisesim")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", "-o", exe, os.path.join(ROOT, "tests", "denoisesim", "denoisesim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("w,h", SAME_SIZES)
def test_forms_agree_without_a_colour_term_host(denoisesim, momentsim, tmp_path, w, h):
    inp = same_inputs(w, h)
    no_variance = {k: v for k, v in inp.items() if k != "variance"}
    for it in ITERATIONS:
        rp, plain = run_sim_on([denoisesim], str(tmp_path), no_variance, w, h, it, SAME_GUIDES, list(SAME_PLAIN.values()), False)
        rv, var = run_sim_on([momentsim, "denoisevar"], str(tmp_path), inp, w, h, it, SAME_GUIDES, list(SAME_VAR.values()), False)
        assert rp.returncode == 0 and rv.returncode == 0, rp.stderr + rv.stderr
        assert_same_bits(plain, var, f"denoisesim / momentsim denoisevar {w}x{h} iterations {it}")


# -- quality: the gates of the default parameters ----------------------------------------------------------------------
def host_tonemap(hostsim, tmp, frame):
    h, w = frame.shape[:2]
    src, dst = os.path.join(tmp, "t.in"), os.path.join(tmp, "t.out")
    np.ascontiguousarray(frame, np.float32).tofile(src)
    subprocess.run([hostsim, "tonemap", src, str(w), str(h), "none", dst, os.path.join(tmp, "t.ppm")], check=True)
    return np.fromfile(dst, np.float32).reshape(h, w, 4)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


@pytest.mark.parametrize("name,w,h", [("cornell", 96, 96), ("material", 96, 64)])
def test_default_parameters_beat_not_denoising_and_the_plain_filter(hostsim, tmp_path, name, w, h):
    """tests/golden/denoise/: the host path tracer's frame of the golden scene at 16 spp and at 1024 spp, the 16-spp frame's guides
    (tools/denoise_sweep.py) and the variance of those same 16 samples per pixel (tools/denoise_var_sweep.py, which asserts that
    its frame is <scene>_lo.f32 on bits). At the defaults the filtered 16-spp frame is strictly closer to the 1024-spp frame than
    the unfiltered one — RMSE over the AgX-tonemapped frames — and, the sweep having found such defaults
    (profiles/denoise_var_sweep.txt), no further from it than the plain filter's at its defaults (atrous_reference, in this run)."""
    from yart_amd.denoise import atrous_reference, atrous_var_reference
    d = os.path.join(GOLDEN, "denoise")
    load = lambda key, *shape: np.fromfile(os.path.join(d, f"{name}_{key}.f32"), np.float32).reshape(h, w, *shape)
    lo, hi, var = load("lo", 4), load("hi", 4), load("var")
    assert np.isfinite(var).all() and (var >= 0).all() and var.max() > 0
    guides = (load("albedo", 3), load("normal", 3), load("depth"))
    out = atrous_var_reference(lo, var, *guides)
    plain = atrous_reference(lo, *guides)
    tm = lambda x: host_tonemap(hostsim, str(tmp_path), x)
    ref = tm(hi)
    noisy, clean, clean_plain = rmse(tm(lo), ref), rmse(tm(out), ref), rmse(tm(plain), ref)
    print(f"{name}: RMSE noisy {noisy:.5f}, variance-guided {clean:.5f} (ratio {clean / noisy:.4f}), plain {clean_plain:.5f} "
          f"(ratio {clean_plain / noisy:.4f})")
    assert clean < noisy
    assert clean <= clean_plain


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


def device_denoise(api, w, h, it, gs, sig, in_place):
    a, n, d, dm = gs
    inp = inputs(w, h)
    frame = inp["rgba"].copy()
    got = api.denoise_var(frame, inp["variance"], *guides_of(inp, a, n, d), iterations=it, demodulate=dm,
                          out=frame if in_place else None, **dict(SIGMAS if sig is None else sig))
    if not in_place:
        assert np.array_equal(bits(frame), bits(inp["rgba"]))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_denoise_var_equals_the_numpy_statement_on_bits(gpu_api, tmp_path_factory, w, h):
    """k_dn_prepare<true> / k_dn_atrous<true, 0 and 1> / k_dn_finish through api.denoise_var == atrous_var_reference with libm's expf /
    logf, bit for bit, over the grid of the host test, out of place and with `out` aliasing the input frame."""
    for it, gs, sig in grid(w, h):
        want = reference(tmp_path_factory, w, h, it, gs, sig)
        for in_place in (False, True):
            got = device_denoise(gpu_api, w, h, it, gs, sig, in_place)
            bit_identical_or_drift(got, want, f"denoise_var {w}x{h} iterations {it} guides {gs} sigmas {sig} in_place {in_place}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SAME_SIZES)
def test_forms_agree_without_a_colour_term_device(gpu_api, w, h):
    inp = same_inputs(w, h)
    guides = guides_of(inp, True, True, True)
    for it in ITERATIONS:
        plain = gpu_api.denoise(inp["rgba"], *guides, iterations=it, demodulate=True, **SAME_PLAIN)
        var = gpu_api.denoise_var(inp["rgba"], inp["variance"], *guides, iterations=it, demodulate=True, **SAME_VAR)
        assert_same_bits(plain, var, f"api.denoise / api.denoise_var {w}x{h} iterations {it}")


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_denoise_var as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_denoise_var_into():
    import torch
    from yart_amd import api
    for w, h in GPU_SIZES:
        inp = inputs(w, h)
        dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in inp.items()}
        for it, gs in ((2, (True, True, True, True)), (5, (False, True, True, False)), (1, (False, False, False, False))):
            a, n, d, dm = gs
            want = api.denoise_var(inp["rgba"], inp["variance"], *guides_of(inp, a, n, d), iterations=it, demodulate=dm, **SIGMAS)
            guides = {k: dev[k] for k, on in (("albedo", a), ("normal", n), ("depth", d)) if on}
            out = torch.zeros_like(dev["rgba"])
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                api.denoise_var_into(out, dev["rgba"], dev["variance"], guides, iterations=it, demodulate=dm, **SIGMAS)
                assert np.array_equal(bits(out.cpu().numpy()), bits(want)), f"{w}x{h} {gs}: out of place on a side stream"
                for k, v in inp.items():
                    assert np.array_equal(bits(dev[k].cpu().numpy()), bits(v)), k + " was written"
                frame = dev["rgba"].clone()
                api.denoise_var_into(frame, frame, dev["variance"], guides, iterations=it, demodulate=dm, **SIGMAS)      # in place
                assert np.array_equal(bits(frame.cpu().numpy()), bits(want)), f"{w}x{h} {gs}: in place on a side stream"


@pytest.mark.gpu
def test_denoise_var_into_equals_the_host_form(gpu_api):
    """api.denoise_var_into on torch tensors, on a non-default stream, at every size: the bits of api.denoise_var (itself held
    to the NumPy statement above); inputs untouched when out != in; in place too."""
    run_torch_child("child_denoise_var_into()")


def child_render_denoised():
    from yart_amd import api
    p = dict(load_params(os.path.join(GOLDEN, "cornell.txt")), size=(64, 64))
    scene = api.DeviceScene(os.path.join(GOLDEN, "cornell.yscn"), device=0)
    frame, aovs, moms, _ = scene.render_moments(p, ("variance",), ("albedo", "normal", "depth"))
    noisy, clean, guides = scene.render_denoised(p, variance_guided=True)
    assert np.array_equal(bits(noisy.cpu().numpy()), bits(frame)), "noisy frame"
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(bits(guides[k].cpu().numpy()), bits(aovs[k])), k
    assert np.array_equal(bits(guides["variance"].cpu().numpy()), bits(moms["variance"])), "variance"
    want = api.denoise_var(frame, moms["variance"], aovs["albedo"], aovs["normal"], aovs["depth"], demodulate=True)
    assert np.array_equal(bits(clean.cpu().numpy()), bits(want)), "denoised frame"
    assert not np.array_equal(bits(want), bits(frame))
    # the default argument: today's result, i.e. render_aovs then the plain filter at its defaults
    noisy0, clean0, guides0 = scene.render_denoised(p)
    assert set(guides0) == {"albedo", "normal", "depth"}
    assert np.array_equal(bits(noisy0.cpu().numpy()), bits(frame))
    want0 = api.denoise(frame, aovs["albedo"], aovs["normal"], aovs["depth"], demodulate=True)
    assert np.array_equal(bits(clean0.cpu().numpy()), bits(want0)), "plain denoised frame"
    assert not np.array_equal(bits(want0), bits(want))
    scene.close()


@pytest.mark.gpu
def test_render_denoised_variance_guided(gpu_api):
    """DeviceScene.render_denoised(variance_guided=True) on cornell.yscn at 64 x 64 == render_moments followed by denoise_var, bit
    for bit; with the default argument it is render_aovs followed by the plain filter, as before."""
    run_torch_child("child_render_denoised()")
