"""The moments form of the temporal accumulator — SVGF's variance estimation (include/yart_hip.h:
yart_hip_temporal_accumulate_moments_*, YartTemporalMomentParams).

The definition is the header comment; yart_amd/temporal.py `temporal_moments_reference` states both passes in NumPy float32 and
is the reference of every comparison here, on bits: csrc/temporal.hpp compiled for the host (tests/temporalsim
temporalsim_moments.cpp) and the device kernels k_tp_accumulate<true> + k_tp_spatial_variance through
api.TemporalAccumulator(moments=True). Scene, cameras and frames are those of tests/test_temporal.py. Beyond reproducibility:
the estimate is held to the empirical variance of the accumulated luminance on iid noise, and the chain moments form ->
variance-guided filter to "better than the plain form" at 1 spp, where the plain form's variance is all zero."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_temporal as tt
from tests.conftest import GOLDEN, ROOT, bit_identical_or_drift
from tests.paramfile import load_params

bits, assert_same = tt.bits, tt.assert_same
CPU_SIZES, GPU_SIZES, SEQUENCES, FRAMES = tt.CPU_SIZES, tt.GPU_SIZES, tt.SEQUENCES, tt.FRAMES
# test_temporal.PARAMS with the cap at 8, so that the length grows to 3, and the smallest min_moment_history: three frames reach
# the temporal estimate (N >= 2) and the spatial one
PARAMS = dict(alpha_min=0.2, max_history=8, normal_cos_min=0.95, plane_tolerance=0.01, min_moment_history=2)
LONG_FRAMES = 5                                          # the sequence at the default min_moment_history
LONG_PARAMS = dict(alpha_min=0.1, max_history=8, normal_cos_min=0.95, plane_tolerance=0.01, min_moment_history=4)

_reference = {}


def long_frames(w, h):
    """Five frames of the sub-pixel pan of test_temporal: its three, then the same three inputs seen from two further cameras
    (the feature buffers of frame k are those of camera k, so only a static or a repeated camera can reuse them: frames 3 and
    4 repeat cameras 1 and 2, a pan back)."""
    f = tt.frames_of(w, h, "subpixel")
    return [f[0], f[1], f[2], f[1], f[2]]


def frames_of(w, h, seq):
    return long_frames(w, h) if seq == "long" else tt.frames_of(w, h, seq)


def params_of(seq):
    return LONG_PARAMS if seq == "long" else PARAMS


def reference(w, h, seq, demodulate):
    """temporal_moments_reference over the sequence -> [(frame, variance, length)] per frame and the history's moments, once"""
    from yart_amd.temporal import TemporalHistory, temporal_moments_reference
    key = (w, h, seq, demodulate)
    if key not in _reference:
        hist = TemporalHistory(w, h)
        res, info = [], []
        for k, f in enumerate(frames_of(w, h, seq)):
            if seq == "reset" and k == 2:
                hist.reset()
            r = temporal_moments_reference(hist, f["camera"], f["rgba"], f["variance"], f["position"], f["normal"], f["depth"],
                                           f["coverage"], f["ids"], f["albedo"] if demodulate else None, demodulate=demodulate,
                                           **params_of(seq))
            for v in r:
                v.setflags(write=False)
            res.append(r)
            info.append(hist.moments.copy())
        _reference[key] = (res, info)
    return _reference[key][0]


def classes(w, h, seq, demodulate, k):
    """(temporal estimate, spatial estimate with k >= 2, short with k < 2) masks of frame k, from the NumPy statement's outputs:
    a pixel is long iff N >= min_moment_history and w2 < 1; a short pixel was spatially estimated iff its variance is not the
    propagated one. Counted here again, independently of the statement's own loop."""
    res = reference(w, h, seq, demodulate)
    m = _reference[(w, h, seq, demodulate)][1][k]
    ln = res[k][2]
    usable = ln >= 1
    long_ = usable & (ln >= params_of(seq)["min_moment_history"]) & (m[..., 2] < 1)
    fr = frames_of(w, h, seq)[k]
    node = np.where(usable, fr["ids"][..., 0], 0)
    n, P = np.where(usable[..., None], fr["normal"], 0).astype(np.float32), np.where(usable[..., None], fr["position"], 0).astype(np.float32)
    prm = params_of(seq)
    cnt = np.zeros((h, w), int)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    with np.errstate(all="ignore"):
        tol = np.float32(prm["plane_tolerance"]) * fr["depth"]
        for y in range(h):
            for x in range(w):
                y0, y1, x0, x1 = max(0, y - 3), min(h, y + 4), max(0, x - 3), min(w, x + 4)
                ok = usable[y0:y1, x0:x1] & (node[y0:y1, x0:x1] == node[y, x])
                ok &= dot(n[y, x], n[y0:y1, x0:x1]) >= np.float32(prm["normal_cos_min"])
                ok &= np.abs(dot(n[y, x], (P[y0:y1, x0:x1] - P[y, x]).astype(np.float32))) <= tol[y, x]
                cnt[y, x] = ok.sum()
    short = usable & ~long_
    return long_, short & (cnt >= 2), short & (cnt < 2)


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
MOMENT_SYMBOLS = ("yart_hip_temporal_accumulate_moments_device", "yart_hip_temporal_accumulate_moments_host")


def test_moments_abi_and_argument_errors(built, tmp_path):
    """The two symbols exist and are in api.EXPORTS, the ABI is still 3 and YartTemporalParams still 24 bytes;
    YartTemporalMomentParams and its default agree between ctypes, yart_amd/temporal.py and a C++ compiler (which also sees
    yart::hip::Temporal::accumulateMoments and temporalMomentDefaults); every argument error of the plain call, and
    min_moment_history 0 and 1, is YART_E_INVALID with a telling message and no device touched."""
    from yart_amd import api, temporal
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in MOMENT_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    assert ctypes.sizeof(api.TemporalParams) == 24
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %u %zu\\n\", sizeof(YartTemporalMomentParams), YART_TEMPORAL_DEFAULT_MIN_MOMENT_HISTORY, sizeof(YartTemporalParams));\n"
                "  yart::hip::Temporal t(4, 4);\n"
                "  yart::hip::TemporalFrame (yart::hip::Temporal::*fn)(const YartCameraDesc&, const std::vector<float>&, const std::vector<float>&, const yart::hip::TemporalFeatures&, const YartTemporalMomentParams&) = &yart::hip::Temporal::accumulateMoments;\n"
                "  const YartTemporalMomentParams d = yart::hip::temporalMomentDefaults(true);\n"
                "  return fn && d.struct_size == sizeof(YartTemporalMomentParams) && d.flags == YART_TEMPORAL_DEMODULATE\n"
                "    && d.min_moment_history == YART_TEMPORAL_DEFAULT_MIN_MOMENT_HISTORY && d.max_history == YART_TEMPORAL_DEFAULT_MAX_HISTORY ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.TemporalMomentParams), temporal.DEFAULT_MIN_MOMENT_HISTORY, 24]
    assert ctypes.sizeof(api.TemporalMomentParams) == 28 and temporal.DEFAULT_MIN_MOMENT_HISTORY == 4
    tp = api.make_temporal_moment_params()
    assert (tp.struct_size, tp.max_history, tp.min_moment_history, tp.flags) == (28, temporal.DEFAULT_MAX_HISTORY, 4, 0)
    assert api.make_temporal_moment_params(min_moment_history=2, demodulate=True).flags == api.FLAG_TEMPORAL_DEMODULATE

    h = ctypes.c_void_p()
    assert L.yart_hip_temporal_create(4, 4, 0, ctypes.byref(h)) == api.YART_OK and h.value
    buf = np.zeros((4, 4, 4), np.float32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    cam_ok = api.make_camera(tt.base_camera(4, 4))
    needed = ("position", "normal", "depth", "coverage", "ids")

    def call(device, handle=h, cam=cam_ok, rgba=ptr, variance=ptr, aovs=needed, aov_null=None, aov_size=None, have_aovs=True,
             out=ptr, params=True, plain=False, **over):
        tp = api.make_temporal_params() if plain else api.make_temporal_moment_params()
        for k, v in over.items():
            setattr(tp, k, v)
        ab = api.AovBuffers()
        ab.struct_size = ctypes.sizeof(api.AovBuffers) if aov_size is None else aov_size
        for name in aovs:
            ab.mask |= api.AOVS[name][0]
            setattr(ab, name, None if name == aov_null else ptr)
        pc = None if cam is None else ctypes.byref(cam)
        pa = ctypes.byref(ab) if have_aovs else None
        pp = ctypes.byref(tp) if params else None
        if plain:
            fn = L.yart_hip_temporal_accumulate_device if device else L.yart_hip_temporal_accumulate_host
        else:
            fn = L.yart_hip_temporal_accumulate_moments_device if device else L.yart_hip_temporal_accumulate_moments_host
        return fn(handle, pc, rgba, variance, pa, pp, out, None, None, None) if device else fn(handle, pc, rgba, variance, pa, pp, out, None, None)

    cam_size = api.make_camera(tt.base_camera(5, 4))
    cases = [(dict(handle=None), b"handle"), (dict(cam=None), b"camera"), (dict(rgba=None), b"null"), (dict(out=None), b"null"),
             (dict(variance=None), b"variance"), (dict(have_aovs=False), b"aovs"), (dict(params=False), b"params"),
             (dict(struct_size=24), b"struct_size"), (dict(struct_size=0), b"struct_size"),
             (dict(flags=2), b"flags"), (dict(flags=1 | 0x80000000), b"flags"),
             (dict(alpha_min=float("nan")), b"finite"), (dict(normal_cos_min=float("inf")), b"finite"),
             (dict(plane_tolerance=float("-inf")), b"finite"), (dict(alpha_min=-0.01), b"alpha_min"), (dict(alpha_min=1.5), b"alpha_min"),
             (dict(max_history=0), b"max_history"), (dict(min_moment_history=0), b"min_moment_history"),
             (dict(min_moment_history=1), b"min_moment_history"), (dict(cam=cam_size), b"size"),
             (dict(flags=api.FLAG_TEMPORAL_DEMODULATE), b"albedo"), (dict(aov_size=4), b"struct_size"),
             (dict(aovs=needed + ("albedo",), aov_size=16, flags=0), b"missing")]
    cases += [(dict(aovs=tuple(n for n in needed if n != miss)), miss.encode()) for miss in needed]
    cases += [(dict(aov_null=miss), miss.encode()) for miss in needed]
    for device in (False, True):
        for kw, word in cases:
            assert call(device, **kw) == api.YART_E_INVALID, (device, kw)
            assert word in L.yart_hip_last_error(), (device, kw, L.yart_hip_last_error())
        if L.yart_hip_device_count() == 0:
            # well-formed arguments, no device: that, and nothing else — in either form and in either order on one handle (a
            # call that failed leaves the handle in no form); the refusal of a mixed handle is the GPU suite's
            assert call(device) == api.YART_E_NO_DEVICE
            assert call(device, min_moment_history=2, aovs=needed + ("albedo",), flags=api.FLAG_TEMPORAL_DEMODULATE) == api.YART_E_NO_DEVICE
            assert call(device, plain=True) == api.YART_E_NO_DEVICE
            assert call(device) == api.YART_E_NO_DEVICE
    L.yart_hip_temporal_destroy(h)
    # the Python layer: the accumulator's form decides the parameter struct
    acc = api.TemporalAccumulator(4, 4, moments=True, min_moment_history=3)
    assert isinstance(acc._params(False, {}), api.TemporalMomentParams) and acc._params(False, {}).min_moment_history == 3
    assert acc._params(True, dict(min_moment_history=5)).min_moment_history == 5
    acc.close()
    acc = api.TemporalAccumulator(4, 4)
    assert isinstance(acc._params(False, {}), api.TemporalParams)
    with pytest.raises(AssertionError):
        acc._params(False, dict(min_moment_history=2))
    acc.close()


def run_hand(hist, cam, fr, **kw):
    from yart_amd.temporal import temporal_moments_reference
    return temporal_moments_reference(hist, cam, fr["rgba"], fr["variance"], fr["position"], fr["normal"], fr["depth"], fr["coverage"],
                                      fr["ids"], fr.get("albedo"), **kw)


def luma(c):
    f = np.float32
    return (f(c) * f(0.2126) + f(c) * f(0.7152)) + f(c) * f(0.0722)


def test_numpy_statement_on_hand_made_inputs():
    """temporal_moments_reference on 1- and 2-pixel frames whose answer is worked out by hand, in float32."""
    from yart_amd.temporal import TemporalHistory
    f = np.float32
    cam = tt.hand_camera(1)
    kw = dict(alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01, min_moment_history=2)
    y8, y4, y9 = luma(8), luma(4), luma(9)
    assert y8 == 8 and y4 == 4                           # the luma weights sum to 1.0f, and 8 and 4 only shift the exponent
    # frame 1, grey 8: m = (8, 64), w2 = 1, N = 1: short; the window holds the pixel alone (k = 1): the propagated value, v = 2
    hist = TemporalHistory(1, 1)
    out, var, ln = run_hand(hist, cam, tt.hand_frame(1, 8.0, 2.0, [0.0]), **kw)
    assert out[0, 0].tolist() == [8, 8, 8, 0.25] and ln[0, 0] == 1 and var[0, 0] == 2 and hist.variance[0, 0] == 2
    assert hist.moments[0, 0].tolist() == [8, 64, 1]
    # frame 2, grey 4: N = 2, a = 1/2: m1 = 8 + (4 - 8) / 2 = 6, m2 = 64 + (16 - 64) / 2 = 40, w2 = 1/4 + 1/4 = 1/2
    # vt = 40 - 36 = 4; N >= 2 and w2 < 1: v_acc = 4 * ((1/2) / (1/2)) = 4 = vt / (N - 1). The input variance 4 plays no part.
    out, var, ln = run_hand(hist, cam, tt.hand_frame(1, 4.0, 4.0, [0.0]), **kw)
    assert out[0, 0].tolist() == [6, 6, 6, 0.25] and ln[0, 0] == 2 and var[0, 0] == 4 and hist.variance[0, 0] == 4
    assert hist.moments[0, 0].tolist() == [6, 40, 0.5]
    # frame 3, grey 9: N = 3, a = float32(1 / 3)
    a = f(1) / f(3)
    b = f(1) - a
    m1 = f(6) + a * (y9 - f(6))
    m2 = f(40) + a * (y9 * y9 - f(40))
    w2 = (a * a) * f(1) + (b * b) * f(0.5)
    vt = m2 - m1 * m1
    want = vt * (w2 / (f(1) - w2))
    out, var, ln = run_hand(hist, cam, tt.hand_frame(1, 9.0, 0.0, [0.0]), **kw)
    assert ln[0, 0] == 3 and out[0, 0, 0] == f(6) + a * (f(9) - f(6))
    assert np.array_equal(bits(hist.moments[0, 0]), bits(np.array([m1, m2, w2], f)))
    assert bits(var)[0, 0] == bits(np.array([want], f))[0] and vt > 0
    assert abs(float(w2) - 1 / 3) < 1e-6 and abs(float(want) - (64 + 16 + 81 - 3 * 7.0 ** 2) / 3 / 2) < 1e-4   # 1/N; s^2 / (N - 1)
    # the alpha_min floor changes w2 and not N: the same third frame with alpha_min = 0.75:
    # w2 = 0.5625 + 0.0625 / 2 = 0.59375; m1 = 6 + 0.75 * (y9 - 6); v_acc = vt * (0.59375 / 0.40625)
    hist = TemporalHistory(1, 1)
    run_hand(hist, cam, tt.hand_frame(1, 8.0, 2.0, [0.0]), **kw)
    run_hand(hist, cam, tt.hand_frame(1, 4.0, 4.0, [0.0]), **kw)
    out, var, ln = run_hand(hist, cam, tt.hand_frame(1, 9.0, 0.0, [0.0]), **dict(kw, alpha_min=0.75))
    m1 = f(6) + f(0.75) * (y9 - f(6))
    m2 = f(40) + f(0.75) * (y9 * y9 - f(40))
    vt = m2 - m1 * m1
    assert ln[0, 0] == 3 and hist.moments[0, 0, 2] == 0.59375
    assert np.array_equal(bits(hist.moments[0, 0, :2]), bits(np.array([m1, m2], f)))
    assert bits(var)[0, 0] == bits(np.array([vt * (f(0.59375) / (f(1) - f(0.59375)))], f))[0]
    # min_moment_history = 3: the second frame is short (N = 2 < 3) and alone in its window: the propagated value of the plain
    # form, 4 / 4 + 2 / 4 = 1.5; its moments are kept all the same
    hist = TemporalHistory(1, 1)
    run_hand(hist, cam, tt.hand_frame(1, 8.0, 2.0, [0.0]), **dict(kw, min_moment_history=3))
    out, var, ln = run_hand(hist, cam, tt.hand_frame(1, 4.0, 4.0, [0.0]), **dict(kw, min_moment_history=3))
    assert ln[0, 0] == 2 and var[0, 0] == 1.5 and hist.moments[0, 0].tolist() == [6, 40, 0.5]
    # a pixel that is not usable: passed through, all-zero records
    hist = TemporalHistory(1, 1)
    bad = tt.hand_frame(1, np.nan, 2.0, [0.0])
    out, var, ln = run_hand(hist, cam, bad, **kw)
    assert np.array_equal(bits(out), bits(bad["rgba"])) and var[0, 0] == 2 and ln[0, 0] == 0 and hist.moments[0, 0].tolist() == [0, 0, 0]
    # 2 x 1, a first frame, greys 8 and 4 on one node and one plane: both short, each window holds both (k = 2):
    # e1 = 6, e2 = 40, vs = 4, v_acc = (4 * (2 / 1)) * 1 = 8, the unbiased sample variance of {8, 4}; the input variance is not used
    cam2 = tt.hand_camera(2)
    for node1, want_v in ((7, (8.0, 8.0)), (9, (2.0, 6.0))):         # on two nodes each is alone again: the propagated values
        hist = TemporalHistory(2, 1)
        first = tt.hand_frame(2, 8.0, 2.0, [-1.5, 1.5])
        first["rgba"][0, 1, :3], first["variance"][0, 1], first["ids"][0, 1, 0] = 4.0, 6.0, node1
        out, var, ln = run_hand(hist, cam2, first, **kw)
        assert ln.tolist() == [[1, 1]] and var[0].tolist() == list(want_v) and hist.variance[0].tolist() == list(want_v)
        assert np.array_equal(bits(out), bits(first["rgba"]))
    # ... and demodulated: the estimate is formed on the luminance of rgb / d and returned times luma(d)^2
    hist = TemporalHistory(2, 1)
    first = tt.hand_frame(2, 8.0, 2.0, [-1.5, 1.5])
    first["rgba"][0, 1, :3] = 4.0
    alb = np.array([[[0.5, 0.0, 2.0], [0.5, 0.0, 2.0]]], f)
    out, var, ln = run_hand(hist, cam2, dict(first, albedo=alb), **kw)
    ys = [(f(c) / f(0.5) * f(0.2126) + f(c) * f(0.7152)) + f(c) / f(2) * f(0.0722) for c in (8, 4)]
    e1, e2 = (ys[0] + ys[1]) / f(2), (ys[0] * ys[0] + ys[1] * ys[1]) / f(2)
    ld = (f(0.5) * f(0.2126) + f(1) * f(0.7152)) + f(2) * f(0.0722)
    want = ((e2 - e1 * e1) * (f(2) / f(1))) * f(1)
    assert hist.variance[0, 0] == want and var[0, 0] == want * (ld * ld) and var[0, 1] == var[0, 0]
    # the two forms do not mix on one history
    with pytest.raises(AssertionError):
        tt.run_hand(hist, cam2, first, alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01)
    hist.reset()
    tt.run_hand(hist, cam2, first, alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01)


@pytest.fixture(scope="module")
def momentsim(built, tmp_path_factory):
    """tests/temporalsim/temporalsim_moments.cpp: both passes of csrc/temporal.hpp compiled for the host"""
    exe = str(tmp_path_factory.mktemp("temporalsim_moments") / "temporalsim_moments")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tests", "temporalsim", "temporalsim_moments.cpp"),
                        os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_sim(exe, tmp, w, h, seq, demodulate, in_place):
    from yart_amd import api
    prm = params_of(seq)
    frames = frames_of(w, h, seq)
    n = w * h
    fin, fout = os.path.join(tmp, "tm.in"), os.path.join(tmp, "tm.out")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(frames), 1 if demodulate else 0, 1 if in_place else 0, prm["max_history"],
                          prm["min_moment_history"]], np.uint32).tobytes())
        f.write(np.array([prm["alpha_min"], prm["normal_cos_min"], prm["plane_tolerance"]], np.float32).tobytes())
        for k, fr in enumerate(frames):
            f.write(np.array([1 if seq == "reset" and k == 2 else 0], np.uint32).tobytes())
            f.write(bytes(api.make_camera(fr["camera"])))
            for name in ("rgba", "variance", "position", "normal", "depth", "coverage", "ids", "albedo"):
                f.write(fr[name].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    words = np.fromfile(fout, np.uint32).reshape(len(frames), n * 6)
    return r, [(words[k, :n * 4].view(np.float32).reshape(h, w, 4), words[k, n * 4:n * 5].view(np.float32).reshape(h, w),
                words[k, n * 5:].reshape(h, w)) for k in range(len(frames))]


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_equals_the_numpy_statement_on_bits(momentsim, tmp_path, w, h):
    """Both passes of csrc/temporal.hpp on the host == temporal_moments_reference, bit for bit: every camera sequence of
    test_temporal at min_moment_history 2 and the five-frame one at the default 4, demodulation on and off, out of place and in
    place, frame, variance and length of all frames."""
    for seq in SEQUENCES + ["long"]:
        for dm in (False, True):
            want = reference(w, h, seq, dm)
            for in_place in (False, True):
                r, got = run_sim(momentsim, str(tmp_path), w, h, seq, dm, in_place)
                assert r.returncode == 0, r.stderr
                assert len(got) == len(want)
                for k in range(len(want)):
                    assert_same(got[k], want[k], f"{w}x{h} {seq} demodulate {dm} in_place {in_place} frame {k}")


@pytest.mark.parametrize("w,h", [(37, 23), (131, 67)])
def test_the_inputs_take_every_branch(w, h):
    """A condition on the inputs, asserted on the NumPy statement: in the last frame of the multi-pixel move the pixels with a
    temporal estimate and the short pixels estimated from their neighbourhood (k >= 2) each are at least a tenth; in the first
    frame at least a tenth are short (all usable ones are); short pixels alone in their window (k < 2) occur; in the five-frame
    sequence at the default min_moment_history both estimates occur as well; and the moments form changes nothing but the
    variance."""
    n = w * h
    long_, spatial, alone = classes(w, h, "move", False, 2)
    assert long_.sum() >= n / 10 and spatial.sum() >= n / 10, (int(long_.sum()), int(spatial.sum()), n)
    first = classes(w, h, "move", False, 0)
    assert first[0].sum() == 0 and (first[1] | first[2]).sum() >= n / 10 and first[1].sum() >= n / 10
    assert sum(int(classes(w, h, "move", False, k)[2].sum()) for k in range(FRAMES)) >= 1
    res = reference(w, h, "move", False)
    plain = tt.reference(w, h, "move", False, {k: v for k, v in PARAMS.items() if k != "min_moment_history"})
    for k in range(FRAMES):
        assert np.array_equal(bits(res[k][0]), bits(plain[k][0])) and np.array_equal(res[k][2], plain[k][2])
    # where the statement's spatial estimate applied, the variance is not the plain form's (it is on every other pixel)
    same = bits(res[2][1]) == bits(plain[2][1])
    assert same[alone].all() and (~same[spatial]).mean() > 0.9 and (~same[long_]).mean() > 0.9
    long5, spatial5, _ = classes(w, h, "long", True, LONG_FRAMES - 1)
    assert long5.sum() >= n / 2
    long3, spatial3, _ = classes(w, h, "long", True, 2)                 # N = 3 < 4: every usable pixel is still short
    assert long3.sum() == 0 and spatial3.sum() >= n / 2


def noise_frames(sigma, frames=8, size=64, seed=7):
    """A static camera on one plane of one node, constant colour 1 plus iid Gaussian luminance noise, input variance 0"""
    rng = np.random.RandomState(seed)
    cam = tt.base_camera(size, size)
    _, plane, _, p = tt.see(cam, 1e6)                   # one checkerboard cell
    depth = np.linalg.norm(p - np.array(cam["eye"]), axis=-1).astype(np.float32)
    nrm = np.where(plane[..., None] == 2, -1.0, 1.0) * np.array([0.0, 0.0, 1.0])
    ids = np.zeros((size, size, 4), np.int32)
    ids[..., 0] = plane
    out = []
    for _ in range(frames):
        rgba = np.ones((size, size, 4), np.float32)
        rgba[..., :3] = (1.0 + sigma * rng.normal(size=(size, size)))[..., None]
        out.append(dict(camera=cam, rgba=rgba, variance=np.zeros((size, size), np.float32), position=p.astype(np.float32),
                        normal=nrm.astype(np.float32), depth=depth, coverage=np.ones((size, size), np.float32), ids=ids))
    return out


@pytest.mark.parametrize("alpha_min", [0.0, 0.5])
def test_the_estimate_is_the_variance_of_the_accumulated_luminance(alpha_min):
    """Static camera, 64 x 64, iid luminance noise of variance sigma^2 = 0.01 on a constant colour, input variance all 0 (1 spp),
    8 frames, the NumPy statement. The mean over the pixels of out_variance after frame 8 is within 10 % of the empirical
    variance over the pixels of the accumulated luminance — with equal weights (alpha_min 0, max_history 8: w2 = 1/8) and with
    the floor binding (alpha_min 0.5: w2 -> 1/3, where vt / (N - 1) would be 2.3 times too small). Frame 1, where every pixel
    takes the spatial branch, gives sigma^2 within 10 %. Relative standard errors: of the mean estimate sqrt(2/7)/64 = 0.8 %, of the
    empirical variance sqrt(2/4095) = 2.2 %, of the mean spatial estimate sqrt(2/48)/9 = 2.3 % (the windows overlap: 81 disjoint
    ones): 10 % is four sigma or more."""
    from yart_amd.temporal import TemporalHistory, _luma
    sigma = 0.1
    frames = noise_frames(sigma)
    hist = TemporalHistory(64, 64)
    kw = dict(alpha_min=alpha_min, max_history=8, normal_cos_min=0.8, plane_tolerance=0.01, min_moment_history=4)
    for k, fr in enumerate(frames):
        out, var, ln = run_hand(hist, fr["camera"], fr, **kw)
        if k == 0:
            assert (ln == 1).all()
            first = float(var.astype(np.float64).mean())
            print(f"frame 1: mean spatial estimate {first:.6f}, sigma^2 {sigma ** 2:.6f}, ratio {first / sigma ** 2:.4f}")
            assert abs(first / sigma ** 2 - 1) < 0.1
    assert (ln == 8).all()
    empirical = float(_luma(out[..., :3]).astype(np.float64).var(ddof=1))
    estimate = float(var.astype(np.float64).mean())
    w2 = float(hist.moments[0, 0, 2])
    print(f"alpha_min {alpha_min}: w2 {w2:.5f}, mean estimate {estimate:.6f}, empirical {empirical:.6f}, ratio {estimate / empirical:.4f}; "
          f"sigma^2 * w2 {sigma ** 2 * w2:.6f}")
    assert abs(estimate / empirical - 1) < 0.1
    assert abs(w2 - (0.125 if alpha_min == 0 else 1 / 3)) < 2e-3


# -- quality: the gate at the sample count this is for -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def temporalsim(built, tmp_path_factory):
    """tests/temporalsim/temporalsim.cpp, for its host path tracer with feature buffers (`render`)"""
    exe = str(tmp_path_factory.mktemp("temporalsim") / "temporalsim")
    r = tt._build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def accumulate_orbit(frames, moments, **kw):
    from yart_amd.temporal import TemporalHistory, temporal_moments_reference, temporal_reference
    fn = temporal_moments_reference if moments else temporal_reference
    h, w = frames[0]["rgba"].shape[:2]
    hist = TemporalHistory(w, h)
    for fr in frames:
        r = fn(hist, fr["camera"], fr["rgba"], fr["variance"], fr["position"], fr["normal"], fr["depth"], fr["coverage"],
               fr["ids"], fr["albedo"], demodulate=True, **kw)
    return r


def orbit_ratios(hostsim, temporalsim, tmp, name, spp, hi):
    """RMSE over AgX-tonemapped frames against `hi` of: the accumulated frame; plain form + variance-guided filter; moments
    form + the same filter (all at the defaults) -> (accumulated, plain_filtered, moments_filtered)"""
    from yart_amd.denoise import atrous_var_reference
    p = load_params(os.path.join(GOLDEN, name + ".txt"))
    frames = [tt.render_orbit_frame(temporalsim, tmp, name, (96, 96), spp, eye) for eye in tt.orbit_eyes(p)]
    last = frames[-1]
    guides = (last["albedo"], last["normal"], last["depth"])
    tm = lambda x: tt.host_tonemap(hostsim, tmp, x)
    ref = tm(hi)
    acc, acc_var, _ = accumulate_orbit(frames, False)
    macc, macc_var, _ = accumulate_orbit(frames, True)
    assert np.array_equal(bits(acc), bits(macc))
    return (tt.rmse(tm(acc), ref), tt.rmse(tm(atrous_var_reference(acc, acc_var, *guides)), ref),
            tt.rmse(tm(atrous_var_reference(macc, macc_var, *guides)), ref), acc_var, macc_var)


def test_moments_form_beats_the_plain_form_at_one_sample(hostsim, temporalsim, tmp_path):
    """The 6-frame orbit of cornell.yscn of test_temporal (same eyes, tests/golden/temporal/cornell_orbit_hi.f32 as the target)
    at 96 x 96 and 1 spp, where the within-pixel variance is 0 everywhere. RMSE over the AgX-tonemapped frames: the moments
    form followed by the variance-guided filter at its defaults is strictly closer to the 1024-spp frame than the plain form
    followed by the same filter (the chain as it stood, which returns its input), and strictly closer than the accumulated frame
    unfiltered. The 4-spp orbit through both forms is printed, not asserted (profiles/temporal_moments_sweep.txt)."""
    hi = np.fromfile(os.path.join(GOLDEN, "temporal", "cornell_orbit_hi.f32"), np.float32).reshape(96, 96, 4)
    accumulated, plain, moments, plain_var, _ = orbit_ratios(hostsim, temporalsim, str(tmp_path), "cornell", 1, hi)
    assert not plain_var.any()                           # 1 spp: the chain as it stood has no variance at all
    print(f"cornell orbit 1 spp: RMSE accumulated {accumulated:.5f}, plain form filtered {plain:.5f}, moments form filtered "
          f"{moments:.5f} (ratio to plain {moments / plain:.4f}, to unfiltered {moments / accumulated:.4f})")
    a4, p4, m4, _, _ = orbit_ratios(hostsim, temporalsim, str(tmp_path), "cornell", tt.ORBIT_SPP, hi)
    print(f"cornell orbit 4 spp: RMSE accumulated {a4:.5f}, plain form filtered {p4:.5f}, moments form filtered {m4:.5f} "
          f"(ratio to plain {m4 / p4:.4f}, to unfiltered {m4 / a4:.4f})")
    assert moments < plain
    assert moments < accumulated


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


def device_sequence(api, w, h, seq, demodulate, in_place):
    acc = api.TemporalAccumulator(w, h, device=0, moments=True, **params_of(seq))
    res = []
    for k, fr in enumerate(frames_of(w, h, seq)):
        if seq == "reset" and k == 2:
            acc.reset()
        frame, var = fr["rgba"].copy(), fr["variance"].copy()
        got = acc.accumulate(fr["camera"], frame, var, tt.aovs_of(fr, demodulate), demodulate=demodulate,
                             out=frame if in_place else None, out_variance=var if in_place else None)
        if not in_place:
            assert np.array_equal(bits(frame), bits(fr["rgba"])) and np.array_equal(bits(var), bits(fr["variance"]))
        res.append(got)
    acc.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_moments_form_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_tp_accumulate<true> + k_tp_spatial_variance through api.TemporalAccumulator(moments=True).accumulate ==
    temporal_moments_reference, bit for bit: frame, variance and length of every frame (the history, rec3 included, through the
    next frame's result), every camera sequence and the five-frame one at the default, demodulation on and off, out of place
    and with the outputs aliasing the inputs."""
    for seq in SEQUENCES + ["long"]:
        for dm in (False, True):
            want = reference(w, h, seq, dm)
            for in_place in (False, True):
                got = device_sequence(gpu_api, w, h, seq, dm, in_place)
                for k in range(len(want)):
                    tag = f"temporal moments {w}x{h} {seq} demodulate {dm} in_place {in_place} frame {k}"
                    bit_identical_or_drift(got[k][0], want[k][0], tag)
                    assert_same(got[k], want[k], tag)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(37, 23), (131, 67)])
def test_the_forms_do_not_mix_and_the_plain_form_is_untouched(gpu_api, w, h):
    """A plain-form handle next to a moments-form handle on the same inputs gives test_temporal's reference, on bits. The other
    form on a handle that has a history is YART_E_INVALID with a telling message and changes nothing; after a reset it is
    accepted."""
    api = gpu_api
    prm = {k: v for k, v in PARAMS.items() if k != "min_moment_history"}
    plain, moments = api.TemporalAccumulator(w, h, device=0, **prm), api.TemporalAccumulator(w, h, device=0, moments=True, **PARAMS)
    want_plain, want_moments = tt.reference(w, h, "move", True, prm), reference(w, h, "move", True)
    L = api.lib()
    for k, fr in enumerate(tt.frames_of(w, h, "move")):
        args = (fr["camera"], fr["rgba"], fr["variance"], tt.aovs_of(fr, True))
        assert_same(moments.accumulate(*args, demodulate=True), want_moments[k], f"moments form frame {k}")
        assert_same(plain.accumulate(*args, demodulate=True), want_plain[k], f"plain form frame {k}")
        if k == 0:                                       # each handle refuses the other form, and is none the worse for it
            for acc, other in ((plain, True), (moments, False)):
                acc.moments = other
                if other:
                    acc.params["min_moment_history"] = 2
                else:
                    acc.params.pop("min_moment_history")
                with pytest.raises(api.YartError) as e:
                    acc.accumulate(*args, demodulate=True)
                assert e.value.code == api.YART_E_INVALID and "form" in str(e.value) and "reset" in str(e.value)
                acc.moments = not other
                if other:
                    acc.params.pop("min_moment_history")
                else:
                    acc.params["min_moment_history"] = 2
    # after a reset the handle takes the other form: frame 0 again
    fr = tt.frames_of(w, h, "move")[0]
    args = (fr["camera"], fr["rgba"], fr["variance"], tt.aovs_of(fr, True))
    plain.reset()
    plain.moments, plain.params["min_moment_history"] = True, 2
    assert_same(plain.accumulate(*args, demodulate=True), want_moments[0], "moments form on a reset plain handle")
    fr1 = tt.frames_of(w, h, "move")[1]
    assert_same(plain.accumulate(fr1["camera"], fr1["rgba"], fr1["variance"], tt.aovs_of(fr1, True), demodulate=True), want_moments[1],
                "moments form on a reset plain handle, frame 1")
    moments.reset()
    moments.moments = False
    moments.params.pop("min_moment_history")
    assert_same(moments.accumulate(*args, demodulate=True), want_plain[0], "plain form on a reset moments handle")
    assert_same(moments.accumulate(fr1["camera"], fr1["rgba"], fr1["variance"], tt.aovs_of(fr1, True), demodulate=True), want_plain[1],
                "plain form on a reset moments handle, frame 1")
    plain.close()
    moments.close()


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_temporal_moments as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_accumulate_into():
    import torch
    from yart_amd import api
    for w, h in GPU_SIZES:
        for seq, dm in (("move", True), ("subpixel", False)):
            host = api.TemporalAccumulator(w, h, device=0, moments=True, **PARAMS)
            dev = api.TemporalAccumulator(w, h, device=0, moments=True, **PARAMS)
            side = torch.cuda.Stream()
            for k, fr in enumerate(tt.frames_of(w, h, seq)):
                want = host.accumulate(fr["camera"], fr["rgba"], fr["variance"], tt.aovs_of(fr, dm), demodulate=dm)
                t = {name: torch.from_numpy(fr[name].copy()).cuda() for name in fr if name != "camera"}
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    if k == 1:                           # in place, nothing optional
                        out, var = t["rgba"], t["variance"]
                        dev.accumulate_into(out, var, None, fr["camera"], out, var, tt.aovs_of(t, dm), demodulate=dm)
                        got = (out.cpu().numpy(), var.cpu().numpy(), want[2])
                    else:
                        out, var = torch.zeros_like(t["rgba"]), torch.zeros_like(t["variance"])
                        ln = torch.zeros((h, w), dtype=torch.int32, device="cuda")
                        dev.accumulate_into(out, var, ln, fr["camera"], t["rgba"], t["variance"], tt.aovs_of(t, dm), demodulate=dm)
                        got = (out.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy().view(np.uint32))
                        for name in t:
                            assert np.array_equal(bits(t[name].cpu().numpy()), bits(fr[name])), name + " was written"
                assert_same(got, want, f"accumulate_into (moments form) {w}x{h} {seq} frame {k}")
            host.close()
            dev.close()


@pytest.mark.gpu
def test_accumulate_into_equals_the_host_form(gpu_api):
    """api.TemporalAccumulator(moments=True).accumulate_into on torch tensors, on a non-default stream, at every size: the bits
    of accumulate (itself held to the NumPy statement above); inputs untouched when out != in; in place, and without the optional
    length output, too."""
    run_torch_child("child_accumulate_into()")


def child_render_denoised():
    from yart_amd import api
    base = dict(load_params(os.path.join(GOLDEN, "cornell.txt")), size=(96, 96), spp=1)
    scene = api.DeviceScene(os.path.join(GOLDEN, "cornell.yscn"), device=0)
    acc = api.TemporalAccumulator(96, 96, device=0, moments=True)
    hand = api.TemporalAccumulator(96, 96, device=0, moments=True)
    names = ("albedo", "normal", "depth", "position", "coverage", "ids")
    for eye in tt.orbit_eyes(base, frames=3):
        p = dict(base, eye=eye)
        noisy, clean, guides = scene.render_denoised(p, temporal=acc)
        frame, aovs, moms, _ = scene.render_moments(p, ("variance",), names)
        assert np.array_equal(bits(noisy.cpu().numpy()), bits(frame)), "noisy frame"
        assert not moms["variance"].any(), "1 spp: the within-pixel variance is 0"
        a, av, ln = hand.accumulate(p, frame, moms["variance"], aovs, demodulate=True)
        assert np.array_equal(bits(guides["accumulated"].cpu().numpy()), bits(a)), "accumulated frame"
        assert np.array_equal(bits(guides["accumulated_variance"].cpu().numpy()), bits(av)), "accumulated variance"
        assert np.array_equal(bits(guides["length"].cpu().numpy()), bits(ln)), "length"
        want = api.denoise_var(a, av, aovs["albedo"], aovs["normal"], aovs["depth"], demodulate=True)
        got = clean.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), "denoised frame"
        changed = float((bits(got[..., :3]) != bits(a[..., :3])).any(-1).mean())
        print(f"pixels the filter changed: {changed:.3f}; pixels with a variance {float((av > 0).mean()):.3f}")
        assert changed > 0.5, "the filter returned its input: the accumulated variance does not guide it"
    scene.close()


@pytest.mark.gpu
def test_render_denoised_temporal_moments(gpu_api):
    """DeviceScene.render_denoised(temporal=acc) with a moments-form accumulator on cornell.yscn at 96 x 96 and 1 spp, three
    frames of a small orbit: every step == render_moments, accumulate and denoise_var called by hand, bit for bit, and the
    denoised frame differs from the accumulated one on more than half of the pixels (with the plain form's all-zero variance the
    filter returns its input)."""
    run_torch_child("child_render_denoised()")
