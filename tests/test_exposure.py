"""Auto-exposure (include/yart_hip.h: yart_hip_exposure_*): the log-luminance histogram, the trimmed mean, the eye-style adaptation
and the fused gain + AgX + 8-bit pass.

The NumPy statement (yart_amd/exposure.py, with the machine's libm through tests/libmref.py) is the reference of every comparison
here, on bits: histograms and counts as integers, state and frames as uint32 views. The CPU suite holds csrc/exposure.hpp compiled
for the host (tests/exposuresim) to it and works the arithmetic out by hand; the GPU suite holds the kernels to it through the
host entries (AutoExposure.meter / apply), the device entries (meter_into / apply_into) and DeviceScene.render_denoised."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.paramfile import load_params

F = np.float32
CPU_SIZES = [(1, 1), (5, 3), (37, 23)]
GPU_SIZES = CPU_SIZES + [(131, 67)]
# k_ex_histogram's grid is at most 512 workgroups (csrc/postprocess.inc kExMaxBlocks) of 256 lanes, each lane taking 4 pixels per
# pass (csrc/exposure_kernels.inc kExUnroll): 524288 pixels per pass. 727 x 727 = 528529 pixels: every workgroup makes one full pass,
# and a second pass has 4241 pixels left — four whole workgroups, a fifth whose first run of 256 has 145 pixels (two whole waves and
# 17 lanes of a third) and whose other three runs have none, the rest nothing: the grid-stride loop runs twice, the last pass ragged.
STRIDE_SIZE = (727, 727)
KINDS = ("constant", "checker", "loguniform", "pow2", "nonfinite", "ignored")
LOOKS = (0, 1, 2, -1)


def bits(a):
    """the words of a float32 array; every NaN as the one quiet NaN (IEEE 754 leaves a NaN result's sign and payload open, and
    the host's and the device's invalid operations do choose differently: which pixels are NaN is compared, not which NaN)"""
    a = np.ascontiguousarray(a)
    w = a.view(np.uint32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), w) if a.dtype == F else w


def word(x):
    return int(bits(np.array([x], F))[0])


def frame_of(kind, w, h, seed=0, ev_min=-16.0, ev_max=16.0):
    """(h, w, 4) float32 frames that take every branch of the meter"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    f = np.empty((h, w, 4), F)
    f[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(F)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "constant":
        f[..., :3] = (F(0.5), F(0.25), F(0.125))
    elif kind == "checker":
        f[..., :3] = np.where(((xx + yy) & 1)[..., None] == 0, np.array([0.04, 0.05, 0.06], F), np.array([3.0, 2.0, 1.0], F))
    elif kind in ("loguniform", "nonfinite"):
        ev = rng.uniform(ev_min - 2.0, ev_max + 2.0, (h, w))
        f[..., :3] = (np.exp2(ev)[..., None] * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F)
        if w * h >= 2:                                   # both clamps, whatever the draw
            f.reshape(-1, 4)[0, :3] = F(2.0 ** (ev_min - 1.5))
            f.reshape(-1, 4)[-1, :3] = F(2.0 ** (ev_max + 1.5))
        if kind == "nonfinite":
            flat = f.reshape(-1, 4)
            bad = [np.nan, np.inf, -np.inf, -1.0, 0.0, 1e-42, -0.0]
            for i in range(0, flat.shape[0], 2):
                flat[i, (i // 2) % 3] = F(bad[(i // 2) % len(bad)])
            if flat.shape[0] > 4:
                flat[3, :3] = F(1e-42)                   # a denormal pixel: counted, in bin 0
                flat[4, :3] = F(0.0)                     # a black pixel: ignored
    elif kind == "pow2":
        k = ((xx + 3 * yy) % 41 - 20).astype(np.float64)    # 2^-20 .. 2^20: on the bin edges, and beyond both ends
        f[..., :3] = np.exp2(k)[..., None].astype(F)
    elif kind == "ignored":
        pick = (xx + yy) % 4
        f[..., :3] = np.where(pick[..., None] == 0, F(np.nan), np.where(pick[..., None] == 1, F(0.0), np.where(pick[..., None] == 2, F(-2.0), F(np.inf))))
    else:
        raise KeyError(kind)
    return f


@pytest.fixture(scope="module")
def libm(tmp_path_factory):
    """the machine's libm as the statement's log2f / expf / powf"""
    from tests.libmref import LibmRef
    ref = LibmRef(tmp_path_factory.mktemp("libm_exposure"))

    class Fns:
        @staticmethod
        def log2f(x):
            x = np.asarray(x, F)
            return ref.eval("log2f", x.reshape(-1)).view(F).reshape(x.shape)

        @staticmethod
        def expf(x):
            x = np.asarray(x, F)
            return ref.eval("expf", x.reshape(-1)).view(F).reshape(x.shape)

        @staticmethod
        def powf(x, y):
            x, y = np.asarray(x, F), np.asarray(y, F)
            return ref.eval("powf", x.reshape(-1), y.reshape(-1)).view(F).reshape(x.shape)
    return Fns


def statement(libm, frames, params, dts, look, resets=()):
    """the NumPy statement over a sequence: per frame (hist, state dict + valid, ldr, rgb8)"""
    from yart_amd.exposure import ExposureState, apply_reference, exposure_reference
    st = ExposureState()
    out = []
    for k, (fr, dt) in enumerate(zip(frames, dts)):
        if k in resets:
            st = ExposureState()
        hist = exposure_reference(st, fr, params, dt, log2f=libm.log2f, expf=libm.expf)
        ldr, rgb8 = apply_reference(fr, st.gain, look, log2f=libm.log2f, powf=libm.powf)
        out.append((hist, dict(st.asdict(), valid=int(st.valid)), ldr, rgb8))
    return out


STATE_FLOATS = ("cur_ev", "target_ev", "mean_ev", "gain")
STATE_INTS = ("n_counted", "n_ignored", "frames", "flags")


def assert_state(got, want, tag):
    for k in STATE_FLOATS:
        assert word(got[k]) == word(want[k]), f"{tag}: {k} {got[k]!r} != {want[k]!r}"
    for k in STATE_INTS + (("valid",) if "valid" in got else ()):
        assert int(got[k]) == int(want[k]), f"{tag}: {k} {got[k]} != {want[k]}"


def assert_frame(got, want, tag):
    hist, st, ldr, rgb8 = got
    assert np.array_equal(np.asarray(hist, np.uint32), want[0]), f"{tag}: histogram"
    assert_state(st, want[1], tag)
    if ldr is not None:
        assert np.array_equal(bits(ldr), bits(want[2])), f"{tag}: ldr, {int((bits(ldr) != bits(want[2])).sum())} words differ"
    if rgb8 is not None:
        assert np.array_equal(rgb8, want[3]), f"{tag}: rgb8, {int((rgb8 != want[3]).sum())} bytes differ"


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def _build_sim(path, flags=("-O2",)):
    return subprocess.run(["g++", "-std=c++17", *flags, "-ffp-contract=off", "-o", path,
                           os.path.join(ROOT, "tests", "exposuresim", "exposuresim.cpp")], capture_output=True, text=True)


@pytest.fixture(scope="module")
def exposuresim(tmp_path_factory):
    """tests/exposuresim/exposuresim.cpp: csrc/exposure.hpp compiled for the host"""
    exe = str(tmp_path_factory.mktemp("exposuresim") / "exposuresim")
    r = _build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


PARAM_ORDER = ("ev_min", "ev_max", "trim_low", "trim_high", "key", "compensation_ev", "gain_ev_min", "gain_ev_max", "speed_up", "speed_down")


def run_sim(exe, tmp, frames, params, dts, look, resets=()):
    h, w = frames[0].shape[:2]
    n = w * h
    fin, fout = os.path.join(tmp, "ex.in"), os.path.join(tmp, "ex.out")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(frames)], np.uint32).tobytes())
        f.write(np.array([look], np.int32).tobytes())
        f.write(np.array([params[k] for k in PARAM_ORDER], F).tobytes())
        f.write(np.array(params["window"] or (0, 0, 0, 0), np.uint32).tobytes())
        for k, (fr, dt) in enumerate(zip(frames, dts)):
            f.write(np.array([dt], F).tobytes())
            f.write(np.array([1 if k in resets else 0], np.uint32).tobytes())
            f.write(np.ascontiguousarray(fr, F).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blob = open(fout, "rb").read()
    per = 256 * 4 + 9 * 4 + n * 16 + n * 3
    assert len(blob) == per * len(frames)
    out = []
    for k in range(len(frames)):
        b = blob[k * per:(k + 1) * per]
        hist = np.frombuffer(b, np.uint32, 256, 0)
        fs = np.frombuffer(b, F, 4, 1024)
        us = np.frombuffer(b, np.uint32, 5, 1040)
        st = dict(zip(STATE_FLOATS, fs), **dict(zip(STATE_INTS + ("valid",), (int(v) for v in us))))
        ldr = np.frombuffer(b, F, n * 4, 1060).reshape(h, w, 4)
        rgb8 = np.frombuffer(b, np.uint8, n * 3, 1060 + n * 16).reshape(h, w, 3)
        out.append((hist, st, ldr, rgb8))
    return out


def windows_of(w, h):
    """the whole frame, one pixel, a ragged interior rectangle, a rectangle on the last row and column"""
    wins = [None, (w // 2, h // 2, w // 2 + 1, h // 2 + 1)]
    if w >= 5 and h >= 3:
        wins.append((1, 1, w - 1 - (w > 8), h - 1))
    wins.append((max(0, w - 3), max(0, h - 2), w, h))
    return wins


def test_abi_struct_sizes_and_argument_errors(built, tmp_path):
    """The entries exist and are in api.EXPORTS, the ABI is still 3, YartExposureParams (60 bytes) and YartExposureState (36) and
    the defaults agree between ctypes, yart_amd/exposure.py and a C++ compile of both headers (which also sees
    yart::hip::Exposure and exposureDefaults), and every refusal the header lists is YART_E_INVALID with a telling message,
    before any device is touched: the calls are made here whether or not there is a device."""
    from yart_amd import api, exposure
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in ("create", "destroy", "reset", "meter_device", "meter_host", "apply_device", "apply_host", "get"):
        assert hasattr(raw, "yart_hip_exposure_" + name) and "yart_hip_exposure_" + name in api.EXPORTS, name
    assert L.yart_hip_abi_version() == 3
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n#include <cstddef>\n'
                "int main() { YartExposureParams p = yart::hip::exposureDefaults();\n"
                "  std::printf(\"%zu %zu %zu %zu %zu %u %u\\n\", sizeof(YartExposureParams), sizeof(YartExposureState), offsetof(YartExposureParams, key),\n"
                "      offsetof(YartExposureParams, x0), offsetof(YartExposureState, n_counted), YART_EXPOSURE_BINS, YART_EXPOSURE_EMPTY);\n"
                "  std::printf(\"%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\\n\", p.ev_min, p.ev_max, p.trim_low, p.trim_high, p.key,\n"
                "      p.compensation_ev, p.gain_ev_min, p.gain_ev_max, p.speed_up, p.speed_down);\n"
                "  if (p.struct_size != sizeof(p) || p.x0 || p.y0 || p.x1 || p.y1) return 3;\n"
                "  yart::hip::Exposure e(0);\n"
                "  YartExposureState s = e.state();\n"
                "  if (s.gain != 1.0f || s.frames != 0u) return 4;\n"
                "  e.reset();\n"
                "  p.key = 0.0f;\n"
                "  try { e.meter(std::vector<float>(4, 1.0f), 1, 1, p, 0.0f); return 2; } catch (const yart::hip::Error&) {}\n"
                "  return 0; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    P, S = api.ExposureParams, api.ExposureStateRecord
    assert [int(v) for v in out[:7]] == [ctypes.sizeof(P), ctypes.sizeof(S), P.key.offset, P.x0.offset, S.n_counted.offset, exposure.BINS,
                                         exposure.FLAG_EMPTY]
    assert ctypes.sizeof(P) == 60 and ctypes.sizeof(S) == 36
    assert [F(v) for v in out[7:17]] == [F(exposure.DEFAULTS[k]) for k in PARAM_ORDER]
    assert exposure.DEFAULTS["window"] is None

    h = ctypes.c_void_p()
    assert L.yart_hip_exposure_create(0, None) == api.YART_E_INVALID and b"out pointer" in L.yart_hip_last_error()
    assert L.yart_hip_exposure_create(0, ctypes.byref(h)) == api.YART_OK and h.value
    frame = np.ones((4, 4, 4), F)
    ptr = frame.ctypes.data_as(ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")

    def meter(entry, handle=h, rgba=ptr, w=4, hh=4, dt=0.0, struct_size=None, null_params=False, **over):
        ep = api.make_exposure_params(**over)
        if struct_size is not None:
            ep.struct_size = struct_size
        args = [handle, rgba, w, hh, None if null_params else ctypes.byref(ep), dt]
        return (L.yart_hip_exposure_meter_device(*args, None) if entry == "device" else L.yart_hip_exposure_meter_host(*args))
    cases = [(dict(handle=None), b"handle"), (dict(rgba=None), b"rgba"), (dict(null_params=True), b"params pointer"),
             (dict(struct_size=56), b"struct_size"), (dict(struct_size=0), b"struct_size"),
             (dict(w=0), b"width or height"), (dict(hh=0), b"width or height"), (dict(w=1 << 15, hh=(1 << 13) + 1), b"2^28"),
             (dict(ev_min=nan), b"ev_min"), (dict(ev_max=inf), b"ev_min"), (dict(ev_min=2.0, ev_max=2.0), b"ev_min"), (dict(ev_min=3.0, ev_max=2.0), b"ev_min"),
             (dict(trim_low=-0.1), b"trim_low"), (dict(trim_low=1.0), b"trim_low"), (dict(trim_high=1.0), b"trim_low"), (dict(trim_high=nan), b"trim_low"),
             (dict(trim_low=0.5, trim_high=0.5), b"trim_low"), (dict(trim_low=nan), b"trim_low"),
             (dict(key=0.0), b"key"), (dict(key=-1.0), b"key"), (dict(key=nan), b"key"), (dict(key=inf), b"key"),
             (dict(compensation_ev=nan), b"compensation_ev"), (dict(compensation_ev=-inf), b"compensation_ev"),
             (dict(gain_ev_min=1.0, gain_ev_max=0.5), b"gain_ev_min"), (dict(gain_ev_min=nan), b"gain_ev_min"), (dict(gain_ev_max=inf), b"gain_ev_min"),
             (dict(speed_up=-1.0), b"speed_up"), (dict(speed_down=nan), b"speed_up"), (dict(speed_up=inf), b"speed_up"),
             (dict(dt=-1.0), b"dt"), (dict(dt=nan), b"dt"), (dict(dt=inf), b"dt"),
             (dict(window=(2, 0, 2, 4)), b"window"), (dict(window=(0, 0, 5, 4)), b"window"), (dict(window=(0, 3, 4, 5)), b"window"),
             (dict(window=(3, 0, 2, 4)), b"window"), (dict(window=(0, 0, 0, 4)), b"window")]
    for entry in ("device", "host"):
        for kw, word in cases:
            assert meter(entry, **kw) == api.YART_E_INVALID, (entry, kw, L.yart_hip_last_error())
            assert word in L.yart_hip_last_error(), (entry, kw, L.yart_hip_last_error())
    ldr, rgb = np.empty((4, 4, 4), F), np.empty((4, 4, 3), np.uint8)
    pl, pr = ldr.ctypes.data_as(ctypes.c_void_p), rgb.ctypes.data_as(ctypes.c_void_p)

    def apply(entry, handle=h, rgba=ptr, w=4, hh=4, look=0, o1=pl, o2=pr):
        args = [handle, rgba, w, hh, look, o1, o2]
        return L.yart_hip_exposure_apply_device(*args, None) if entry == "device" else L.yart_hip_exposure_apply_host(*args)
    cases = [(dict(handle=None), b"handle"), (dict(rgba=None), b"rgba"), (dict(o1=None, o2=None), b"both outputs"), (dict(w=0), b"width or height"),
             (dict(hh=0), b"width or height"), (dict(w=1 << 15, hh=(1 << 13) + 1), b"2^28"), (dict(look=-2), b"look"), (dict(look=3), b"look")]
    for entry in ("device", "host"):
        for kw, word in cases:
            assert apply(entry, **kw) == api.YART_E_INVALID, (entry, kw, L.yart_hip_last_error())
            assert word in L.yart_hip_last_error(), (entry, kw, L.yart_hip_last_error())
    rec = S(ctypes.sizeof(S))
    assert L.yart_hip_exposure_get(None, ctypes.byref(rec), None) == api.YART_E_INVALID and b"handle" in L.yart_hip_last_error()
    assert L.yart_hip_exposure_get(h, None, None) == api.YART_E_INVALID and b"state pointer" in L.yart_hip_last_error()
    rec.struct_size = 32
    assert L.yart_hip_exposure_get(h, ctypes.byref(rec), None) == api.YART_E_INVALID and b"struct_size" in L.yart_hip_last_error()
    assert L.yart_hip_exposure_reset(None) == api.YART_E_INVALID and b"handle" in L.yart_hip_last_error()
    assert L.yart_hip_exposure_reset(h) == api.YART_OK
    L.yart_hip_exposure_destroy(h)
    L.yart_hip_exposure_destroy(None)
    # the Python surface: a handle that has metered nothing reports a new handle's state and touches no device
    ex = api.AutoExposure(key=0.25, window=(0, 0, 2, 2))
    assert ex.params["key"] == 0.25 and ex.params["ev_min"] == exposure.DEFAULTS["ev_min"]
    st = ex.state(histogram=True)
    assert st["gain"] == F(1.0) and st["frames"] == 0 and st["flags"] == 0 and not st["histogram"].any()
    with pytest.raises(AssertionError):
        api.AutoExposure(sigma=1.0)
    ex.reset()
    ex.close()
    if L.yart_hip_device_count() == 0:
        ex = api.AutoExposure()
        with pytest.raises(api.YartError) as e:
            ex.meter(frame, 0.0)
        assert e.value.code == api.YART_E_NO_DEVICE
        ex.close()


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_equals_the_numpy_statement_on_bits(exposuresim, libm, tmp_path, w, h):
    """csrc/exposure.hpp on the host == yart_amd/exposure.py with the machine's libm, bit for bit: histogram, state and the
    applied frame of every frame kind as a three-frame sequence (the second a darker copy, the third the kind again), every
    look, every metering window."""
    from yart_amd.exposure import params_of
    for i, kind in enumerate(KINDS):
        base = frame_of(kind, w, h)
        frames = [base, (base * F(0.125)).astype(F), frame_of(kind, w, h, seed=1)]
        dts = [0.0, 1.0 / 30.0, 0.5]
        for j, win in enumerate(windows_of(w, h)):
            prm = params_of(window=win, compensation_ev=0.5 * j)
            look = LOOKS[(i + j) % 4]
            want = statement(libm, frames, prm, dts, look)
            got = run_sim(exposuresim, str(tmp_path), frames, prm, dts, look)
            for k in range(3):
                assert_frame(got[k], want[k], f"{kind} {w}x{h} window {win} look {look} frame {k}")


def test_the_inputs_take_every_branch(libm):
    """What the frames are made for, at 37 x 23 with the defaults: constant — one bin holds every pixel; checker — two bins, half
    each; loguniform — both clamps (bins 0 and 255) and the bins between; pow2 — every counted pixel's t is an integer (ev on a
    bin edge); nonfinite — ignored pixels of every cause and a denormal pixel that is counted; ignored — N == 0, the state
    untouched, the flag set."""
    from yart_amd.exposure import BINS, FLAG_EMPTY, ExposureState, exposure_reference, histogram_reference, params_of
    w, h, prm = 37, 23, params_of()
    hist, ign, bins = histogram_reference(frame_of("constant", w, h), prm, libm.log2f)
    Y = (F(0.2126) * F(0.5) + F(0.7152) * F(0.25)) + F(0.0722) * F(0.125)
    b = int((libm.log2f(np.array([Y], F))[0] + F(16.0)) * F(8.0))
    assert ign == 0 and hist[b] == w * h and hist.sum() == w * h
    hist, ign, _ = histogram_reference(frame_of("checker", w, h), prm, libm.log2f)
    assert ign == 0 and sorted(hist[hist > 0]) == [w * h // 2, w * h - w * h // 2]
    hist, ign, _ = histogram_reference(frame_of("loguniform", w, h), prm, libm.log2f)
    assert ign == 0 and hist[0] > 1 and hist[255] > 1 and (hist[1:255] > 0).sum() > 200
    fr = frame_of("pow2", w, h)
    hist, ign, _ = histogram_reference(fr, prm, libm.log2f)
    assert ign == 0 and hist[0] > 0 and hist[255] > 0
    assert not hist[np.arange(BINS) % 8 != 0][:-1].any() and hist[255] + hist[::8].sum() == w * h, "powers of two land on whole EVs"
    fr = frame_of("nonfinite", w, h)
    hist, ign, bins = histogram_reference(fr, prm, libm.log2f)
    flat, fb = fr.reshape(-1, 4), bins.reshape(-1)
    assert ign > 0 and ign + hist.sum() == w * h
    assert fb[3] == 0 and fb[4] == BINS, "a denormal pixel is counted (bin 0), a black one ignored"
    for i in range(flat.shape[0]):
        fin = np.isfinite(flat[i, :3]).all()
        assert fin or fb[i] == BINS, "a pixel with a channel that is not finite is ignored"
    st = ExposureState(cur_ev=F(1.5), target_ev=F(2.0), mean_ev=F(-3.0), gain=F(2.75), frames=3, valid=True)
    hist = exposure_reference(st, frame_of("ignored", w, h), prm, 0.1, libm.log2f, libm.expf)
    assert not hist.any() and st.n_counted == 0 and st.n_ignored == w * h and st.flags == FLAG_EMPTY
    assert (st.cur_ev, st.target_ev, st.mean_ev, st.gain, st.frames, st.valid) == (F(1.5), F(2.0), F(-3.0), F(2.75), 3, True)
    exposure_reference(st, frame_of("constant", w, h), prm, 0.1, libm.log2f, libm.expf)
    assert st.flags == 0 and st.frames == 4 and st.n_ignored == 0


def test_resolve_on_hand_worked_histograms(libm):
    """The trimmed mean worked out by hand. Bin centres at the defaults: centre_b = -16 + (b + 0.5) / 8, exact in binary32."""
    from yart_amd.exposure import BINS, ExposureState, exposure_reference, params_of, resolve_reference
    centre = lambda b: -16.0 + (b + 0.5) / 8.0
    prm = params_of()
    # N = 1 with the default trims: lo = floor(0.1) = 0, hi = 1 - 0 = 1, K = 1
    hist = np.zeros(BINS, np.uint32)
    hist[100] = 1
    N, K, S, mean, ks = resolve_reference(hist, prm)
    assert (N, K) == (1, 1) and ks[100] == 1 and sum(ks) == 1 and mean == F(centre(100))
    # no trims: the plain mean over the bins
    hist = np.zeros(BINS, np.uint32)
    hist[[10, 20, 200]] = [3, 5, 2]
    N, K, S, mean, ks = resolve_reference(hist, params_of(trim_low=0.0, trim_high=0.0))
    assert (N, K) == (10, 10) and ks[10] == 3 and ks[20] == 5 and ks[200] == 2
    assert mean == F((3 * centre(10) + 5 * centre(20) + 2 * centre(200)) / 10.0)
    # trims that cut inside a bin: N = 40; lo = floor(double(0.25f) * 40) = 10, hi = 40 - floor(double(0.3f) * 40) = 40 - 12 = 28
    # (0.3f is 0.300000011..., so the product is just above 12). Bins: 8 pixels in bin 5 -> [0, 8), 12 in bin 6 -> [8, 20), 20 in
    # bin 7 -> [20, 40). [10, 28) takes 0 of bin 5, 10 of bin 6 (cut at its low end), 8 of bin 7 (cut at its high end): K = 18
    hist = np.zeros(BINS, np.uint32)
    hist[[5, 6, 7]] = [8, 12, 20]
    N, K, S, mean, ks = resolve_reference(hist, params_of(trim_low=0.25, trim_high=0.3))
    assert (N, K) == (40, 18) and (ks[5], ks[6], ks[7]) == (0, 10, 8) and sum(ks) == 18
    assert S == 10 * centre(6) + 8 * centre(7) and mean == F(S / 18.0)
    # and the state step from it: key 0.18, compensation 0.25 -> target = (log2f(0.18f) - mean) + 0.25f; a first frame snaps
    fr = np.zeros((1, 40, 4), F)
    for i, b in enumerate([5] * 8 + [6] * 12 + [7] * 20):
        fr[0, i, :3] = F(2.0 ** (centre(b)))            # mid-bin luminances (the weights sum to 1.0f exactly)
    st = ExposureState()
    got = exposure_reference(st, fr, params_of(trim_low=0.25, trim_high=0.3, compensation_ev=0.25), 0.0, libm.log2f, libm.expf)
    assert np.array_equal(got, hist)
    key_ev = libm.log2f(np.array([0.18], F))[0]
    assert st.mean_ev == mean and st.target_ev == (key_ev - mean) + F(0.25) and st.cur_ev == st.target_ev and st.valid
    assert st.gain == libm.expf(np.array([st.cur_ev * F(0.6931472)], F))[0] and st.frames == 1
    # the target's clamp
    st = ExposureState()
    exposure_reference(st, fr, params_of(gain_ev_min=-1.0, gain_ev_max=2.0), 0.0, libm.log2f, libm.expf)
    assert st.target_ev == F(2.0)
    st = ExposureState()
    exposure_reference(st, (fr * F(2.0 ** 20)).astype(F), params_of(gain_ev_min=-1.0, gain_ev_max=2.0), 0.0, libm.log2f, libm.expf)
    assert st.target_ev == F(-1.0)


# The metering window of the scaling property: columns 16 .. 111 of rows 0 .. 92 of the cornell golden. The rows below hold the
# frame's darkest pixels, below 2^-16 (bin 0, the lower clamp) or black; and of the windows without a clamped pixel this is one for
# which the three roundings to binary32 that follow the exact shift — of mean_ev, of the target, and of cur_ev * 0.6931472f — land on
# values exactly 2.0 apart (gain: exactly a factor 4): a rounding does not commute with a shift across a power of two (over rows
# 0 .. 92 at full width mean_ev is -2.3788717 and -4.378872, which differ by 2 + 2^-22), so the property is one of chosen inputs.
SCALING_WINDOW = (16, 0, 112, 93)


def scaling_frames():
    p = load_params(os.path.join(GOLDEN, "cornell.txt"))
    w, h = int(p["size"][0]), int(p["size"][1])
    a = np.fromfile(os.path.join(GOLDEN, "cornell.f32"), F).reshape(h, w, 4)
    b = (a * F(0.25)).astype(F)
    assert np.array_equal(bits((b * F(4.0)).astype(F)), bits(a)), "the scaling is exact"
    return a, b


def assert_scaling(ra, rb, run):
    """(hist, state, ldr, rgb8) of the frame and of the frame times 0.25"""
    assert np.array_equal(np.roll(ra[0], -16), rb[0]) and not ra[0][:16].any(), run
    print(run, "mean_ev", ra[1]["mean_ev"], rb[1]["mean_ev"], "target_ev", ra[1]["target_ev"], rb[1]["target_ev"], "gain", ra[1]["gain"], rb[1]["gain"])
    assert F(ra[1]["mean_ev"]) - F(rb[1]["mean_ev"]) == F(2.0) and F(rb[1]["mean_ev"]) + F(2.0) == F(ra[1]["mean_ev"]), run
    assert F(rb[1]["target_ev"]) - F(ra[1]["target_ev"]) == F(2.0) and F(ra[1]["target_ev"]) + F(2.0) == F(rb[1]["target_ev"]), run
    print(run, "applied frames: identical words", float(np.mean(bits(ra[2]) == bits(rb[2]))), "differing bytes", int((ra[3] != rb[3]).sum()))
    assert np.array_equal(bits(ra[2]), bits(rb[2])) and np.array_equal(ra[3], rb[3]), f"{run}: the applied frames differ"


def test_scaling_a_frame_moves_the_histogram(exposuresim, libm, tmp_path):
    """The cornell golden times 0.25 (exact in binary32): at the default range, 8 bins per EV, every counted pixel moves down by
    exactly 16 bins — metered over SCALING_WINDOW, where no pixel of either frame is clamped, which is asserted —, mean_ev drops
    by exactly 2.0, the target rises by exactly 2.0, and the applied frames (the whole frames) are the same bits. Held for the
    NumPy statement and for csrc/exposure.hpp on the host."""
    from yart_amd.exposure import BINS, histogram_reference, params_of
    a, b = scaling_frames()
    x0, y0, x1, y1 = SCALING_WINDOW
    prm = params_of(window=SCALING_WINDOW)
    ha, ia, ba = histogram_reference(a, prm, libm.log2f)
    hb, ib, bb = histogram_reference(b, prm, libm.log2f)
    counted = ba < BINS
    assert counted.sum() == (x1 - x0) * (y1 - y0) and ia == ib == 0 and np.array_equal(counted, bb < BINS)
    assert ba[counted].min() >= 17 and ba[counted].max() <= 254 and bb[counted].min() >= 1, "a pixel is clamped"
    assert np.array_equal(bb[counted] + 16, ba[counted]), "every counted pixel moves by exactly 16 bins"
    assert_scaling(statement(libm, [a], prm, [0.0], 0)[0], statement(libm, [b], prm, [0.0], 0)[0], "statement")
    assert_scaling(run_sim(exposuresim, str(tmp_path), [a], prm, [0.0], 0)[0], run_sim(exposuresim, str(tmp_path), [b], prm, [0.0], 0)[0], "exposuresim")


def adaptation_frames(w, h):
    """eight frames: the brightness stepped down (x 1/8) at frame 3 and up (x 16) at frame 6"""
    base = frame_of("checker", w, h)
    scale = [1.0, 1.0, 1.0, 0.125, 0.125, 0.125, 2.0, 2.0]
    return [(base * F(s)).astype(F) for s in scale]


def test_adaptation_follows_the_recurrence(exposuresim, libm, tmp_path):
    """Eight frames at dt = 1/30 with the brightness stepped down at frame 3 and up at frame 6: cur_ev follows
    cur += (target - cur) * (a_up when the target is above, else a_down), a = 1 - expf(-(dt * speed)), worked out here from the
    targets; the exposure rises after the step down and falls after the step up. speed 0 freezes it at the first target; a
    large dt reaches the target to within the last rounding of the recurrence; a reset snaps to the target."""
    from yart_amd.exposure import params_of
    w, h = 5, 3
    frames = adaptation_frames(w, h)
    dt = 1.0 / 30.0
    dts = [dt] * 8
    prm = params_of()
    want = statement(libm, frames, prm, dts, 0)
    got = run_sim(exposuresim, str(tmp_path), frames, prm, dts, 0)
    for k in range(8):
        assert_frame(got[k], want[k], f"adaptation frame {k}")
    a_up = F(1.0) - libm.expf(np.array([-(F(dt) * F(3.0))], F))[0]
    a_down = F(1.0) - libm.expf(np.array([-(F(dt) * F(1.0))], F))[0]
    assert 0 < a_down < a_up < 1
    cur = None
    for k in range(8):
        st = want[k][1]
        target = F(st["target_ev"])
        if cur is None:
            cur = target
        else:
            d = target - cur
            cur = cur + d * (a_up if d > 0 else a_down)
        assert cur.dtype == F and word(cur) == word(st["cur_ev"]), f"frame {k}: cur_ev {st['cur_ev']!r}, the recurrence gives {cur!r}"
        assert st["frames"] == k + 1
    t = [F(s[1]["target_ev"]) for s in want]
    c = [F(s[1]["cur_ev"]) for s in want]
    # (a frame times 2^k moves the mean by -k up to the rounding of mean_ev and the target to binary32: a few ulps of 4)
    assert t[0] == t[1] == t[2] == c[2] and abs(t[3] - (t[2] + F(3.0))) < 2e-6 and abs(t[6] - (t[2] - F(1.0))) < 2e-6
    assert c[2] < c[3] < c[4] < c[5] < t[5] and c[5] > c[6] > c[7] > t[7]
    # speed 0: a = 1 - expf(-0) = 0
    frozen = statement(libm, frames, params_of(speed_up=0.0, speed_down=0.0), dts, 0)
    got = run_sim(exposuresim, str(tmp_path), frames, params_of(speed_up=0.0, speed_down=0.0), dts, 0)
    for k in range(8):
        assert_frame(got[k], frozen[k], f"frozen frame {k}")
        assert F(frozen[k][1]["cur_ev"]) == t[0]
    # a large dt: a = 1 - expf(-300) = 1, cur + (target - cur) * 1 is the target up to the rounding of the two operations
    fast = statement(libm, frames, prm, [100.0] * 8, 0)
    got = run_sim(exposuresim, str(tmp_path), frames, prm, [100.0] * 8, 0)
    for k in range(8):
        assert_frame(got[k], fast[k], f"fast frame {k}")
        cur, target = F(fast[k][1]["cur_ev"]), F(fast[k][1]["target_ev"])
        assert abs(np.float64(cur) - np.float64(target)) <= np.spacing(np.abs(target)), (k, cur, target)
    # reset before frame 4: it snaps
    snap = statement(libm, frames, prm, dts, 0, resets=(4,))
    got = run_sim(exposuresim, str(tmp_path), frames, prm, dts, 0, resets=(4,))
    for k in range(8):
        assert_frame(got[k], snap[k], f"reset frame {k}")
    assert F(snap[4][1]["cur_ev"]) == F(snap[4][1]["target_ev"]) and snap[4][1]["frames"] == 1
    assert F(snap[3][1]["cur_ev"]) != F(snap[3][1]["target_ev"])


def test_metering_window(libm):
    """The window is half open and only its pixels are counted: the whole frame, one pixel, a ragged interior rectangle and a
    rectangle on the last row and column give the histogram of the cropped frame; apply is not windowed."""
    from yart_amd.exposure import histogram_reference, params_of
    for w, h in CPU_SIZES:
        fr = frame_of("nonfinite", w, h)
        for win in windows_of(w, h):
            hist, ign, _ = histogram_reference(fr, params_of(window=win), libm.log2f)
            x0, y0, x1, y1 = win or (0, 0, w, h)
            crop = np.ascontiguousarray(fr[y0:y1, x0:x1])
            hist2, ign2, _ = histogram_reference(crop, params_of(), libm.log2f)
            assert np.array_equal(hist, hist2) and ign == ign2 and hist.sum() + ign == (x1 - x0) * (y1 - y0)
    for bad in ((0, 0, 0, 3), (2, 0, 2, 3), (0, 0, 6, 3), (0, 0, 5, 4)):
        with pytest.raises(AssertionError):
            histogram_reference(frame_of("constant", 5, 3), params_of(window=bad), libm.log2f)


def test_the_host_statement_under_sanitizers(libm, tmp_path):
    """tests/exposuresim once more with -fsanitize=address,undefined, a stand-alone program: 5 x 3 and 37 x 23 with a window on
    the last row and column, the frame with the values that are not finite: no report, and the statement's bits."""
    from yart_amd.exposure import params_of
    exe = str(tmp_path / "exposuresim_san")
    r = _build_sim(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert r.returncode == 0, r.stderr[-2000:]
    for w, h in ((5, 3), (37, 23)):
        win = windows_of(w, h)[-1]
        assert win[2] == w and win[3] == h
        for kind, look in (("nonfinite", 1), ("loguniform", -1), ("ignored", 0)):
            frames = [frame_of(kind, w, h), frame_of(kind, w, h, seed=2)]
            prm = params_of(window=win)
            want = statement(libm, frames, prm, [0.0, 0.25], look)
            got = run_sim(exe, str(tmp_path), frames, prm, [0.0, 0.25], look)
            for k in range(2):
                assert_frame(got[k], want[k], f"sanitized {kind} {w}x{h} frame {k}")


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def device_state(ex):
    st = ex.state(histogram=True)
    return st.pop("histogram"), st


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_meter_and_apply_equal_the_numpy_statement_on_bits(gpu_api, libm, w, h):
    """k_ex_histogram, k_ex_resolve and k_ex_apply<true, true> through AutoExposure.meter / apply — the host entries — == the
    NumPy statement with the machine's libm, bit for bit: the histogram, the state and the applied frame of every frame kind as a
    three-frame sequence, every look, every metering window. 131 x 67 is 35 workgroups, the last one ragged."""
    from yart_amd.exposure import params_of
    for i, kind in enumerate(KINDS):
        base = frame_of(kind, w, h)
        frames = [base, (base * F(0.125)).astype(F), frame_of(kind, w, h, seed=1)]
        dts = [0.0, 1.0 / 30.0, 0.5]
        for j, win in enumerate(windows_of(w, h)):
            prm = params_of(window=win, compensation_ev=0.5 * j)
            look = LOOKS[(i + j) % 4]
            want = statement(libm, frames, prm, dts, look)
            ex = gpu_api.AutoExposure(device=0, **prm)
            for k in range(3):
                keep = frames[k].copy()
                ex.meter(frames[k], dts[k])
                hist, st = device_state(ex)
                ldr, rgb8 = ex.apply(frames[k], None if look < 0 else look)
                assert np.array_equal(bits(keep), bits(frames[k])), "the frame was written"
                assert_frame((hist, st, ldr, rgb8), want[k], f"device {kind} {w}x{h} window {win} look {look} frame {k}")
            ex.close()


@pytest.mark.gpu
def test_device_adaptation_reset_and_empty_frames(gpu_api, libm):
    """The adaptation sequence of the CPU suite on the device, with a reset before frame 4 and an all-ignored frame in the
    middle (the state stays, YART_EXPOSURE_EMPTY is set, apply keeps the gain); the histogram read back after each call is that
    frame's alone — k_ex_resolve's clear works."""
    from yart_amd.exposure import FLAG_EMPTY, params_of
    w, h = 37, 23
    frames = adaptation_frames(w, h)
    frames.insert(2, frame_of("ignored", w, h))
    dts = [1.0 / 30.0] * len(frames)
    prm = params_of(speed_up=2.0, speed_down=0.5)
    want = statement(libm, frames, prm, dts, 2, resets=(5,))
    assert want[2][1]["flags"] == FLAG_EMPTY and not want[2][0].any() and want[3][1]["flags"] == 0
    ex = gpu_api.AutoExposure(device=0, **prm)
    ldr0, _ = ex.apply(frames[0], "punchy")              # never metered: gain 1
    from yart_amd.exposure import apply_reference
    assert np.array_equal(bits(ldr0), bits(apply_reference(frames[0], 1.0, 2, libm.log2f, libm.powf)[0]))
    for k, fr in enumerate(frames):
        if k == 5:
            ex.reset()
            assert ex.state()["gain"] == F(1.0) and ex.state()["frames"] == 0
        ex.meter(fr, dts[k])
        hist, st = device_state(ex)
        ldr, rgb8 = ex.apply(fr, "punchy")
        assert_frame((hist, st, ldr, rgb8), want[k], f"device adaptation frame {k}")
    ex.close()


@pytest.mark.gpu
def test_device_scaling_a_frame_moves_the_histogram(gpu_api, libm):
    """test_scaling_a_frame_moves_the_histogram on the device: the statement's bits, and the property itself."""
    from yart_amd.exposure import params_of
    prm = params_of(window=SCALING_WINDOW)
    got = []
    for fr in scaling_frames():
        ex = gpu_api.AutoExposure(device=0, **prm)
        ex.meter(fr, 0.0)
        hist, st = device_state(ex)
        got.append((hist, st) + ex.apply(fr, "none"))
        ex.close()
        assert_frame(got[-1], statement(libm, [fr], prm, [0.0], 0)[0], "device scaling")
    assert_scaling(got[0], got[1], "device")


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_exposure as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_libm():
    import tempfile
    from tests.libmref import LibmRef
    ref = LibmRef(tempfile.mkdtemp(prefix="libm_exposure_"))

    class Fns:
        log2f = staticmethod(lambda x: ref.eval("log2f", np.asarray(x, F).reshape(-1)).view(F).reshape(np.shape(x)))
        expf = staticmethod(lambda x: ref.eval("expf", np.asarray(x, F).reshape(-1)).view(F).reshape(np.shape(x)))
        powf = staticmethod(lambda x, y: ref.eval("powf", np.asarray(x, F).reshape(-1), np.asarray(y, F).reshape(-1)).view(F).reshape(np.shape(x)))
    return Fns


def child_into():
    import torch
    from yart_amd import api
    from yart_amd.exposure import params_of
    libm = child_libm()
    side = torch.cuda.Stream()
    L = api.lib()
    for (w, h), kinds in [(s, ("loguniform", "nonfinite")) for s in GPU_SIZES] + [(STRIDE_SIZE, ("constant", "loguniform", "checker"))]:
        # three frames in a row on one handle: the histogram after each call is that frame's alone
        frames = [frame_of(kind, w, h) for kind in kinds] + [frame_of(kinds[0], w, h, seed=3)]
        frames = frames[:3]
        dts = [0.0, 1.0 / 30.0, 1.0 / 30.0]
        win = None if (w, h) != (131, 67) else (3, 2, 130, 67)
        prm = params_of(window=win)
        want = statement(libm, frames, prm, dts, 1)
        ex = api.AutoExposure(device=0, **prm)
        for k, fr in enumerate(frames):
            t = torch.from_numpy(fr.copy()).cuda()
            ldr = torch.zeros_like(t)
            rgb8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                ex.meter_into(t, dts[k])
                ex.apply_into(ldr, rgb8, t, "golden")
            hist, st = device_state(ex)
            if kinds[k % len(kinds)] == "constant" and k == 0:
                assert hist.max() == w * h and hist.sum() == w * h, "the constant frame: one bin holds every pixel"
            assert np.array_equal(bits(t.cpu().numpy()), bits(fr)), "the frame was written"
            assert_frame((hist, st, ldr.cpu().numpy(), rgb8.cpu().numpy()), want[k], f"meter_into / apply_into {w}x{h} frame {k}")
        # both forms of k_ex_histogram (per-wave counting, interleaved replicas), one launch each: the statement's counts
        for k, fr in enumerate(frames[:2]):
            t = torch.from_numpy(fr.copy()).cuda()
            for form in (0, 1):
                ms = ctypes.c_float()
                ep = api.make_exposure_params(**prm)
                api._check(L.yart_hip_debug_exposure_time(ex.handle, ctypes.c_void_p(t.data_ptr()), w, h, ctypes.byref(ep), form, 1, None, None,
                                                          ctypes.byref(ms)), L)
                assert np.array_equal(ex.state(histogram=True)["histogram"], want[k][0]), f"k_ex_histogram<{form}> {w}x{h} frame {k}"
        ex.reset()
        ex.meter_into(torch.from_numpy(frames[-1].copy()).cuda(), 0.0)
        # the fused pass against the entries it replaces, on the same device, with the metered handle's gain
        fr = frames[-1]
        want = statement(libm, [fr], prm, [0.0], 1)
        t = torch.from_numpy(fr.copy()).cuda()
        gain = torch.tensor(float(ex.state()["gain"]), dtype=torch.float32, device="cuda")
        assert gain.item() == float(want[-1][1]["gain"])
        prod = t.clone()
        prod[..., :3] = t[..., :3] * gain
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())
        for look in (0, 1, 2, -1):
            both_l, both_b = torch.zeros_like(t), torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            ex.apply_into(both_l, both_b, t, None if look < 0 else look)
            if look >= 0:
                pair_l, pair_b = torch.zeros_like(t), torch.zeros_like(both_b)
                api._check(L.yart_hip_tonemap_agx(ptr(prod), w, h, look, ptr(pair_l), None), L)
                api._check(L.yart_hip_encode_rgb8(ptr(pair_l), w, h, ptr(pair_b), None), L)
            else:
                pair_l, pair_b = prod, torch.zeros_like(both_b)
                api._check(L.yart_hip_encode_rgb8(ptr(prod), w, h, ptr(pair_b), None), L)
            assert np.array_equal(bits(both_l.cpu().numpy()), bits(pair_l.cpu().numpy())), f"fused ldr {w}x{h} look {look}"
            assert torch.equal(both_b, pair_b), f"fused rgb8 {w}x{h} look {look}"
            # either output absent: the other is unchanged; in place, too
            only_l, only_b = torch.zeros_like(t), torch.zeros_like(both_b)
            ex.apply_into(only_l, None, t, None if look < 0 else look)
            ex.apply_into(None, only_b, t, None if look < 0 else look)
            assert np.array_equal(bits(only_l.cpu().numpy()), bits(both_l.cpu().numpy())) and torch.equal(only_b, both_b), f"one output {w}x{h} look {look}"
            inplace = t.clone()
            ex.apply_into(inplace, None, inplace, None if look < 0 else look)
            assert np.array_equal(bits(inplace.cpu().numpy()), bits(both_l.cpu().numpy())), f"in place {w}x{h} look {look}"
        ex.close()
    print("child_into: ok")


@pytest.mark.gpu
def test_meter_into_and_apply_into(gpu_api):
    """AutoExposure.meter_into / apply_into — the device entries — on torch tensors, on a non-default stream, at every size and
    at 727 x 727 (STRIDE_SIZE above: k_ex_histogram's grid-stride loop runs twice, the last pass ragged), where the first frame is
    the constant one — every lane of every wave on one bin, the most contention the LDS histogram can see — and hist[bin] == N
    exactly. Three frames in a row on one handle: the histogram read back after each is that frame's alone. Both forms of
    k_ex_histogram — the kept one and the other — count what the statement counts. The fused apply
    against frame x gain in torch float32 through yart_hip_tonemap_agx and yart_hip_encode_rgb8 on the same device: equal on bits
    for looks 0, 1, 2; for look -1 ldr is the product and rgb8 its encoding; with either output absent the other is unchanged."""
    run_torch_child("child_into()")


def child_render_denoised():
    from yart_amd import api
    from yart_amd.exposure import ExposureState, apply_reference, exposure_reference, params_of
    libm = child_libm()
    from yart_amd import yscn
    from tests.test_lighting_update_host import scale_lights
    base = dict(load_params(os.path.join(GOLDEN, "cornell.txt")), size=(64, 64), spp=4)
    desc = yscn.Scene.load(os.path.join(GOLDEN, "cornell.yscn"))
    dim = scale_lights(desc, lambda i, l: True, 0.25)
    assert len(desc.lights) > 0 and all(l.type == 0 for l in desc.lights)
    scene = api.DeviceScene(desc, device=0)
    acc = api.TemporalAccumulator(64, 64, device=0)
    ex = api.AutoExposure(device=0)
    st = ExposureState()
    targets = []
    for k in range(3):
        if k == 1:                                       # from the second frame on: every light's emission (and its material's) at a quarter
            scene.update_lighting(materials=dim.materials, lights=dim.lights)
        noisy, clean, g = scene.render_denoised(base, temporal=acc, exposure=ex, dt=1.0 / 30.0, look="none")
        frame = clean.cpu().numpy()
        exposure_reference(st, frame, params_of(), 1.0 / 30.0, libm.log2f, libm.expf)
        dev = ex.state()
        assert_state(dev, st.asdict(), f"render_denoised frame {k}")
        ldr, rgb8 = apply_reference(frame, st.gain, "none", libm.log2f, libm.powf)
        assert tuple(g["display"].shape) == (64, 64, 4) and tuple(g["display_rgb8"].shape) == (64, 64, 3)
        assert np.array_equal(bits(g["display"].cpu().numpy()), bits(ldr)), f"display, frame {k}"
        assert np.array_equal(g["display_rgb8"].cpu().numpy(), rgb8), f"display_rgb8, frame {k}"
        targets.append(float(dev["target_ev"]))
        print(f"frame {k}: target_ev {dev['target_ev']} cur_ev {dev['cur_ev']} gain {dev['gain']}")
    assert targets[1] > targets[0], targets
    noisy, clean, g = scene.render_denoised(base, temporal=acc)
    assert "display" not in g and "display_rgb8" not in g
    scene.close()
    acc.close()
    ex.close()
    print("child_render_denoised: ok")


@pytest.mark.gpu
def test_render_denoised_with_auto_exposure(gpu_api):
    """DeviceScene.render_denoised(temporal=acc, exposure=ex, dt=1/30, look="none") on cornell.yscn at 64 x 64, three frames, every
    light's emission dimmed to a quarter with update_lighting from the second frame on: "display" and "display_rgb8" are
    apply_reference of the returned denoised frame at the statement's state, on bits; the state is the statement's; the second
    frame's target_ev is above the first's. Without exposure= the guides are what they were."""
    run_torch_child("child_render_denoised()")
