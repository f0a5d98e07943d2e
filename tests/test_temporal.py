"""Temporal accumulation with camera reprojection (include/yart_hip.h: yart_hip_temporal_*, YartTemporalParams).

The definition is the header comment; yart_amd/temporal.py `temporal_reference` states it in NumPy float32 and is the reference
of every comparison here, on bits: csrc/temporal.hpp compiled for the host (tests/temporalsim `accumulate`) and the device
kernel through api.TemporalAccumulator.accumulate / accumulate_into / DeviceScene.render_denoised(temporal=...). The inputs are
an analytic scene seen through real cameras, so that reprojection really succeeds: the planes z = 0 (normal +z) and z = 6
(normal -z) and, in front of the first, the half plane z = 2, x < 0.35; node ids from a world-space checkerboard per plane.
The quality test holds the default parameters to "better than not accumulating" on an orbit of the cornell scene."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT, bit_identical_or_drift
from tests.paramfile import load_params

CPU_SIZES = [(1, 1), (5, 3), (37, 23)]                  # (width, height)
GPU_SIZES = CPU_SIZES + [(131, 67)]                     # + several workgroups in both directions, no multiple of 16
SEQUENCES = ["static", "subpixel", "move", "away", "reset"]
FRAMES = 3
# parameters at which every branch is taken on these inputs: the cap binds in frame 3, the floor does not
PARAMS = dict(alpha_min=0.2, max_history=2, normal_cos_min=0.95, plane_tolerance=0.01)
EDGE, CELL_PIXELS = 0.35, 6.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene, in float64
# ---------------------------------------------------------------------------------------------------------------------
def base_camera(w, h):
    return dict(size=(w, h), focal=35.0, sensor=(36.0, 24.0), eye=(0.1, 0.2, 5.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))


def pixel_world(w, h):
    """edge of a pixel on the plane z = 0, for the base camera"""
    from yart_amd.temporal import camera_basis
    return float(np.linalg.norm(camera_basis(base_camera(w, h))["dU"].astype(np.float64)))


def cameras(w, h, seq):
    """The three cameras of a sequence. The moves are in pixels of the image, so that every size sees the same thing."""
    px = pixel_world(w, h)
    cam = base_camera(w, h)

    def moved(k, shift_px, turn_px=0.0):
        e, t = np.array(cam["eye"]), np.array(cam["target"])
        e = e + k * np.array([shift_px * px, 0.37 * shift_px * px, 0.0])
        t = t + k * np.array([(shift_px + turn_px) * px, 0.0, 0.0])
        return dict(cam, eye=tuple(float(v) for v in e), target=tuple(float(v) for v in t))
    if seq == "static":
        return [cam, cam, cam]
    if seq in ("subpixel", "reset"):
        return [moved(k, 0.3, 0.11) for k in range(FRAMES)]
    if seq == "move":                                   # a translation and a turn, ~0.15 of the width per frame, at least 3 pixels
        s = max(3.0, 0.11 * w)
        return [moved(k, s, 0.4 * s) for k in range(FRAMES)]
    assert seq == "away"                                # every other camera looks the other way: all points are behind the previous one
    back = dict(cam, target=(0.0, 0.0, 10.0))
    return [cam, back, cam]


def camera64(cam):
    """position, top-left pixel centre, pixel steps: derived here in float64 from the description, not from camera_basis"""
    w, h = cam["size"]
    eye, target, up = (np.array(cam[k], np.float64) for k in ("eye", "target", "up"))
    aspect = w / h
    cropped = cam["sensor"][0] / max(cam["sensor"][0] / cam["sensor"][1], aspect)
    fwd = target - eye
    focus = np.linalg.norm(fwd)
    vh = focus * cropped / cam["focal"]
    vw = vh * aspect
    wv = -fwd / focus
    u = np.cross(up / np.linalg.norm(up), wv)
    v = np.cross(wv, u)
    du, dv = u * vw / w, -v * vh / h
    tl = eye - wv * focus - (u * vw - v * vh) / 2 + (du + dv) / 2
    return eye, tl, du, dv


def surface(o, d, cell):
    """first surface along o + t d (arrays (..., 3)): t, plane index (0: z = 0, 1: z = 2 half plane, 2: z = 6; -1: none), node id"""
    with np.errstate(all="ignore"):
        best_t = np.full(d.shape[:-1], np.inf)
        plane = np.full(d.shape[:-1], -1)
        for idx, z in ((0, 0.0), (1, 2.0), (2, 6.0)):
            t = (z - o[..., 2]) / d[..., 2]
            x = o[..., 0] + t * d[..., 0]
            ok = np.isfinite(t) & (t > 0) & (t < best_t)
            if idx == 1:
                ok &= x < EDGE
            best_t = np.where(ok, t, best_t)
            plane = np.where(ok, idx, plane)
        p = o + best_t[..., None] * d
        ix = np.floor(p[..., 0] / cell).astype(np.int64) + 512
        iy = np.floor(p[..., 1] / cell).astype(np.int64) + 512
    node = np.where(plane >= 0, plane * (1 << 20) + ix * 1024 + iy, -1)
    return best_t, plane, node, p


def see(cam, cell):
    """what every pixel centre of `cam` sees: (t, plane, node, P) in float64, (H, W, ...)"""
    w, h = cam["size"]
    eye, tl, du, dv = camera64(cam)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = tl + xs[..., None] * du + ys[..., None] * dv - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return surface(np.broadcast_to(eye, d.shape), d, cell)


_frames, _reference = {}, {}


def frames_of(w, h, seq):
    """The three frames of a sequence: camera, frame, variance and feature buffers. Frame and variance are the seeded random
    values of tests/test_denoise_var.py::inputs (fireflies, a NaN, an Inf, a negative and a huge variance), another draw per
    frame; coverage is < 1 on a few per cent of the pixels; albedo has exact zeros; a normal and a position are not finite once."""
    if (w, h, seq) not in _frames:
        cell = CELL_PIXELS * pixel_world(w, h)
        out = []
        for k, cam in enumerate(cameras(w, h, seq)):
            rng = np.random.RandomState(1000 * w + 10 * h + k)
            n = w * h
            t, plane, node, p = see(cam, cell)
            assert (plane >= 0).all()
            rgba = rng.uniform(0, 50, (h, w, 4)).astype(np.float32)
            rgba[..., 3] = rng.uniform(0, 1, (h, w))
            flat = rgba.reshape(n, 4)
            for i in rng.choice(n, n // 50, replace=False):
                flat[i, rng.randint(3)] = 1e4
            nz = np.where(plane == 2, -1.0, 1.0)
            nrm = (np.stack([np.zeros((h, w)), np.zeros((h, w)), nz], -1) + rng.normal(0, 0.02, (h, w, 3))).astype(np.float32)
            alb = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
            alb[rng.rand(h, w, 3) < 0.05] = 0.0
            var = (rng.uniform(0, 40, (h, w)) * rng.uniform(0, 1, (h, w)) ** 4).astype(np.float32)
            var[rng.rand(h, w) < 0.1] = 0.0
            var[rng.rand(h, w) < 0.03] = 1e30
            cov = np.ones((h, w), np.float32)
            cov[rng.rand(h, w) < 0.04] = 0.75
            pos = p.astype(np.float32)
            depth = t.astype(np.float32)
            ids = np.stack([node, np.zeros_like(node), plane, node % 7], -1).astype(np.int32)
            if n >= 8:
                flat[n // 3, 1] = np.nan
                flat[(2 * n) // 3, 0] = np.inf
                vf = var.reshape(n)
                vf[n // 5] = np.nan
                vf[(2 * n) // 5] = -1.0
                vf[(3 * n) // 5] = np.inf
                nrm.reshape(n, 3)[n // 7, 2] = np.nan
                pos.reshape(n, 3)[n // 9, 0] = np.inf
                depth.reshape(n)[n // 11] = np.nan
                alb.reshape(n, 3)[n // 13, 1] = np.nan
            out.append(dict(camera=cam, rgba=rgba, variance=var, position=pos, normal=nrm, depth=depth, coverage=cov, ids=ids, albedo=alb))
        for f in out:
            for v in f.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _frames[(w, h, seq)] = out
    return _frames[(w, h, seq)]


def aovs_of(f, demodulate):
    names = ("position", "normal", "depth", "coverage", "ids") + (("albedo",) if demodulate else ())
    return {k: f[k] for k in names}


def reference(w, h, seq, demodulate, params=None):
    """temporal_reference over the sequence -> [(frame, variance, length)] per frame, computed once"""
    from yart_amd.temporal import TemporalHistory, temporal_reference
    prm = dict(PARAMS if params is None else params)
    key = (w, h, seq, demodulate, tuple(sorted(prm.items())))
    if key not in _reference:
        hist = TemporalHistory(w, h)
        res = []
        for k, f in enumerate(frames_of(w, h, seq)):
            if seq == "reset" and k == 2:
                hist.reset()
            a = aovs_of(f, True)
            r = temporal_reference(hist, f["camera"], f["rgba"], f["variance"], a["position"], a["normal"], a["depth"], a["coverage"],
                                   a["ids"], a["albedo"] if demodulate else None, demodulate=demodulate, **prm)
            for v in r:
                v.setflags(write=False)
            res.append(r)
        _reference[key] = res
    return _reference[key]


def assert_same(got, want, tag):
    for name, g, w_ in zip(("frame", "variance", "length"), got, want):
        diff = bits(g) != bits(w_)
        assert not diff.any(), f"{tag} {name}: {int(diff.sum())} words differ, first at {np.argwhere(diff)[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def test_temporal_abi_and_argument_errors(built, tmp_path):
    """The symbols exist and are in api.EXPORTS, the ABI is still 3, YartTemporalParams and the defaults agree between ctypes,
    yart_amd/temporal.py and a C++ compiler (which also sees yart::hip::Temporal), and every argument error is YART_E_INVALID with
    a telling message — a handle is made without a device, and none is touched."""
    from yart_amd import api, temporal
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    for name in ("yart_hip_temporal_create", "yart_hip_temporal_destroy", "yart_hip_temporal_reset",
                 "yart_hip_temporal_accumulate_device", "yart_hip_temporal_accumulate_host"):
        assert hasattr(raw, name), name
        assert name in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %u\\n\", sizeof(YartTemporalParams), YART_TEMPORAL_DEFAULT_MAX_HISTORY);\n"
                "  std::printf(\"%.9g %.9g %.9g\\n\", YART_TEMPORAL_DEFAULT_ALPHA_MIN, YART_TEMPORAL_DEFAULT_NORMAL_COS_MIN, YART_TEMPORAL_DEFAULT_PLANE_TOLERANCE);\n"
                "  yart::hip::Temporal t(4, 4);\n"
                "  yart::hip::TemporalFrame (yart::hip::Temporal::*fn)(const YartCameraDesc&, const std::vector<float>&, const std::vector<float>&, const yart::hip::TemporalFeatures&, const YartTemporalParams&) = &yart::hip::Temporal::accumulate;\n"
                "  t.reset();\n"
                "  return fn && yart::hip::temporalDefaults().struct_size == sizeof(YartTemporalParams) ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:2]] == [ctypes.sizeof(api.TemporalParams), temporal.DEFAULT_MAX_HISTORY]
    assert ctypes.sizeof(api.TemporalParams) == 24
    assert [np.float32(v) for v in out[2:]] == [np.float32(v) for v in (temporal.DEFAULT_ALPHA_MIN, temporal.DEFAULT_NORMAL_COS_MIN,
                                                                     temporal.DEFAULT_PLANE_TOLERANCE)]
    # the existing structs are frozen
    assert ctypes.sizeof(api.DenoiseVarParams) == 24 and ctypes.sizeof(api.AovBuffers) == 8 + 7 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(api.CameraDesc) == 68

    h = ctypes.c_void_p()
    assert L.yart_hip_temporal_create(4, 4, 0, None) == api.YART_E_INVALID and b"null" in L.yart_hip_last_error()
    assert L.yart_hip_temporal_create(0, 4, 0, ctypes.byref(h)) == api.YART_E_INVALID and b"width" in L.yart_hip_last_error()
    assert L.yart_hip_temporal_create(4, 0, 0, ctypes.byref(h)) == api.YART_E_INVALID and b"height" in L.yart_hip_last_error()
    assert L.yart_hip_temporal_create(1 << 15, 1 << 14, 0, ctypes.byref(h)) == api.YART_E_INVALID and b"2^28" in L.yart_hip_last_error()
    assert L.yart_hip_temporal_reset(None) == api.YART_E_INVALID
    assert L.yart_hip_temporal_create(4, 4, 0, ctypes.byref(h)) == api.YART_OK and h.value
    assert L.yart_hip_temporal_reset(h) == api.YART_OK
    buf = np.zeros((4, 4, 4), np.float32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    cam_ok = api.make_camera(base_camera(4, 4))
    needed = ("position", "normal", "depth", "coverage", "ids")

    def call(device, handle=h, cam=cam_ok, rgba=ptr, variance=ptr, aovs=needed, aov_null=None, aov_size=None, have_aovs=True,
             out=ptr, params=True, **over):
        tp = api.make_temporal_params()
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
        if device:
            return L.yart_hip_temporal_accumulate_device(handle, pc, rgba, variance, pa, pp, out, None, None, None)
        return L.yart_hip_temporal_accumulate_host(handle, pc, rgba, variance, pa, pp, out, None, None)

    cam_size = api.make_camera(base_camera(5, 4))
    cases = [(dict(handle=None), b"handle"), (dict(cam=None), b"camera"), (dict(rgba=None), b"null"), (dict(out=None), b"null"),
             (dict(variance=None), b"variance"), (dict(have_aovs=False), b"aovs"), (dict(params=False), b"params"),
             (dict(struct_size=20), b"struct_size"), (dict(struct_size=0), b"struct_size"),
             (dict(flags=2), b"flags"), (dict(flags=1 | 0x80000000), b"flags"),
             (dict(alpha_min=float("nan")), b"finite"), (dict(normal_cos_min=float("inf")), b"finite"),
             (dict(plane_tolerance=float("-inf")), b"finite"), (dict(alpha_min=-0.01), b"alpha_min"), (dict(alpha_min=1.5), b"alpha_min"),
             (dict(max_history=0), b"max_history"), (dict(cam=cam_size), b"size"),
             (dict(flags=api.FLAG_TEMPORAL_DEMODULATE), b"albedo"), (dict(aov_size=4), b"struct_size"),
             (dict(aovs=needed + ("albedo",), aov_size=16, flags=0), b"missing")]
    cases += [(dict(aovs=tuple(n for n in needed if n != miss)), miss.encode()) for miss in needed]
    cases += [(dict(aov_null=miss), miss.encode()) for miss in needed]
    for device in (False, True):
        for kw, word in cases:
            assert call(device, **kw) == api.YART_E_INVALID, (device, kw)
            assert word in L.yart_hip_last_error(), (device, kw, L.yart_hip_last_error())
        if L.yart_hip_device_count() == 0:             # well-formed arguments, no device: that, and nothing else
            assert call(device) == api.YART_E_NO_DEVICE
            assert call(device, aovs=needed + ("albedo",), flags=api.FLAG_TEMPORAL_DEMODULATE) == api.YART_E_NO_DEVICE
    L.yart_hip_temporal_destroy(h)
    L.yart_hip_temporal_destroy(None)


def hand_camera(w):
    """A camera whose derived quantities are exact binary32 numbers: eye (0, 0, 5) looking at the origin, focal 30 on a 36 x 24
    sensor. 1 x 1: the pixel is 4 x 4 world units and its centre the origin. 2 x 1: pixels of 3 x 3, centres (-1.5, 0, 0), (1.5, 0, 0)."""
    return dict(size=(w, 1), focal=30.0, sensor=(36.0, 24.0), eye=(0.0, 0.0, 5.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))


def hand_frame(w, colour, var, xs, z=0.0, node=7, normal=(0.0, 0.0, 1.0), coverage=1.0):
    f = np.float32
    rgba = np.zeros((1, w, 4), f)
    rgba[0, :, :3] = np.asarray(colour, f).reshape(-1, 1) if np.ndim(colour) == 1 and w > 1 else colour
    rgba[..., 3] = 0.25
    pos = np.zeros((1, w, 3), f)
    pos[0, :, 0] = xs
    pos[0, :, 2] = z
    ids = np.zeros((1, w, 4), np.int32)
    ids[..., 0] = node
    return dict(rgba=rgba, variance=np.full((1, w), var, f), position=pos, normal=np.tile(np.asarray(normal, f), (1, w, 1)),
                depth=(5.0 - pos[..., 2]).astype(f), coverage=np.full((1, w), coverage, f), ids=ids)


def run_hand(hist, cam, fr, **kw):
    from yart_amd.temporal import temporal_reference
    return temporal_reference(hist, cam, fr["rgba"], fr["variance"], fr["position"], fr["normal"], fr["depth"], fr["coverage"],
                              fr["ids"], fr.get("albedo"), **kw)


def test_numpy_statement_on_hand_made_inputs():
    """temporal_reference on 1- and 2-pixel frames whose answer is worked out by hand."""
    from yart_amd.temporal import TemporalHistory, camera_basis
    f = np.float32
    cam = hand_camera(1)
    k = camera_basis(cam)
    assert k["top_left"].tolist() == [0, 0, 0] and k["dU"].tolist() == [4, 0, 0] and k["dV"].tolist() == [0, -4, 0]
    kw = dict(alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01)
    # a first frame: out = c, v_out = v, length 1, alpha kept
    hist = TemporalHistory(1, 1)
    a = hand_frame(1, 8.0, 2.0, [0.0])
    out, var, ln = run_hand(hist, cam, a, **kw)
    assert np.array_equal(bits(out), bits(a["rgba"])) and var[0, 0] == 2 and ln[0, 0] == 1
    # a static second frame: N = 2, a = 1/2: out = 8 + (4 - 8) / 2 = 6, v = 4 / 4 + 2 / 4 = 1.5
    b = hand_frame(1, 4.0, 4.0, [0.0])
    out, var, ln = run_hand(hist, cam, b, **kw)
    assert out[0, 0].tolist() == [6, 6, 6, 0.25] and var[0, 0] == 1.5 and ln[0, 0] == 2
    # a third: N = 3, a = float32(1 / 3)
    third = f(1) / f(3)
    out, var, ln = run_hand(hist, cam, hand_frame(1, 9.0, 0.0, [0.0]), **kw)
    want = f(6) + third * (f(9) - f(6))
    assert out[0, 0, 0] == want and ln[0, 0] == 3
    assert var[0, 0] == (third * third) * f(0) + ((f(1) - third) * (f(1) - third)) * f(1.5)
    # the alpha_min floor: the same third frame with alpha_min = 0.75 -> 6 + 0.75 * 3
    # the max_history cap: with max_history = 2 the third frame blends with a = 1/2 again and its length stays 2
    for over, want_c, want_n in ((dict(alpha_min=0.75), 8.25, 3), (dict(max_history=2), 7.5, 2)):
        hist = TemporalHistory(1, 1)
        run_hand(hist, cam, a, **kw)
        run_hand(hist, cam, b, **kw)
        out, var, ln = run_hand(hist, cam, hand_frame(1, 9.0, 0.0, [0.0]), **dict(kw, **over))
        assert out[0, 0, 0] == want_c and ln[0, 0] == want_n
    # reset: a first frame again
    hist.reset()
    out, var, ln = run_hand(hist, cam, b, **kw)
    assert np.array_equal(bits(out), bits(b["rgba"])) and ln[0, 0] == 1
    # each of the five tap conditions failing alone, against the control in which the tap counts (length 2)
    def second(first_over=None, **over):
        hist = TemporalHistory(1, 1)
        run_hand(hist, cam, hand_frame(1, 8.0, 2.0, [0.0], **(first_over or {})), **kw)
        fr = hand_frame(1, 4.0, 4.0, [over.pop("x", 0.0)], **over)
        out, var, ln = run_hand(hist, cam, fr, **kw)
        return out[0, 0, 0], var[0, 0], ln[0, 0]
    assert second() == (6, 1.5, 2)
    assert second(x=6.0) == (4, 4, 1)                                   # projects to jx = 1.5: no tap inside the image
    assert second(first_over=dict(coverage=0.5)) == (6, 1.5, 2)         # (a partly covered pixel still leaves a record of length 1)
    hist = TemporalHistory(1, 1)
    bad = hand_frame(1, np.nan, 2.0, [0.0])
    out, var, ln = run_hand(hist, cam, bad, **kw)                       # not usable: passed through, a record of length 0
    assert np.array_equal(bits(out), bits(bad["rgba"])) and var[0, 0] == 2 and ln[0, 0] == 0 and hist.length[0, 0] == 0
    out, var, ln = run_hand(hist, cam, b, **kw)
    assert (out[0, 0, 0], var[0, 0], ln[0, 0]) == (4, 4, 1)             # history length 0: no tap
    assert second(node=8) == (4, 4, 1)                                  # another node
    assert second(normal=(1.0, 0.0, 0.0)) == (4, 4, 1)                  # dot(n, n_hist) = 0 < 0.9
    assert second(normal=(0.0, 0.4375, 0.9)) == (6, 1.5, 2)             # ... and 0.9 >= 0.9
    assert second(z=1.0) == (4, 4, 1)                                   # on the axis, 1 off the plane: 1 > 0.01 * 4
    assert second(z=0.03125) == (6, 1.5, 2)                             # 0.03125 <= 0.01 * 4.96875
    assert second(coverage=0.5) == (4, 4, 1) and second(z=6.0) == (4, 4, 1)     # not reprojectable; behind the previous camera
    # two pixels, a point between them: both taps at weight 1/2; then with one of them on another node
    cam2 = hand_camera(2)
    k = camera_basis(cam2)
    assert k["top_left"].tolist() == [-1.5, 0, 0] and k["dU"].tolist() == [3, 0, 0]
    for node1, want_c, want_v, want_n in ((7, 10.0, 2.0, 2), (9, 6.0, 1.5, 2)):
        hist = TemporalHistory(2, 1)
        first = hand_frame(2, 8.0, 2.0, [-1.5, 1.5])
        first["rgba"][0, 1, :3], first["variance"][0, 1], first["ids"][0, 1, 0] = 24.0, 6.0, node1
        run_hand(hist, cam2, first, **kw)
        out, var, ln = run_hand(hist, cam2, hand_frame(2, 4.0, 4.0, [0.0, 9.0]), **kw)
        # node 7: h = (8 / 2 + 24 / 2) / 1 = 16, v_h = (2 / 2 + 6 / 2) / 1 = 4: out = 16 + (4 - 16) / 2 = 10, v = 4 / 4 + 4 / 4 = 2
        # node 9: only the left tap counts: h = (8 / 2) / (1 / 2) = 8, v_h = 2: out = 6, v = 4 / 4 + 2 / 4 = 1.5
        assert (out[0, 0, 0], ln[0, 0]) == (want_c, want_n) and var[0, 0] == want_v
        assert (out[0, 1, 0], var[0, 1], ln[0, 1]) == (4, 4, 1)         # x = 9 projects to jx = 3.5: outside
    # demodulation: albedo 0.5 / 0 (-> 1) / 2: accumulated in rgb / d, returned * d; the variance over luma(d)^2 and back
    hist = TemporalHistory(1, 1)
    alb = np.array([[[0.5, 0.0, 2.0]]], f)
    run_hand(hist, cam, dict(a, albedo=alb), **kw)
    out, var, ln = run_hand(hist, cam, dict(b, albedo=alb), **kw)
    assert out[0, 0].tolist() == [6, 6, 6, 0.25] and ln[0, 0] == 2 and hist.colour[0, 0].tolist() == [12, 6, 3]
    ld = (f(0.5) * f(0.2126) + f(1) * f(0.7152)) + f(2) * f(0.0722)
    v1, v2 = f(2) / (ld * ld), f(4) / (ld * ld)
    assert var[0, 0] == (f(0.25) * v2 + f(0.25) * v1) * (ld * ld)


def _build_sim(path):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", path,
                           os.path.join(ROOT, "tests", "temporalsim", "temporalsim.cpp"),
                           os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def temporalsim(built, tmp_path_factory):
    """tests/temporalsim/temporalsim.cpp: csrc/temporal.hpp compiled for the host, and the host path tracer with feature buffers"""
    exe = str(tmp_path_factory.mktemp("temporalsim") / "temporalsim")
    r = _build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_sim(exe, tmp, w, h, seq, demodulate, in_place, params=None):
    from yart_amd import api
    prm = dict(PARAMS if params is None else params)
    n = w * h
    fin, fout = os.path.join(tmp, "tp.in"), os.path.join(tmp, "tp.out")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, FRAMES, 1 if demodulate else 0, 1 if in_place else 0, prm["max_history"]], np.uint32).tobytes())
        f.write(np.array([prm["alpha_min"], prm["normal_cos_min"], prm["plane_tolerance"]], np.float32).tobytes())
        for k, fr in enumerate(frames_of(w, h, seq)):
            f.write(np.array([1 if seq == "reset" and k == 2 else 0], np.uint32).tobytes())
            f.write(bytes(api.make_camera(fr["camera"])))
            for name in ("rgba", "variance", "position", "normal", "depth", "coverage", "ids", "albedo"):
                f.write(fr[name].tobytes())
    r = subprocess.run([exe, "accumulate", fin, fout], capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    words = np.fromfile(fout, np.uint32).reshape(FRAMES, n * 6)
    return r, [(words[k, :n * 4].view(np.float32).reshape(h, w, 4), words[k, n * 4:n * 5].view(np.float32).reshape(h, w),
                words[k, n * 5:].reshape(h, w)) for k in range(FRAMES)]


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_equals_the_numpy_statement_on_bits(temporalsim, tmp_path, w, h):
    """csrc/temporal.hpp on the host == temporal_reference, bit for bit: every camera sequence, demodulation on and off, out of
    place and in place, all three frames (so: both history images, and the history itself through the next frame)."""
    for seq in SEQUENCES:
        for dm in (False, True):
            want = reference(w, h, seq, dm)
            for in_place in (False, True):
                r, got = run_sim(temporalsim, str(tmp_path), w, h, seq, dm, in_place)
                assert r.returncode == 0, r.stderr
                for k in range(FRAMES):
                    assert_same(got[k], want[k], f"{w}x{h} {seq} demodulate {dm} in_place {in_place} frame {k}")


@pytest.mark.parametrize("w,h", [(37, 23), (131, 67)])
def test_the_inputs_take_both_branches(w, h):
    """A condition on the inputs, checked on the NumPy statement: in the last frame of the multi-pixel move at least a tenth of the
    pixels have a history (length > 1) and at least a tenth have none (length 1); the cap and the growing length both occur; the
    static sequence keeps nearly everything, the turned-away one and the reset nothing."""
    n = w * h
    ln = reference(w, h, "move", False)[2][2]
    assert (ln > 1).sum() >= n / 10 and (ln == 1).sum() >= n / 10, ((ln > 1).sum(), (ln == 1).sum(), n)
    grown = reference(w, h, "move", False, dict(PARAMS, max_history=8))[2][2]
    assert (grown == 3).sum() >= n / 10 and (grown == 2).sum() > 0 and ln.max() == 2
    for seq in ("static", "subpixel"):
        assert (reference(w, h, seq, True)[2][2] == 2).sum() >= 0.8 * n
    for seq in ("away", "reset"):
        assert (reference(w, h, seq, True)[2][2] <= 1).all()
    assert (reference(w, h, "reset", True)[1][2] == 2).sum() >= 0.8 * n
    assert (reference(w, h, "static", False)[0][2] == 0).sum() >= 4          # the unusable pixels


@pytest.mark.parametrize("w,h", [(37, 23), (131, 67)])
def test_disocclusions_start_a_new_history(w, h):
    """Frame 2 of the multi-pixel move: a pixel whose surface point projects, in the previous frame, among four pixels that all saw
    another surface (the other plane, or another cell of the checkerboard) has length 1 and out == c. Which pixels those are is
    worked out here in float64 from the scene, for points that project at least a pixel inside the previous image and not within
    0.02 pixel of a pixel row or column."""
    cams = cameras(w, h, "move")
    cell = CELL_PIXELS * pixel_world(w, h)
    _, _, node_prev, _ = see(cams[0], cell)
    _, plane, node, p = see(cams[1], cell)
    eye, tl, du, dv = camera64(cams[0])
    nrm = np.cross(du, dv)
    rel = p - eye
    s = np.dot(tl - eye, nrm) / (rel @ nrm)
    X = eye + rel * s[..., None] - tl
    jx, jy = (X @ du) / (du @ du), (X @ dv) / (dv @ dv)
    sure = (s > 0) & (jx > 1) & (jx < w - 2) & (jy > 1) & (jy < h - 2)
    sure &= (np.abs(jx - np.round(jx)) > 0.02) & (np.abs(jy - np.round(jy)) > 0.02)
    x0, y0 = np.floor(np.where(sure, jx, 0)).astype(int), np.floor(np.where(sure, jy, 0)).astype(int)
    other = sure.copy()
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        other &= node_prev[np.clip(y0 + dy, 0, h - 1), np.clip(x0 + dx, 0, w - 1)] != node
    fr = frames_of(w, h, "move")[1]
    out, var, ln = reference(w, h, "move", False)[1]
    usable = np.isfinite(fr["rgba"][..., :3]).all(-1) & np.isfinite(fr["variance"]) & (fr["variance"] >= 0)
    pick = other & usable
    assert pick.sum() >= max(4, 0.01 * w * h), int(pick.sum())
    assert (ln[pick] == 1).all()
    assert np.array_equal(bits(out[pick]), bits(fr["rgba"][pick])) and np.array_equal(bits(var[pick]), bits(fr["variance"][pick]))
    # and the other way round: where all four saw this very surface, the usable, fully covered pixels have a history
    same = sure & usable & (fr["coverage"] == 1) & np.isfinite(fr["position"]).all(-1) & np.isfinite(fr["normal"]).all(-1) & np.isfinite(fr["depth"])
    prev = frames_of(w, h, "move")[0]
    prev_ok = np.isfinite(prev["rgba"][..., :3]).all(-1) & np.isfinite(prev["variance"]) & (prev["variance"] >= 0)
    facing = np.zeros((h, w), bool)                     # the normals are noisy: at least one tap clearly passes normal_cos_min
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        qy, qx = np.clip(y0 + dy, 0, h - 1), np.clip(x0 + dx, 0, w - 1)
        same &= (node_prev[qy, qx] == node) & prev_ok[qy, qx] & np.isfinite(prev["position"][qy, qx]).all(-1) & np.isfinite(prev["normal"][qy, qx]).all(-1)
        with np.errstate(all="ignore"):
            facing |= (fr["normal"].astype(np.float64) * prev["normal"][qy, qx].astype(np.float64)).sum(-1) >= PARAMS["normal_cos_min"] + 0.01
    same &= facing
    assert same.sum() >= 0.1 * w * h and (ln[same] == 2).all()


# -- quality: the gate of the default parameters -----------------------------------------------------------------------------
ORBIT_FRAMES, ORBIT_STEP_DEGREES, ORBIT_SPP, ORBIT_HI_SPP = 6, 1.5, 4, 1024


def orbit_eyes(p, frames=ORBIT_FRAMES, step=ORBIT_STEP_DEGREES):
    """eye positions of an orbit about the vertical axis through the target, `step` degrees per frame, as binary32 values"""
    eye, target = np.array(p["eye"], np.float64), np.array(p["target"], np.float64)
    out = []
    for k in range(frames):
        a = np.radians(step * k)
        d = eye - target
        e = target + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
        out.append(tuple(float(np.float32(v)) for v in e))
    return out


def render_orbit_frame(exe, tmp, name, size, spp, eye, threads=None):
    """tests/temporalsim `render` -> dict(camera, rgba, variance, albedo, normal, position, depth, coverage, ids)"""
    w, h = size
    base = [ln for ln in open(os.path.join(GOLDEN, name + ".txt")).read().splitlines()
            if ln.split()[0] not in ("size", "spp", "threads", "probe_pixels")]
    pp, fp = os.path.join(tmp, f"{name}_orbit.txt"), os.path.join(tmp, f"{name}_orbit.out")
    with open(pp, "w") as f:
        f.write("\n".join(base + [f"size {w} {h}", f"spp {spp}", f"threads {threads or min(16, os.cpu_count() or 1)}"]) + "\n")
    subprocess.run([exe, "render", os.path.join(GOLDEN, name + ".yscn"), pp] + [f"{v:.9g}" for v in eye] + [fp], check=True)
    words = np.fromfile(fp, np.uint32).reshape(h, w, 20)
    fl = words.view(np.float32)
    p = dict(load_params(pp), eye=eye)
    return dict(camera=p, rgba=fl[..., 0:4].copy(), variance=fl[..., 4].copy(), albedo=fl[..., 5:8].copy(), normal=fl[..., 8:11].copy(),
                position=fl[..., 11:14].copy(), depth=fl[..., 14].copy(), coverage=fl[..., 15].copy(), ids=words[..., 16:20].view(np.int32).copy())


def accumulate_orbit(frames, **kw):
    from yart_amd.temporal import TemporalHistory, temporal_reference
    h, w = frames[0]["rgba"].shape[:2]
    hist = TemporalHistory(w, h)
    for fr in frames:
        r = temporal_reference(hist, fr["camera"], fr["rgba"], fr["variance"], fr["position"], fr["normal"], fr["depth"], fr["coverage"],
                               fr["ids"], fr["albedo"], demodulate=True, **kw)
    return r


def host_tonemap(hostsim, tmp, frame):
    h, w = frame.shape[:2]
    src, dst = os.path.join(tmp, "t.in"), os.path.join(tmp, "t.out")
    np.ascontiguousarray(frame, np.float32).tofile(src)
    subprocess.run([hostsim, "tonemap", src, str(w), str(h), "none", dst, os.path.join(tmp, "t.ppm")], check=True)
    return np.fromfile(dst, np.float32).reshape(h, w, 4)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def test_default_parameters_beat_not_accumulating(hostsim, temporalsim, tmp_path):
    """A 6-frame orbit of cornell.yscn at 96 x 96 and 4 spp, rendered here by the host path tracer with its feature buffers and
    variance (tests/temporalsim `render`); tests/golden/temporal/cornell_orbit_hi.f32 is the last camera's frame at 1024 spp
    (tools/temporal_sweep.py --fixtures). RMSE over the AgX-tonemapped frames: at the defaults the accumulated last frame is
    strictly closer to the 1024-spp frame than the last 4-spp frame alone, and the accumulated frame followed by the
    variance-guided filter is no further from it than the variance-guided filter of the last frame alone."""
    from yart_amd.denoise import atrous_var_reference
    p = load_params(os.path.join(GOLDEN, "cornell.txt"))
    frames = [render_orbit_frame(temporalsim, str(tmp_path), "cornell", (96, 96), ORBIT_SPP, eye) for eye in orbit_eyes(p)]
    hi = np.fromfile(os.path.join(GOLDEN, "temporal", "cornell_orbit_hi.f32"), np.float32).reshape(96, 96, 4)
    last = frames[-1]
    acc, acc_var, length = accumulate_orbit(frames)
    assert (length == ORBIT_FRAMES).mean() > 0.5
    guides = (last["albedo"], last["normal"], last["depth"])
    tm = lambda x: host_tonemap(hostsim, str(tmp_path), x)
    ref = tm(hi)
    noisy, accumulated = rmse(tm(last["rgba"]), ref), rmse(tm(acc), ref)
    spatial = rmse(tm(atrous_var_reference(last["rgba"], last["variance"], *guides)), ref)
    both = rmse(tm(atrous_var_reference(acc, acc_var, *guides)), ref)
    print(f"cornell orbit: RMSE last frame {noisy:.5f}, accumulated {accumulated:.5f} (ratio {accumulated / noisy:.4f}); "
          f"filtered alone {spatial:.5f}, accumulated and filtered {both:.5f} (ratio {both / spatial:.4f})")
    assert accumulated < noisy
    assert both <= spatial


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def device_sequence(api, w, h, seq, demodulate, in_place):
    acc = api.TemporalAccumulator(w, h, device=0, **PARAMS)
    res = []
    for k, fr in enumerate(frames_of(w, h, seq)):
        if seq == "reset" and k == 2:
            acc.reset()
        frame, var = fr["rgba"].copy(), fr["variance"].copy()
        got = acc.accumulate(fr["camera"], frame, var, aovs_of(fr, demodulate), demodulate=demodulate,
                             out=frame if in_place else None, out_variance=var if in_place else None)
        if not in_place:
            assert np.array_equal(bits(frame), bits(fr["rgba"])) and np.array_equal(bits(var), bits(fr["variance"]))
        res.append(got)
    acc.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_accumulate_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_tp_accumulate through api.TemporalAccumulator.accumulate == temporal_reference, bit for bit: frame, variance and length of
    all three frames (the history through the next frame's result), every camera sequence, demodulation on and off, out of place
    and with the outputs aliasing the inputs."""
    for seq in SEQUENCES:
        for dm in (False, True):
            want = reference(w, h, seq, dm)
            for in_place in (False, True):
                got = device_sequence(gpu_api, w, h, seq, dm, in_place)
                for k in range(FRAMES):
                    tag = f"temporal {w}x{h} {seq} demodulate {dm} in_place {in_place} frame {k}"
                    bit_identical_or_drift(got[k][0], want[k][0], tag)
                    assert_same(got[k], want[k], tag)


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_temporal as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_accumulate_into():
    import torch
    from yart_amd import api
    for w, h in GPU_SIZES:
        for seq, dm in (("move", True), ("subpixel", False)):
            host, dev = api.TemporalAccumulator(w, h, device=0, **PARAMS), api.TemporalAccumulator(w, h, device=0, **PARAMS)
            side = torch.cuda.Stream()
            for k, fr in enumerate(frames_of(w, h, seq)):
                want = host.accumulate(fr["camera"], fr["rgba"], fr["variance"], aovs_of(fr, dm), demodulate=dm)
                t = {name: torch.from_numpy(fr[name].copy()).cuda() for name in fr if name != "camera"}
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    if k == 1:                           # in place, nothing optional
                        out, var = t["rgba"], t["variance"]
                        dev.accumulate_into(out, var, None, fr["camera"], out, var, aovs_of(t, dm), demodulate=dm)
                        got = (out.cpu().numpy(), var.cpu().numpy(), want[2])
                    else:
                        out, var = torch.zeros_like(t["rgba"]), torch.zeros_like(t["variance"])
                        ln = torch.zeros((h, w), dtype=torch.int32, device="cuda")
                        dev.accumulate_into(out, var, ln, fr["camera"], t["rgba"], t["variance"], aovs_of(t, dm), demodulate=dm)
                        got = (out.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy().view(np.uint32))
                        for name in t:
                            assert np.array_equal(bits(t[name].cpu().numpy()), bits(fr[name])), name + " was written"
                assert_same(got, want, f"accumulate_into {w}x{h} {seq} frame {k}")
            host.close()
            dev.close()


@pytest.mark.gpu
def test_accumulate_into_equals_the_host_form(gpu_api):
    """api.TemporalAccumulator.accumulate_into on torch tensors, on a non-default stream, at every size: the bits of accumulate
    (itself held to the NumPy statement above); inputs untouched when out != in; in place, and without the optional outputs, too."""
    run_torch_child("child_accumulate_into()")


def child_render_denoised():
    from yart_amd import api
    base = dict(load_params(os.path.join(GOLDEN, "cornell.txt")), size=(96, 96), spp=4)
    scene = api.DeviceScene(os.path.join(GOLDEN, "cornell.yscn"), device=0)
    acc, hand = api.TemporalAccumulator(96, 96, device=0), api.TemporalAccumulator(96, 96, device=0)
    names = ("albedo", "normal", "depth", "position", "coverage", "ids")
    grown = False
    for eye in orbit_eyes(base, frames=3):
        p = dict(base, eye=eye)
        noisy, clean, guides = scene.render_denoised(p, temporal=acc)
        frame, aovs, moms, _ = scene.render_moments(p, ("variance",), names)
        assert np.array_equal(bits(noisy.cpu().numpy()), bits(frame)), "noisy frame"
        for k in names:
            assert np.array_equal(bits(guides[k].cpu().numpy()), bits(aovs[k])), k
        a, av, ln = hand.accumulate(p, frame, moms["variance"], aovs, demodulate=True)
        assert np.array_equal(bits(guides["accumulated"].cpu().numpy()), bits(a)), "accumulated frame"
        assert np.array_equal(bits(guides["accumulated_variance"].cpu().numpy()), bits(av)), "accumulated variance"
        assert np.array_equal(bits(guides["length"].cpu().numpy()), bits(ln)), "length"
        want = api.denoise_var(a, av, aovs["albedo"], aovs["normal"], aovs["depth"], demodulate=True)
        assert np.array_equal(bits(clean.cpu().numpy()), bits(want)), "denoised frame"
        grown = grown or bool((ln > 1).mean() > 0.5)
        # without `temporal`: today's result
        noisy0, clean0, guides0 = scene.render_denoised(p, variance_guided=True)
        assert set(guides0) == {"albedo", "normal", "depth", "variance"}
        want0 = api.denoise_var(frame, moms["variance"], aovs["albedo"], aovs["normal"], aovs["depth"], demodulate=True)
        assert np.array_equal(bits(clean0.cpu().numpy()), bits(want0)), "variance-guided frame without temporal"
        noisy1, clean1, guides1 = scene.render_denoised(p)
        assert set(guides1) == {"albedo", "normal", "depth"}
        want1 = api.denoise(frame, aovs["albedo"], aovs["normal"], aovs["depth"], demodulate=True)
        assert np.array_equal(bits(clean1.cpu().numpy()), bits(want1)), "plain denoised frame without temporal"
    assert grown, "the orbit never reused a history"
    scene.close()


@pytest.mark.gpu
def test_render_denoised_temporal(gpu_api):
    """DeviceScene.render_denoised(temporal=acc) on cornell.yscn at 96 x 96 and 4 spp, three frames of a small orbit: every step ==
    render_moments, accumulate and denoise_var called by hand, bit for bit; without `temporal` it is what it was."""
    run_torch_child("child_render_denoised()")
