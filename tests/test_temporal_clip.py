"""The clip of the temporal accumulator's history to the frame's neighbourhood (include/yart_hip.h: yart_hip_temporal_set_clip,
YartTemporalClip; CLIP in the header comment of yart_hip_temporal_accumulate_device): variance clipping against the ghosting a
change of the lighting leaves behind, which no geometric tap test sees.

yart_amd/temporal.py `temporal_reference` / `temporal_moments_reference` with `clip=` state the definition in NumPy float32 and
are the reference of every comparison here, on bits: csrc/temporal.hpp compiled for the host (tests/temporalclipsim) and the
device kernels k_tp_accumulate<., ., ., true> through api.TemporalAccumulator(clip=) .accumulate / accumulate_into /
DeviceScene.render_denoised(temporal=). Scenes, cameras and frames are those of tests/test_temporal.py, test_temporal_moments.py
(`long`, `noise_frames`) and test_temporal_motion.py (`mixed`, for the two motions). Beyond reproducibility: hand-worked pixels,
the ghost of a stepped colour on iid noise, and the defaults on the cornell orbit with and without a change of the lighting."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_temporal as tt
from tests import test_temporal_moments as tm
from tests import test_temporal_motion as tmo
from tests.conftest import GOLDEN, ROOT, bit_identical_or_drift
from tests.paramfile import load_params

bits, assert_same = tt.bits, tt.assert_same
CPU_SIZES, GPU_SIZES, SEQUENCES = tt.CPU_SIZES, tt.GPU_SIZES, tt.SEQUENCES
CLIPS = [(1, 1.0), (3, 2.0)]                            # the smallest window, and the largest (on 5 x 3: larger than the image)
GHOST_CLIPS = [(1, 1.0), (1, 2.0), (2, 1.0), (2, 2.0), (3, 1.0), (3, 1.5), (3, 2.0), (3, 3.0)]
GHOST_FRAMES, GHOST_STEP_AT, GHOST_FACTOR = 10, 6, 0.25  # the colour is a quarter from frame 7 (index 6) on
DIM_FROM, DIM_FACTOR = 4, 0.25                          # the orbit's lighting change: its frames 4 and 5

_reference = {}


# ---------------------------------------------------------------------------------------------------------------------
# the sequences and the NumPy statement over them
# ---------------------------------------------------------------------------------------------------------------------
def sequences_of(moments):
    return SEQUENCES + (["long"] if moments else [])


def params_of(seq, moments):
    return dict(tm.params_of(seq)) if moments else dict(tt.PARAMS)


def statement(hist, f, demodulate, moments, prm, clip, **motion):
    from yart_amd.temporal import temporal_moments_reference, temporal_reference
    fn = temporal_moments_reference if moments else temporal_reference
    r = fn(hist, f["camera"], f["rgba"], f["variance"], f["position"], f["normal"], f["depth"], f["coverage"], f["ids"],
           f["albedo"] if demodulate else None, demodulate=demodulate, clip=clip, **motion, **prm)
    for v in r:
        v.setflags(write=False)
    return r


def reference(w, h, seq, demodulate, moments, clip):
    """the NumPy statement over a sequence of test_temporal (or `long`) -> ([(frame, variance, length)], [history colour]) per
    frame, computed once"""
    from yart_amd.temporal import TemporalHistory
    key = (w, h, seq, demodulate, moments, clip)
    if key not in _reference:
        hist = TemporalHistory(w, h)
        res, colour = [], []
        for k, f in enumerate(tm.frames_of(w, h, seq)):
            if seq == "reset" and k == 2:
                hist.reset()
            res.append(statement(hist, f, demodulate, moments, params_of(seq, moments), clip))
            colour.append(hist.colour.copy())
        _reference[key] = (res, colour)
    return _reference[key]


def pixel_records(fr):
    """the per-pixel records that say what frame `fr`'s per-node motion says (test_temporal_motion's frames): P' = M P and
    n' = Nm n in the statement's own float32 operations, kind 1 on the pixels of a moving node"""
    from yart_amd import temporal as T
    if fr["motion"] is None:
        return None
    f = np.float32
    rec = T.motion_records(fr["motion"])
    node = np.ascontiguousarray(fr["ids"][..., 0]).view(np.uint32)
    in_range = node < np.uint32(len(rec))
    r = rec[np.where(in_range, node, np.uint32(0))]
    moving = in_range & (r[..., T.MOTION_KIND_WORD].view(np.uint32) == 1)
    with np.errstate(all="ignore"):
        pm = np.stack([T._dot(r[..., 4 * i:4 * i + 3], fr["position"]) + r[..., 4 * i + 3] for i in range(3)], -1).astype(f)
        nm = np.stack([T._dot(r[..., 12 + 4 * i:15 + 4 * i], fr["normal"]) for i in range(3)], -1).astype(f)
    out = np.zeros(node.shape + (8,), f)
    out[..., 0:3] = np.where(moving[..., None], pm, 0)
    out[..., 4:7] = np.where(moving[..., None], nm, 0)
    out.view(np.uint32)[..., 3] = moving
    return out


def motion_frames(w, h):
    """test_temporal_motion's `mixed` sequence (a moving node, a moving camera, random buffers with their non-finite entries),
    each frame with its per-node motion and the per-pixel records that say the same"""
    key = ("motion frames", w, h)
    if key not in _reference:
        _reference[key] = [dict(f, pixel_motion=pixel_records(f)) for f in tmo.frames_of(w, h, "mixed")]
    return _reference[key]


def motion_reference(w, h, demodulate, moments, clip, kind):
    """the NumPy statement over motion_frames with `kind` ("node" or "pixel") motion, computed once"""
    from yart_amd.temporal import TemporalHistory
    key = ("motion", w, h, demodulate, moments, clip, kind)
    if key not in _reference:
        hist = TemporalHistory(w, h)
        prm = tmo.params_of(moments)
        _reference[key] = [statement(hist, f, demodulate, moments, prm, clip,
                                     **({"motion": f["motion"]} if kind == "node" else {"pixel_motion": f["pixel_motion"]}))
                           for f in motion_frames(w, h)]
    return _reference[key]


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def test_set_clip_abi_and_argument_errors(built, tmp_path):
    """yart_hip_temporal_set_clip exists and is in api.EXPORTS, the ABI is still 3, YartTemporalParams is still 24 bytes and
    YartTemporalMomentParams 28, YartTemporalClip and the defaults agree between ctypes, yart_amd/temporal.py and a C++ compile of
    both headers (which also sees yart::hip::Temporal::setClip and temporalClipDefaults), and every refusal the header lists is
    YART_E_INVALID with a telling message — a handle is made without a device, and none is touched. That a refused setting keeps
    the previous one, and that the setting survives reset, shows in results only: test_device_setting_between_frames; here it is
    held on the Python surface, whose `clip` is what the references take."""
    from yart_amd import api, temporal
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    assert hasattr(raw, "yart_hip_temporal_set_clip") and "yart_hip_temporal_set_clip" in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n#include <cstddef>\n'
                "int main() { std::printf(\"%zu %zu %zu %zu %zu %u\\n\", sizeof(YartTemporalClip), offsetof(YartTemporalClip, radius),\n"
                "      offsetof(YartTemporalClip, gamma), sizeof(YartTemporalParams), sizeof(YartTemporalMomentParams),\n"
                "      YART_TEMPORAL_DEFAULT_CLIP_RADIUS);\n"
                "  std::printf(\"%.9g\\n\", YART_TEMPORAL_DEFAULT_CLIP_GAMMA);\n"
                "  yart::hip::Temporal t(4, 4);\n"
                "  void (yart::hip::Temporal::*fn)(const YartTemporalClip*) = &yart::hip::Temporal::setClip;\n"
                "  YartTemporalClip c = yart::hip::temporalClipDefaults();\n"
                "  if (c.struct_size != sizeof(c) || c.radius != YART_TEMPORAL_DEFAULT_CLIP_RADIUS || c.gamma != YART_TEMPORAL_DEFAULT_CLIP_GAMMA) return 3;\n"
                "  t.setClip(c); t.reset(); t.setClip(nullptr);\n"
                "  c.radius = 4;\n"
                "  try { t.setClip(c); return 2; } catch (const yart::hip::Error&) {}\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    T = api.TemporalClip
    assert [int(v) for v in out[:6]] == [ctypes.sizeof(T), T.radius.offset, T.gamma.offset, ctypes.sizeof(api.TemporalParams),
                                         ctypes.sizeof(api.TemporalMomentParams), temporal.DEFAULT_CLIP_RADIUS]
    assert ctypes.sizeof(T) == 12 and ctypes.sizeof(api.TemporalParams) == 24 and ctypes.sizeof(api.TemporalMomentParams) == 28
    assert np.float32(out[6]) == np.float32(temporal.DEFAULT_CLIP_GAMMA)
    assert 1 <= temporal.DEFAULT_CLIP_RADIUS <= temporal.CLIP_MAX_RADIUS == 3 and temporal.DEFAULT_CLIP_GAMMA >= 0

    h = ctypes.c_void_p()
    assert L.yart_hip_temporal_create(4, 4, 0, ctypes.byref(h)) == api.YART_OK and h.value

    def call(handle=h, radius=1, gamma=1.0, struct_size=None, null_clip=False):
        tc = T(ctypes.sizeof(T) if struct_size is None else struct_size, radius, gamma)
        return L.yart_hip_temporal_set_clip(handle, None if null_clip else ctypes.byref(tc))
    assert call() == api.YART_OK
    cases = [(dict(handle=None), b"handle"), (dict(struct_size=8), b"struct_size"), (dict(struct_size=0), b"struct_size"),
             (dict(radius=0), b"radius"), (dict(radius=4), b"radius"), (dict(radius=0xffffffff), b"radius"),
             (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"), (dict(gamma=float("-inf")), b"gamma"),
             (dict(gamma=-0.5), b"gamma"), (dict(gamma=-1e-30), b"gamma")]
    for kw, word in cases:
        assert call(**kw) == api.YART_E_INVALID, kw
        assert word in L.yart_hip_last_error(), (kw, L.yart_hip_last_error())
    # what is not refused: every radius, gamma 0 and a huge one, a larger struct_size, NULL (off), again and after a reset
    for radius in (1, 2, 3):
        assert call(radius=radius) == api.YART_OK
    assert call(gamma=0.0) == api.YART_OK and call(gamma=3e38) == api.YART_OK and call(struct_size=64) == api.YART_OK
    assert call(null_clip=True) == api.YART_OK and call(null_clip=True) == api.YART_OK
    assert call() == api.YART_OK and L.yart_hip_temporal_reset(h) == api.YART_OK and call(null_clip=True) == api.YART_OK
    L.yart_hip_temporal_destroy(h)
    # the Python surface
    acc = api.TemporalAccumulator(4, 4)
    assert acc.clip is None
    acc.set_clip(True)
    assert acc.clip == (temporal.DEFAULT_CLIP_RADIUS, temporal.DEFAULT_CLIP_GAMMA)
    acc.set_clip((3, 2.0))
    for bad, word in (((0, 1.0), "radius"), ((4, 1.0), "radius"), ((2, float("nan")), "gamma"), ((2, -1.0), "gamma")):
        with pytest.raises(api.YartError, match=word):
            acc.set_clip(bad)
        assert acc.clip == (3, 2.0)                     # a refused setting keeps the previous one
    acc.reset()
    assert acc.clip == (3, 2.0)
    acc.set_clip(None)
    assert acc.clip is None
    acc.close()
    acc = api.TemporalAccumulator(4, 4, moments=True, clip=(2, 1.5))
    assert acc.clip == (2, 1.5)
    acc.close()
    assert temporal.clip_of(None) is None and temporal.clip_of(True) == (temporal.DEFAULT_CLIP_RADIUS, temporal.DEFAULT_CLIP_GAMMA)
    for bad in ((0, 1.0), (4, 1.0), (1.5, 1.0), (1, float("inf")), (1, -1.0)):
        with pytest.raises(AssertionError):
            temporal.clip_of(bad)


def test_numpy_statement_on_hand_made_inputs():
    """temporal_reference(clip=) on 1-, 2- and 3-pixel frames whose answer is worked out by hand. The camera is static and every
    pixel projects onto itself: one tap of weight 1, N = 2, a = 1/2 in the second frame."""
    from yart_amd.temporal import TemporalHistory, camera_basis
    f = np.float32
    kw = dict(alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01)
    cam2, cam3 = tt.hand_camera(2), tt.hand_camera(3)
    k = camera_basis(cam3)                               # 3 x 1: pixels of 2 x 2 world units, centres x = -2, 0, 2
    assert k["top_left"].tolist() == [-2, 0, 0] and k["dU"].tolist() == [2, 0, 0] and k["dV"].tolist() == [0, -2, 0]
    centres = {1: [0.0], 2: [-1.5, 1.5], 3: [-2.0, 0.0, 2.0]}

    def two_frames(w, first, second, clip, albedo=None, second_albedo=None):
        """first / second: (w, 3) colours -> (the second frame's (w, 3) colours out, length, history)"""
        cam = tt.hand_camera(w)
        hist = TemporalHistory(w, 1)
        out = None
        for colours, alb in ((first, albedo), (second, second_albedo if second_albedo is not None else albedo)):
            fr = tt.hand_frame(w, 0.0, 2.0, centres[w])
            fr["rgba"][0, :, :3] = np.asarray(colours, f)
            if alb is not None:
                fr["albedo"] = np.asarray(alb, f).reshape(1, w, 3)
            out, var, ln = tt.run_hand(hist, cam, fr, clip=clip, **kw)
        return out[0, :, :3], ln[0], hist
    # 2 x 1, radius 1: both windows hold both pixels (k = 2). History h = (8, 1, 4) on both; the frame is (2, 3, 3) and (4, 5, 5):
    # mu = (3, 4, 4), e2 = (10, 17, 17), var = (1, 1, 1), sd = 1; gamma 1: lo = (2, 3, 3), hi = (4, 5, 5). h.r = 8 is clipped down to
    # 4, h.g = 1 up to 3, h.b = 4 is untouched. out = h' + (c - h') / 2: pixel 0 (3, 3, 3.5), pixel 1 (4, 4, 4.5); without the clip
    # pixel 0 is (5, 2, 3.5) and pixel 1 (6, 3, 4.5)
    hist_c, frame = [(8, 1, 4)] * 2, [(2, 3, 3), (4, 5, 5)]
    out, ln, _ = two_frames(2, hist_c, frame, (1, 1.0))
    assert out.tolist() == [[3, 3, 3.5], [4, 4, 4.5]] and ln.tolist() == [2, 2]
    out, ln, _ = two_frames(2, hist_c, frame, None)
    assert out.tolist() == [[5, 2, 3.5], [6, 3, 4.5]] and ln.tolist() == [2, 2]
    # gamma 2: lo = (1, 2, 2), hi = (5, 6, 6): h' = (5, 2, 4): pixel 0 (3.5, 2.5, 3.5); gamma 0: h' = mu = (3, 4, 4): pixel 0 (2.5, 3.5, 3.5)
    assert two_frames(2, hist_c, frame, (1, 2.0))[0][0].tolist() == [3.5, 2.5, 3.5]
    assert two_frames(2, hist_c, frame, (1, 0.0))[0][0].tolist() == [2.5, 3.5, 3.5]
    # a larger radius on the same two pixels is the same window
    assert two_frames(2, hist_c, frame, (3, 1.0))[0].tolist() == [[3, 3, 3.5], [4, 4, 4.5]]
    # k < 2: the one pixel of a 1 x 1 image is alone in its window: h stays: 8 + (4 - 8) / 2 = 6
    out, ln, _ = two_frames(1, [(8, 8, 8)], [(4, 4, 4)], (1, 1.0))
    assert out.tolist() == [[6, 6, 6]] and ln.tolist() == [2]
    # a neighbour with c.r = 3e38: c * c overflows, e2 = inf — and so does mu * mu (mu = 1.5e38): var = inf - inf is NaN, which
    # the clamp turns into 0, sd = 0: mu and sd are finite, e2 is not: the red channel is left alone (it would be clipped to
    # 1.5e38), the others are clipped as above. Pixel 1: r = 8 + (1 - 8) / 2 = 4.5
    # ... and with c.r = 2e19, where only c * c overflows (mu = 1e19): e2 = var = sd = inf: left alone as well
    out, ln, _ = two_frames(2, hist_c, [(3e38, 3, 3), (1, 5, 5)], (1, 1.0))
    assert out[1].tolist() == [4.5, 4, 4.5] and ln.tolist() == [2, 2]
    assert out[0, 1:].tolist() == [3, 3.5] and out[0, 0] == f(8) + f(0.5) * (f(3e38) - f(8))
    out, ln, _ = two_frames(2, hist_c, [(2e19, 3, 3), (1, 5, 5)], (1, 1.0))
    assert out[1].tolist() == [4.5, 4, 4.5] and ln.tolist() == [2, 2]
    # a non-finite neighbour is excluded: 3 x 1, pixel 0 has a NaN (it is not usable, and is nobody's neighbour): the windows of
    # pixels 1 and 2 hold pixels 1 and 2, the case above; were pixel 0 counted, mu.r would be NaN and h.r = 8 left alone: 5 and 6
    out, ln, _ = two_frames(3, [(8, 1, 4)] * 3, [(np.nan, 3, 3)] + frame, (1, 1.0))
    assert out[1:].tolist() == [[3, 3, 3.5], [4, 4, 4.5]] and ln.tolist() == [0, 2, 2]
    # ... and so is one whose albedo is not finite when demodulating (d = 1 there, so its c is finite): albedo 1 elsewhere
    alb = np.ones((3, 3), f)
    bad_alb = alb.copy()
    bad_alb[0, 1] = np.nan
    out, ln, _ = two_frames(3, [(8, 1, 4)] * 3, [(100, 3, 3)] + frame, (1, 1.0), albedo=alb, second_albedo=bad_alb)
    assert out[1:].tolist() == [[3, 3, 3.5], [4, 4, 4.5]] and ln.tolist() == [0, 2, 2]
    # with a finite albedo pixel 0 counts: pixel 1's window is all three, pixel 2's is pixels 1 and 2
    out, ln, _ = two_frames(3, [(8, 1, 4)] * 3, [(100, 3, 3)] + frame, (1, 1.0), albedo=alb)
    assert out[2].tolist() == [4, 4, 4.5] and out[1].tolist() != [3, 3, 3.5] and ln.tolist() == [2, 2, 2]
    # demodulated: the statistics are those of rgb / d. Albedo 0.5: c = (4, 6, 6) and (8, 10, 10), h = (16, 2, 8): mu = (6, 8, 8),
    # sd = 2: h' = (8, 6, 8); pixel 0: c' = (6, 6, 7) -> times d: (3, 3, 3.5)
    out, ln, hist = two_frames(2, hist_c, frame, (1, 1.0), albedo=np.full((2, 3), 0.5, f))
    assert out.tolist() == [[3, 3, 3.5], [4, 4, 4.5]] and hist.colour[0, 0].tolist() == [6, 6, 7]
    # a uniform region whose colour steps from A = 8 to B = 2: sd = 0, h = mu = B: the frame after the step is B exactly, where the
    # unclipped call returns A + a (B - A) = 5
    for w in (2, 3):
        out, ln, _ = two_frames(w, [(8, 8, 8)] * w, [(2, 2, 2)] * w, (1, 1.0))
        assert (out == 2).all() and (ln == 2).all()
        assert (two_frames(w, [(8, 8, 8)] * w, [(2, 2, 2)] * w, None)[0] == 5).all()
    # a pixel without a counting tap and a first frame are what they are without a clip: another node in the second frame
    cam = cam2
    for clip in (None, (1, 1.0)):
        hist = TemporalHistory(2, 1)
        first = tt.hand_frame(2, 8.0, 2.0, centres[2])
        a = tt.run_hand(hist, cam, first, clip=clip, **kw)
        assert np.array_equal(bits(a[0]), bits(first["rgba"])) and a[2].tolist() == [[1, 1]]
        second = tt.hand_frame(2, 0.0, 4.0, centres[2], node=9)
        second["rgba"][0, :, :3] = np.asarray(frame, f)
        b = tt.run_hand(hist, cam, second, clip=clip, **kw)
        assert np.array_equal(bits(b[0]), bits(second["rgba"])) and b[2].tolist() == [[1, 1]]


def test_numpy_statement_moments_on_hand_made_inputs():
    """temporal_moments_reference(clip=): the translation of the luminance moments. 2 x 1, a grey 8 in frame 1 on both pixels:
    rec3 = (8, 64, 1). Frame 2 is grey 2 and 4: y = (2, 4), mu_y = 3, sd_y = 1: h1 = 8 -> h1' = 4 and h2 = 64 + (16 - 64) = 16.
    N = 2, a = 1/2: pixel 0: m1 = 4 + (2 - 4) / 2 = 3, m2 = 16 + (4 - 16) / 2 = 10, w2 = 1/2, vt = 10 - 9 = 1, v_acc = 1 * (0.5 /
    0.5) = 1; pixel 1: m1 = 4, m2 = 16, vt = 0. Without the clip pixel 0 has m1 = 5, m2 = 34, v_acc = 9: the step read as noise."""
    from yart_amd.temporal import TemporalHistory
    f = np.float32
    cam = tt.hand_camera(2)
    kw = dict(alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01, min_moment_history=2)
    assert tm.luma(2) == 2 and tm.luma(4) == 4 and tm.luma(8) == 8

    def two_frames(greys, clip):
        hist = TemporalHistory(2, 1)
        tm.run_hand(hist, cam, tt.hand_frame(2, 8.0, 2.0, [-1.5, 1.5]), clip=clip, **kw)
        assert hist.moments[0].tolist() == [[8, 64, 1]] * 2
        out, var, ln = tm.run_hand(hist, cam, tt.hand_frame(2, np.asarray(greys, f), 4.0, [-1.5, 1.5]), clip=clip, **kw)
        assert ln.tolist() == [[2, 2]]
        return out, var, hist
    out, var, hist = two_frames((2.0, 4.0), (1, 1.0))
    assert hist.moments[0].tolist() == [[3, 10, 0.5], [4, 16, 0.5]] and var[0].tolist() == [1, 0]
    assert out[0, :, 0].tolist() == [3, 4]               # the colour: h = 8 -> 4, as the luminance
    out, var, hist = two_frames((2.0, 4.0), None)
    assert hist.moments[0].tolist() == [[5, 34, 0.5], [6, 40, 0.5]] and var[0].tolist() == [9, 4]
    # h1 is not clipped: greys 6 and 10, mu_y ~ 8, sd_y ~ 2: h1 = 8 lies inside, and h2 — every word — has the unclipped call's bits
    a, b = two_frames((6.0, 10.0), (1, 1.0)), two_frames((6.0, 10.0), None)
    assert np.array_equal(bits(a[2].moments), bits(b[2].moments)) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(bits(a[0]), bits(b[0]))


def _build_sim(path, flags=("-O2",)):
    return subprocess.run(["g++", "-std=c++17", *flags, "-ffp-contract=off", "-o", path,
                           os.path.join(ROOT, "tests", "temporalclipsim", "temporalclipsim.cpp"),
                           os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def clipsim(built, tmp_path_factory):
    """tests/temporalclipsim/temporalclipsim.cpp: csrc/temporal.hpp, both forms with a Frame (and a Motion), compiled for the host"""
    exe = str(tmp_path_factory.mktemp("temporalclipsim") / "temporalclipsim")
    r = _build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_sim(exe, tmp, frames, prm, demodulate, moments, in_place, clip, motions=None, resets=()):
    """frames: dicts as frames_of makes them; motions: per frame None, ("node", records) or ("pixel", records)"""
    from yart_amd import api
    h, w = frames[0]["rgba"].shape[:2]
    n = w * h
    motions = motions or [None] * len(frames)
    n_nodes = max([1] + [len(m[1]) for m in motions if m is not None and m[0] == "node"])
    fin, fout = os.path.join(tmp, "tc.in"), os.path.join(tmp, "tc.out")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(frames), 1 if demodulate else 0, 1 if in_place else 0, prm["max_history"],
                          prm.get("min_moment_history", 0) if moments else 0, n_nodes, clip[0] if clip else 0], np.uint32).tobytes())
        f.write(np.array([prm["alpha_min"], prm["normal_cos_min"], prm["plane_tolerance"], clip[1] if clip else 0.0], np.float32).tobytes())
        for k, (fr, m) in enumerate(zip(frames, motions)):
            f.write(np.array([1 if k in resets else 0, 0 if m is None else 1 if m[0] == "node" else 2], np.uint32).tobytes())
            f.write(bytes(api.make_camera(fr["camera"])))
            for name in ("rgba", "variance", "position", "normal", "depth", "coverage", "ids", "albedo"):
                f.write(fr[name].tobytes())
            if m is not None:
                assert m[0] == "pixel" or len(m[1]) == n_nodes
                f.write(np.ascontiguousarray(m[1], np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    words = np.fromfile(fout, np.uint32).reshape(len(frames), n * 6)
    return [(words[k, :n * 4].view(np.float32).reshape(h, w, 4), words[k, n * 4:n * 5].view(np.float32).reshape(h, w),
             words[k, n * 5:].reshape(h, w)) for k in range(len(frames))]


def motions_of(frames, kind):
    return [None if f["motion"] is None else (kind, f["motion"] if kind == "node" else f["pixel_motion"]) for f in frames]


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_equals_the_numpy_statement_on_bits(clipsim, tmp_path, w, h):
    """csrc/temporal.hpp on the host, with the Frame accessor, == the NumPy statement with clip=, bit for bit: every sequence of
    test_temporal in both forms (and `long` in the moments form), demodulation on and off, out of place and in place, at (radius 1,
    gamma 1) and (radius 3, gamma 2) — on 5 x 3 a window larger than the image —, every frame."""
    for clip in CLIPS:
        for moments in (False, True):
            for seq in sequences_of(moments):
                frames = tm.frames_of(w, h, seq)
                for dm in (False, True):
                    want = reference(w, h, seq, dm, moments, clip)[0]
                    for in_place in (False, True):
                        got = run_sim(clipsim, str(tmp_path), frames, params_of(seq, moments), dm, moments, in_place, clip,
                                      resets=(2,) if seq == "reset" else ())
                        assert len(got) == len(want)
                        for k in range(len(want)):
                            assert_same(got[k], want[k], f"{w}x{h} clip {clip} {seq} moments {moments} demodulate {dm} in_place {in_place} frame {k}")


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_with_a_motion_equals_the_numpy_statement_on_bits(clipsim, tmp_path, w, h):
    """The same with a per-node and with a per-pixel motion, on test_temporal_motion's `mixed` sequence: both forms, both
    parameter pairs, demodulated out of place and not demodulated in place. The per-pixel records say what the per-node motion
    says, so the two statements agree with each other as well."""
    frames = motion_frames(w, h)
    for clip in CLIPS:
        for moments in (False, True):
            for dm, in_place in ((True, False), (False, True)):
                by_node = motion_reference(w, h, dm, moments, clip, "node")
                by_pixel = motion_reference(w, h, dm, moments, clip, "pixel")
                for kind, want in (("node", by_node), ("pixel", by_pixel)):
                    got = run_sim(clipsim, str(tmp_path), frames, tmo.params_of(moments), dm, moments, in_place, clip,
                                  motions=motions_of(frames, kind))
                    for k in range(len(want)):
                        assert_same(got[k], want[k], f"{w}x{h} clip {clip} {kind} motion moments {moments} demodulate {dm} frame {k}")
                        assert_same(by_pixel[k], by_node[k], f"{w}x{h} the two motions, frame {k}")


def clip_classes(w, h, seq, clip, k=1):
    """Among the pixels with a history in frame k (length > 1): (raised, lowered, identical) masks — a channel of the accumulated
    colour above / below the unclipped run's, or all three channels with its bits. The history is the same in both runs up to
    frame k - 1 only for k = 1, where the clip has not yet acted on it."""
    (res, col), (res0, col0) = reference(w, h, seq, False, False, clip), reference(w, h, seq, False, False, None)
    assert np.array_equal(res[k][2], res0[k][2])
    with_history = res[k][2] > 1
    raised = with_history & (col[k] > col0[k]).any(-1)
    lowered = with_history & (col[k] < col0[k]).any(-1)
    same = with_history & (bits(col[k]) == bits(col0[k])).all(-1)
    return raised, lowered, same


@pytest.mark.parametrize("w,h", [(37, 23), (131, 67)])
def test_the_inputs_take_every_branch(w, h):
    """A condition on the inputs of the bit comparisons, on the NumPy statement: in frame 1 of static / subpixel / move at (1, 1.0),
    among the pixels with a history, at least 20 each are raised, lowered and left bit-identical by the clip; at (3, 2.0) at least
    one is changed and one unchanged; the lengths are the unclipped run's in every frame of every sequence, in both forms."""
    for seq in ("static", "subpixel", "move"):
        raised, lowered, same = clip_classes(w, h, seq, (1, 1.0))
        print(f"{w}x{h} {seq} (1, 1.0): raised {int(raised.sum())}, lowered {int(lowered.sum())}, bit-identical {int(same.sum())}")
        assert raised.sum() >= 20 and lowered.sum() >= 20 and same.sum() >= 20
        raised, lowered, same = clip_classes(w, h, seq, (3, 2.0))
        print(f"{w}x{h} {seq} (3, 2.0): changed {int((raised | lowered).sum())}, bit-identical {int(same.sum())}")
        assert (raised | lowered).sum() >= 1 and same.sum() >= 1
    for clip in CLIPS:
        for moments in (False, True):
            for seq in sequences_of(moments):
                a, b = reference(w, h, seq, True, moments, clip)[0], reference(w, h, seq, True, moments, None)[0]
                for k in range(len(a)):
                    assert np.array_equal(a[k][2], b[k][2]), (clip, moments, seq, k)


def test_no_clip_means_no_change(clipsim, tmp_path):
    """clip=None is the code from before there was a clip: the statement's results equal test_temporal's and
    test_temporal_moments' own references on bits (computed there without the argument), and so do the host statement's with a
    clip radius of 0 in its header — the entry without a Frame."""
    for w, h in CPU_SIZES:
        for seq in SEQUENCES:
            for dm in (False, True):
                for moments, want in ((False, tt.reference(w, h, seq, dm)), (True, tm.reference(w, h, seq, dm))):
                    mine = reference(w, h, seq, dm, moments, None)[0]
                    got = run_sim(clipsim, str(tmp_path), tm.frames_of(w, h, seq), params_of(seq, moments), dm, moments, False, None,
                                  resets=(2,) if seq == "reset" else ())
                    for k in range(len(want)):
                        assert_same(mine[k], want[k], f"numpy {w}x{h} {seq} moments {moments} demodulate {dm} frame {k}")
                        assert_same(got[k], want[k], f"host {w}x{h} {seq} moments {moments} demodulate {dm} frame {k}")


def ghost_rmse(sigma, clip, step):
    """RMSE against the truth of each of the 10 accumulated frames of tm.noise_frames at the defaults; with `step` the colour
    (and the truth) is a quarter from frame 7 on"""
    from yart_amd.temporal import TemporalHistory
    key = ("ghost", sigma, clip, step)
    if key not in _reference:
        hist = TemporalHistory(64, 64)
        out = []
        for k, fr in enumerate(tm.noise_frames(sigma, frames=GHOST_FRAMES)):
            truth = 1.0
            if step and k >= GHOST_STEP_AT:
                fr = dict(fr, rgba=fr["rgba"].copy())
                fr["rgba"][..., :3] *= np.float32(GHOST_FACTOR)
                truth = GHOST_FACTOR
            acc, _, _ = tt.run_hand(hist, fr["camera"], fr, clip=clip)
            out.append(float(np.sqrt(np.mean((acc[..., :3].astype(np.float64) - truth) ** 2))))
        _reference[key] = out
    return _reference[key]


@pytest.mark.parametrize("sigma", [0.1, 0.5])
def test_a_stepped_colour_does_not_ghost(sigma):
    """64 x 64, a static camera on one plane, colour 1 with iid noise of standard deviation sigma, 10 frames at the default
    parameters; from frame 7 on the colour is a quarter. For each of eight (radius, gamma): the RMSE against the new truth is lower
    with the clip than without it in each of frames 7, 8 and 9; and on the sequence without the step the clipped frame 10 is
    within sigma of the truth. This statement gives, at sigma 0.1: 0.643 / 0.563 / 0.493 without the clip, at worst (3, 3.0) 0.063 /
    0.054 / 0.047 with it; unstepped frame 10: 0.027 .. 0.032 (unclipped 0.032). At sigma 0.5: 0.665 / 0.582 / 0.509 without, at
    worst 0.311 / 0.269 / 0.235 with; unstepped 0.134 .. 0.159."""
    without = ghost_rmse(sigma, None, True)
    print(f"sigma {sigma}: unclipped frames 7 - 9: " + " / ".join(f"{v:.4f}" for v in without[GHOST_STEP_AT:GHOST_STEP_AT + 3])
          + f"; unstepped frame 10 {ghost_rmse(sigma, None, False)[-1]:.4f}")
    for clip in GHOST_CLIPS:
        with_ = ghost_rmse(sigma, clip, True)
        steady = ghost_rmse(sigma, clip, False)[-1]
        print(f"sigma {sigma} clip {clip}: frames 7 - 9: " + " / ".join(f"{v:.4f}" for v in with_[GHOST_STEP_AT:GHOST_STEP_AT + 3])
              + f"; unstepped frame 10 {steady:.4f}")
        for k in range(GHOST_STEP_AT, GHOST_STEP_AT + 3):
            assert with_[k] < without[k], (clip, k)
        assert steady < sigma, clip


def dimmed(frames):
    """the orbit with its lighting change: frames 4 and 5 with every emitter at a quarter — radiance is linear in emission, so
    rgba * 0.25 and variance * 0.0625"""
    out = []
    for k, fr in enumerate(frames):
        if k >= DIM_FROM:
            fr = dict(fr, rgba=(fr["rgba"] * np.float32([DIM_FACTOR] * 3 + [1.0])).astype(np.float32),
                      variance=(fr["variance"] * np.float32(DIM_FACTOR * DIM_FACTOR)).astype(np.float32))
        out.append(fr)
    return out


@pytest.fixture(scope="module")
def temporalsim(built, tmp_path_factory):
    """tests/temporalsim/temporalsim.cpp, for its host path tracer with feature buffers (`render`)"""
    exe = str(tmp_path_factory.mktemp("temporalsim") / "temporalsim")
    r = tt._build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_default_clip_on_the_cornell_orbit(hostsim, temporalsim, tmp_path):
    """The 6-frame orbit of cornell.yscn of test_temporal (96 x 96, 4 spp, demodulated, tests/golden/temporal/cornell_orbit_hi.f32
    as the target), RMSE over the AgX-tonemapped frames, at the default clip. Orderings only. Unchanged orbit: the clipped
    accumulation is closer to the 1024-spp frame than the last frame alone. With the lighting change (frames 4 and 5 at a quarter,
    against a quarter of the target): the clipped accumulation is closer than the unclipped one."""
    from yart_amd import temporal
    p = load_params(os.path.join(GOLDEN, "cornell.txt"))
    frames = [tt.render_orbit_frame(temporalsim, str(tmp_path), "cornell", (96, 96), tt.ORBIT_SPP, eye) for eye in tt.orbit_eyes(p)]
    hi = np.fromfile(os.path.join(GOLDEN, "temporal", "cornell_orbit_hi.f32"), np.float32).reshape(96, 96, 4)
    tmap = lambda x: tt.host_tonemap(hostsim, str(tmp_path), x)
    clip = (temporal.DEFAULT_CLIP_RADIUS, temporal.DEFAULT_CLIP_GAMMA)
    ref = tmap(hi)
    noisy = tt.rmse(tmap(frames[-1]["rgba"]), ref)
    plain, clipped = (tt.rmse(tmap(tt.accumulate_orbit(frames, clip=c)[0]), ref) for c in (None, clip))
    print(f"cornell orbit, clip {clip}: RMSE last frame {noisy:.5f}, accumulated {plain:.5f}, clipped {clipped:.5f} "
          f"(ratio to the last frame {clipped / noisy:.4f}, to unclipped {clipped / plain:.4f})")
    assert clipped < noisy
    dim = dimmed(frames)
    ref = tmap((hi * np.float32([DIM_FACTOR] * 3 + [1.0])).astype(np.float32))
    noisy = tt.rmse(tmap(dim[-1]["rgba"]), ref)
    plain, clipped = (tt.rmse(tmap(tt.accumulate_orbit(dim, clip=c)[0]), ref) for c in (None, clip))
    print(f"cornell orbit dimmed to a quarter from frame {DIM_FROM}: RMSE last frame {noisy:.5f}, accumulated {plain:.5f}, clipped "
          f"{clipped:.5f} (ratio to the last frame {clipped / noisy:.4f}, to unclipped {clipped / plain:.4f})")
    assert clipped < plain


def test_the_host_statement_under_sanitizers(built, tmp_path):
    """tests/temporalclipsim once more with -fsanitize=address,undefined, a stand-alone program: 5 x 3 (the window is larger than
    the image) and 37 x 23 at radius 3, both forms, in place and not, with a per-pixel motion: no report, and the statement's bits."""
    exe = str(tmp_path / "temporalclipsim_san")
    r = _build_sim(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert r.returncode == 0, r.stderr[-2000:]
    clip = (3, 2.0)
    for w, h in ((5, 3), (37, 23)):
        for moments in (False, True):
            want = reference(w, h, "move", True, moments, clip)[0]
            for in_place in (False, True):
                got = run_sim(exe, str(tmp_path), tt.frames_of(w, h, "move"), params_of("move", moments), True, moments, in_place, clip)
                for k in range(len(want)):
                    assert_same(got[k], want[k], f"sanitized {w}x{h} moments {moments} in_place {in_place} frame {k}")
            frames = motion_frames(w, h)
            want = motion_reference(w, h, True, moments, clip, "pixel")
            got = run_sim(exe, str(tmp_path), frames, tmo.params_of(moments), True, moments, True, clip, motions=motions_of(frames, "pixel"))
            for k in range(len(want)):
                assert_same(got[k], want[k], f"sanitized {w}x{h} pixel motion moments {moments} frame {k}")


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def device_frame(acc, fr, demodulate, in_place=False, **kw):
    frame, var = fr["rgba"].copy(), fr["variance"].copy()
    got = acc.accumulate(fr["camera"], frame, var, tt.aovs_of(fr, demodulate), demodulate=demodulate,
                         out=frame if in_place else None, out_variance=var if in_place else None, **kw)
    if not in_place:
        assert np.array_equal(bits(frame), bits(fr["rgba"])) and np.array_equal(bits(var), bits(fr["variance"]))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_accumulate_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_tp_accumulate<., false, false, true> through api.TemporalAccumulator(clip=).accumulate — the host entries, which
    accumulate in place on the device: the staging path — == the NumPy statement with clip=, bit for bit: frame, variance and
    length of every frame, every sequence, both forms, both parameter pairs, demodulation on and off, out of place and with the
    outputs aliasing the inputs. 1 x 1 and 5 x 3 are tiles smaller than the halo; 131 x 67 is several workgroups in both
    directions and no multiple of 16."""
    for clip in CLIPS:
        for moments in (False, True):
            for seq in sequences_of(moments):
                for dm in (False, True):
                    want = reference(w, h, seq, dm, moments, clip)[0]
                    for in_place in (False, True):
                        acc = gpu_api.TemporalAccumulator(w, h, device=0, moments=moments, clip=clip, **params_of(seq, moments))
                        for k, fr in enumerate(tm.frames_of(w, h, seq)):
                            if seq == "reset" and k == 2:
                                acc.reset()
                            got = device_frame(acc, fr, dm, in_place)
                            tag = f"temporal clip {clip} {w}x{h} {seq} moments {moments} demodulate {dm} in_place {in_place} frame {k}"
                            bit_identical_or_drift(got[0], want[k][0], tag)
                            assert_same(got, want[k], tag)
                        acc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_accumulate_with_a_motion_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_tp_accumulate<., true, false, true> and <., true, true, true>: the clip with a per-node and with a per-pixel motion, on
    test_temporal_motion's `mixed` sequence: both forms, both parameter pairs, demodulated out of place and not demodulated in place."""
    frames = motion_frames(w, h)
    for clip in CLIPS:
        for moments in (False, True):
            for dm, in_place in ((True, False), (False, True)):
                for kind in ("node", "pixel"):
                    want = motion_reference(w, h, dm, moments, clip, kind)
                    acc = gpu_api.TemporalAccumulator(w, h, device=0, moments=moments, clip=clip, **tmo.params_of(moments))
                    for k, fr in enumerate(frames):
                        kw = {"motion": fr["motion"]} if kind == "node" else {"pixel_motion": fr["pixel_motion"]}
                        got = device_frame(acc, fr, dm, in_place, **kw)
                        assert_same(got, want[k], f"temporal clip {clip} {w}x{h} {kind} motion moments {moments} demodulate {dm} frame {k}")
                    acc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [False, True])
def test_device_setting_between_frames(gpu_api, moments):
    """`subpixel` at 37 x 23 and 131 x 67. A handle that never had a clip, and one whose clip was set and turned off with NULL,
    give test_temporal's / test_temporal_moments' own references on bits. set_clip between frames takes effect on the next
    frame: frames 0 and 1 without, frame 2 with (1, 1.0) is the statement run the same way; a refused setting keeps the previous
    one; the setting survives reset (the frames after it equal the statement's first frames with the clip)."""
    from yart_amd.temporal import TemporalHistory
    api = gpu_api
    for w, h in ((37, 23), (131, 67)):
        seq, dm = "subpixel", True
        frames = tm.frames_of(w, h, seq)
        prm = params_of(seq, moments)
        old = (tm.reference if moments else tt.reference)(w, h, seq, dm)
        for turned_off in (False, True):
            acc = api.TemporalAccumulator(w, h, device=0, moments=moments, **prm)
            if turned_off:
                acc.set_clip((3, 2.0))
                acc.set_clip(None)
            for k, fr in enumerate(frames):
                assert_same(device_frame(acc, fr, dm, in_place=turned_off), old[k], f"{w}x{h} no clip (turned off: {turned_off}) frame {k}")
            acc.close()
        clips = [None, None, (1, 1.0)]
        hist = TemporalHistory(w, h)
        want = [statement(hist, fr, dm, moments, prm, c) for fr, c in zip(frames, clips)]
        assert (bits(want[2][0]) != bits(old[2][0])).any()
        acc = api.TemporalAccumulator(w, h, device=0, moments=moments, **prm)
        for k, fr in enumerate(frames):
            if clips[k] is not None:
                acc.set_clip(clips[k])
                with pytest.raises(api.YartError, match="radius"):
                    acc.set_clip((7, 1.0))              # refused: (1, 1.0) stays
            assert_same(device_frame(acc, fr, dm), want[k], f"{w}x{h} set between frames, frame {k}")
        acc.reset()                                     # the clip survives: the statement with the clip from its first frame
        after = reference(w, h, seq, dm, moments, (1, 1.0))[0]
        for k, fr in enumerate(frames):
            assert_same(device_frame(acc, fr, dm), after[k], f"{w}x{h} after reset, frame {k}")
        acc.close()


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_temporal_clip as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_accumulate_into():
    import torch
    from yart_amd import api
    for w, h in GPU_SIZES:
        for seq, dm, moments, clip in (("move", True, False, (1, 1.0)), ("subpixel", False, True, (3, 2.0))):
            want = reference(w, h, seq, dm, moments, clip)[0]
            dev = api.TemporalAccumulator(w, h, device=0, moments=moments, clip=clip, **params_of(seq, moments))
            side = torch.cuda.Stream()
            for k, fr in enumerate(tm.frames_of(w, h, seq)):
                t = {name: torch.from_numpy(fr[name].copy()).cuda() for name in fr if name != "camera"}
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    if k == 1:                           # in place (the staging copy runs on `side`), nothing optional
                        out, var = t["rgba"], t["variance"]
                        dev.accumulate_into(out, var, None, fr["camera"], out, var, tt.aovs_of(t, dm), demodulate=dm)
                        got = (out.cpu().numpy(), var.cpu().numpy(), want[k][2])
                    else:
                        out, var = torch.zeros_like(t["rgba"]), torch.zeros_like(t["variance"])
                        ln = torch.zeros((h, w), dtype=torch.int32, device="cuda")
                        dev.accumulate_into(out, var, ln, fr["camera"], t["rgba"], t["variance"], tt.aovs_of(t, dm), demodulate=dm)
                        got = (out.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy().view(np.uint32))
                        for name in t:
                            assert np.array_equal(bits(t[name].cpu().numpy()), bits(fr[name])), name + " was written"
                assert_same(got, want[k], f"accumulate_into clip {clip} {w}x{h} {seq} frame {k}")
            dev.close()


@pytest.mark.gpu
def test_accumulate_into_equals_the_numpy_statement_on_bits(gpu_api):
    """api.TemporalAccumulator(clip=).accumulate_into — the device entries — on torch tensors, on a non-default stream, at every
    size: the NumPy statement's bits in both forms; inputs untouched when out != in; in place — the staging copy on the call's
    stream —, and without the optional outputs, too."""
    run_torch_child("child_accumulate_into()")


def child_render_denoised():
    from yart_amd import api
    from yart_amd.temporal import TemporalHistory, temporal_reference
    base = dict(load_params(os.path.join(GOLDEN, "cornell.txt")), size=(96, 96), spp=4)
    scene = api.DeviceScene(os.path.join(GOLDEN, "cornell.yscn"), device=0)
    acc = api.TemporalAccumulator(96, 96, device=0, clip=True)
    hist, hist0 = TemporalHistory(96, 96), TemporalHistory(96, 96)
    changed = False
    for eye in tt.orbit_eyes(base, frames=3):
        p = dict(base, eye=eye)
        noisy, clean, g = scene.render_denoised(p, temporal=acc)
        buf = {name: g[name].cpu().numpy() for name in ("variance", "position", "normal", "depth", "coverage", "ids", "albedo")}
        args = (p, noisy.cpu().numpy(), buf["variance"], buf["position"], buf["normal"], buf["depth"], buf["coverage"], buf["ids"], buf["albedo"])
        want = temporal_reference(hist, *args, demodulate=True, clip=True)
        want0 = temporal_reference(hist0, *args, demodulate=True)
        dev = (g["accumulated"].cpu().numpy(), g["accumulated_variance"].cpu().numpy(), g["length"].cpu().numpy().view(np.uint32))
        assert_same(dev, want, "render_denoised with the default clip")
        want_clean = api.denoise_var(want[0], want[1], buf["albedo"], buf["normal"], buf["depth"], demodulate=True)
        assert np.array_equal(bits(clean.cpu().numpy()), bits(want_clean)), "denoised frame"
        changed = changed or bool((bits(want[0]) != bits(want0[0])).any())
    assert changed, "the clip never acted on the orbit"
    scene.close()
    acc.close()


@pytest.mark.gpu
def test_render_denoised_with_a_clip(gpu_api):
    """DeviceScene.render_denoised(temporal=TemporalAccumulator(clip=True)) on cornell.yscn at 96 x 96 and 4 spp, three frames of
    a small orbit: the accumulated frame, variance and length are the NumPy statement's with the default clip on the same
    rendered buffers, on bits (and not the unclipped statement's); the denoised frame is denoise_var of them."""
    run_torch_child("child_render_denoised()")
