"""Temporal accumulation of moving geometry: per-node motion records (include/yart_hip.h: yart_hip_temporal_set_motion,
YartTemporalMotion; PER-NODE MOTION in the header comment of yart_hip_temporal_accumulate_device).

yart_amd/temporal.py `temporal_reference` / `temporal_moments_reference` with `motion=` state the definition in NumPy float32 and
are the reference of every comparison here, on bits: csrc/temporal.hpp compiled for the host (tests/temporalmotionsim) and the
device kernels k_tp_accumulate<., true> through api.TemporalAccumulator.accumulate / accumulate_into /
DeviceScene.render_denoised(temporal=, motion=).

The inputs are an analytic scene of three nodes seen from (0, 0, 5) straight down -z. Node 0 (the root) carries the plane z = 0,
node 2 (static, under the root, fwd = translate(0, 0, 1)) the half plane z = 1, x > 0.9, and node 1 (under the root) the plane
z_obj = 0 of its own object space, placed at z = 2 and MOVING from frame to frame. In the `cut` layout node 1 is the half plane
x_obj < 0.35, so that all three nodes are seen; in the `full` layout it is the whole plane, alone, and fills the image, which is
what the conditions on what the feature is for are stated on. Four sequences of four frames:
  normal   +0.3 along the plane's normal per frame
  inplane  3 px in x and 1.11 px in y per frame within the plane (px: a pixel's edge on the plane z = 2)
  turn     40 degrees per frame (acos(0.8) = 36.9) about the plane's y axis: -60, -20, 20, 60 degrees
  mixed    inplane, and the camera of tests/test_temporal.py's `move`; frame, variance, normals, albedo and coverage are the seeded
           random buffers of test_temporal.frames_of with their non-finite entries; the motion has two records, so node 2 is out of
           its range
The other three sequences are noise-free: the colour is linear in node 1's object coordinates (in world x, y on the other nodes)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_temporal as tt
from tests.conftest import ROOT, bit_identical_or_drift
from tests.test_temporal import assert_same, bits

CPU_SIZES = [(1, 1), (5, 3), (37, 23)]
GPU_SIZES = CPU_SIZES + [(131, 67)]                     # + several workgroups in both directions, no multiple of 16
FEATURE_SIZES = [(37, 23), (131, 67)]
SEQUENCES = ["normal", "inplane", "turn", "mixed"]
FRAMES = 4
# parameters at which every branch is taken on these inputs: the length grows to the cap in frame 2 and is capped in frame 3
PARAMS = dict(alpha_min=0.2, max_history=3, normal_cos_min=0.95, plane_tolerance=0.01)
MOMENT_PARAMS = dict(PARAMS, min_moment_history=3)
DEFAULTS = {}                                           # the feature conditions: the defaults of yart_amd/temporal.py
EDGE, EDGE2, Z1, Z2 = 0.35, 0.9, 2.0, 1.0
STEP_NORMAL, STEP_PX, TURN_DEGREES = 0.3, (3.0, 1.11), (-60.0, -20.0, 20.0, 60.0)
COLOUR = np.array([[2.0, 0.5, 0.25], [1.5, 0.3, 0.6], [3.0, 0.2, 0.1]])      # per channel: c = a0 + a1 * u + a2 * v


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene, in float64
# ---------------------------------------------------------------------------------------------------------------------
def base_camera(w, h):
    return dict(size=(w, h), focal=35.0, sensor=(36.0, 24.0), eye=(0.0, 0.0, 5.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))


def pixel_on_plane(w, h):
    """edge of a pixel on the plane z = 2, for the base camera"""
    _, _, du, _ = tt.camera64(base_camera(w, h))
    return float(np.linalg.norm(du)) * (5.0 - Z1) / 5.0


def cameras(w, h, seq):
    cam = base_camera(w, h)
    if seq != "mixed":
        return [cam] * FRAMES
    px = float(np.linalg.norm(tt.camera64(cam)[2]))
    s = max(3.0, 0.04 * w)                              # test_temporal's `move`, slower (four frames, and node 1 is to stay in
                                                        # sight): a translation and a turn, at least 3 pixels a frame
    out = []
    for k in range(FRAMES):
        e = np.array(cam["eye"]) + k * np.array([s * px, 0.37 * s * px, 0.0])
        t = np.array(cam["target"]) + k * np.array([1.4 * s * px, 0.0, 0.0])
        out.append(dict(cam, eye=tuple(float(v) for v in e), target=tuple(float(v) for v in t)))
    return out


def nodes_of(w, h, seq, k):
    """the node list of frame k: what yart_amd.temporal.node_motion takes (yscn.Node: parent, fwd as binary32)"""
    from yart_amd.yscn import Node, trs
    if seq == "normal":
        f1 = trs(translation=(0.0, 0.0, Z1 + STEP_NORMAL * k))
    elif seq == "turn":
        f1 = trs(translation=(0.0, 0.0, Z1), axis=(0, 1, 0), angle=np.radians(TURN_DEGREES[k]))
    else:
        px = pixel_on_plane(w, h)
        f1 = trs(translation=(STEP_PX[0] * px * k, STEP_PX[1] * px * k, Z1))
    return [Node(-1, -1), Node(0, 0, *f1), Node(0, 1, *trs(translation=(0.0, 0.0, Z2)))]


def see(cam, nodes, full):
    """what every pixel centre of `cam` sees: (t, node, P, n, uv) in float64, (H, W, ...); uv: node 1's object x, y on node 1,
    world x, y elsewhere. The geometry is that of the nodes' binary32 matrices."""
    w, h = cam["size"]
    eye, tl, du, dv = tt.camera64(cam)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = tl + xs[..., None] * du + ys[..., None] * dv - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best_t = np.full((h, w), np.inf)
    node = np.full((h, w), -1)
    nrm = np.zeros((h, w, 3))
    uv = np.zeros((h, w, 2))
    with np.errstate(all="ignore"):
        for idx in ((1,) if full else (0, 1, 2)):
            m = np.asarray(nodes[idx].fwd, np.float64).reshape(4, 4)
            c, nw = m[:3, 3], m[:3, :3] @ np.array([0.0, 0.0, 1.0])
            t = ((c - eye) @ nw) / (d @ nw)
            p = eye + t[..., None] * d
            obj = (p - c) @ m[:3, :3]                   # rigid: the inverse of the linear part is its transpose
            ok = np.isfinite(t) & (t > 0) & (t < best_t)
            if idx == 1 and not full:
                ok &= obj[..., 0] < EDGE
            if idx == 2:
                ok &= obj[..., 0] > EDGE2
            best_t = np.where(ok, t, best_t)
            node = np.where(ok, idx, node)
            nrm = np.where(ok[..., None], nw, nrm)
            uv = np.where(ok[..., None], obj[..., :2] if idx == 1 else p[..., :2], uv)
    assert (node >= 0).all()
    return best_t, node, eye + best_t[..., None] * d, nrm, uv


_frames, _reference = {}, {}


def frames_of(w, h, seq, full=False):
    """The four frames of a sequence: camera, nodes, motion (None in frame 0), frame, variance and feature buffers."""
    from yart_amd.temporal import node_motion
    key = (w, h, seq, full)
    if key not in _frames:
        out, prev = [], None
        for k, cam in enumerate(cameras(w, h, seq)):
            nodes = nodes_of(w, h, seq, k)
            n = w * h
            t, node, p, nw, uv = see(cam, nodes, full)
            pos, depth = p.astype(np.float32), t.astype(np.float32)
            ids = np.stack([node, np.zeros_like(node), node + 3, node % 2], -1).astype(np.int32)
            cov = np.ones((h, w), np.float32)
            if seq == "mixed":                          # test_temporal.frames_of's buffers
                rng = np.random.RandomState(1000 * w + 10 * h + k)
                rgba = rng.uniform(0, 50, (h, w, 4)).astype(np.float32)
                rgba[..., 3] = rng.uniform(0, 1, (h, w))
                flat = rgba.reshape(n, 4)
                for i in rng.choice(n, n // 50, replace=False):
                    flat[i, rng.randint(3)] = 1e4
                nrm = (nw + rng.normal(0, 0.02, (h, w, 3))).astype(np.float32)
                alb = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
                alb[rng.rand(h, w, 3) < 0.05] = 0.0
                var = (rng.uniform(0, 40, (h, w)) * rng.uniform(0, 1, (h, w)) ** 4).astype(np.float32)
                var[rng.rand(h, w) < 0.1] = 0.0
                var[rng.rand(h, w) < 0.03] = 1e30
                cov[rng.rand(h, w) < 0.04] = 0.75
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
            else:
                rgba = np.ones((h, w, 4), np.float32)
                rgba[..., :3] = COLOUR[:, 0] + uv[..., :1] * COLOUR[:, 1] + uv[..., 1:] * COLOUR[:, 2]
                nrm = nw.astype(np.float32)
                alb = np.full((h, w, 3), 0.5, np.float32)
                var = np.zeros((h, w), np.float32)
            motion = None
            if prev is not None:
                motion = node_motion(prev, nodes)
                assert motion.view(np.uint32)[:, 15].tolist() == [0, 1, 0]
                if seq == "mixed":
                    motion = np.ascontiguousarray(motion[:2])
            prev = nodes
            out.append(dict(camera=cam, nodes=nodes, motion=motion, rgba=rgba, variance=var, position=pos, normal=nrm, depth=depth,
                            coverage=cov, ids=ids, albedo=alb))
        for f in out:
            for v in f.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _frames[key] = out
    return _frames[key]


def aovs_of(f, demodulate):
    names = ("position", "normal", "depth", "coverage", "ids") + (("albedo",) if demodulate else ())
    return {k: f[k] for k in names}


def statement(hist, f, demodulate, moments, prm, motion):
    from yart_amd.temporal import temporal_moments_reference, temporal_reference
    fn = temporal_moments_reference if moments else temporal_reference
    r = fn(hist, f["camera"], f["rgba"], f["variance"], f["position"], f["normal"], f["depth"], f["coverage"], f["ids"],
           f["albedo"] if demodulate else None, demodulate=demodulate, motion=motion, **prm)
    for v in r:
        v.setflags(write=False)
    return r


def params_of(moments, params=None):
    return dict((MOMENT_PARAMS if moments else PARAMS) if params is None else params)


def reference(w, h, seq, demodulate, moments, with_motion=True, params=None, full=False):
    """the NumPy statement over the sequence -> [(frame, variance, length)] per frame, computed once"""
    from yart_amd.temporal import TemporalHistory
    prm = params_of(moments, params)
    key = (w, h, seq, demodulate, moments, with_motion, full, tuple(sorted(prm.items())))
    if key not in _reference:
        hist = TemporalHistory(w, h)
        _reference[key] = [statement(hist, f, demodulate, moments, prm, f["motion"] if with_motion else None)
                           for f in frames_of(w, h, seq, full)]
    return _reference[key]


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def moving_record(m=None, nm=None):
    """a kind-1 record from a 3 x 4 and a 3 x 3 matrix (identity by default)"""
    rec = np.zeros(24, np.float32)
    rec[:12] = np.asarray(np.eye(4)[:3] if m is None else m, np.float32).reshape(12)
    rec[12:].reshape(3, 4)[:, :3] = np.eye(3) if nm is None else nm
    rec.view(np.uint32)[15] = 1
    return rec


def test_set_motion_abi_and_argument_errors(built, tmp_path):
    """yart_hip_temporal_set_motion exists and is in api.EXPORTS, the ABI is still 3, YartTemporalMotion has the same size in ctypes
    and for a C++ compiler (which also sees yart::hip::Temporal::setMotion), and every refusal the header lists is YART_E_INVALID
    with a telling message — a handle is made without a device, and none is touched."""
    from yart_amd import api, temporal
    L = api.lib()
    raw = ctypes.CDLL(api.LIB_PATH)
    assert hasattr(raw, "yart_hip_temporal_set_motion") and "yart_hip_temporal_set_motion" in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    src = os.path.join(tmp_path, "m.cpp")
    with open(src, "w") as f:
        f.write('#include "yart_hip.hpp"\n#include <cstdio>\n'
                "int main() { std::printf(\"%zu %zu\\n\", sizeof(YartTemporalMotion), sizeof(YartTemporalParams));\n"
                "  yart::hip::Temporal t(4, 4);\n"
                "  void (yart::hip::Temporal::*fn)(const std::vector<float>&) = &yart::hip::Temporal::setMotion;\n"
                "  std::vector<float> rec(48, 0.0f);\n"
                "  t.setMotion(rec); t.setMotion({});\n"
                "  try { t.setMotion(std::vector<float>(25, 0.0f)); return 2; } catch (const yart::hip::Error&) {}\n"
                "  return fn ? 0 : 1; }\n")
    exe = os.path.join(tmp_path, "m")
    lib_dir = os.path.join(ROOT, "yart_amd")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib_dir, "-lyart_hip",
                    "-Wl,-rpath," + lib_dir, "-lpthread"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(api.TemporalMotion), ctypes.sizeof(api.TemporalParams)]
    assert ctypes.sizeof(api.TemporalMotion) == 8 + ctypes.sizeof(ctypes.c_void_p) and ctypes.sizeof(api.TemporalParams) == 24
    assert (temporal.MOTION_WORDS, temporal.MOTION_KIND_WORD, temporal.MOTION_MAX_NODES) == (24, 15, 1 << 20)

    h = ctypes.c_void_p()
    assert L.yart_hip_temporal_create(4, 4, 0, ctypes.byref(h)) == api.YART_OK and h.value
    good = np.stack([np.zeros(24, np.float32), moving_record()])

    def call(handle=h, rec=good, n_nodes=None, struct_size=None, null_records=False, null_motion=False):
        rec = np.ascontiguousarray(rec, np.float32)
        tm = api.TemporalMotion(ctypes.sizeof(api.TemporalMotion) if struct_size is None else struct_size,
                                rec.size // 24 if n_nodes is None else n_nodes, None if null_records else rec.ctypes.data_as(ctypes.c_void_p))
        return L.yart_hip_temporal_set_motion(handle, None if null_motion else ctypes.byref(tm))

    def with_word(i, value, kind=1):
        rec = good.copy()
        rec[1, i] = value
        rec.view(np.uint32)[1, 15] = kind
        return rec
    kind2, kind_huge = good.copy(), good.copy()
    kind2.view(np.uint32)[0, 15] = 2
    kind_huge.view(np.uint32)[1, 15] = 0x3f800000       # 1.0f is not the integer 1
    cases = [(dict(handle=None), b"handle"), (dict(struct_size=8), b"struct_size"), (dict(struct_size=0), b"struct_size"),
             (dict(n_nodes=0), b"n_nodes"), (dict(n_nodes=1 << 20), b"n_nodes"), (dict(n_nodes=0xffffffff), b"n_nodes"),
             (dict(null_records=True), b"records"), (dict(rec=kind2), b"kind"), (dict(rec=kind_huge), b"kind")]
    cases += [(dict(rec=with_word(i, v)), b"finite") for i in (0, 3, 11, 12, 14, 16, 19, 23) for v in (np.nan, np.inf, -np.inf)]
    for kw, word in cases:
        assert call(**kw) == api.YART_E_INVALID, kw
        assert word in L.yart_hip_last_error(), (kw, L.yart_hip_last_error())
    # what is not refused: a non-finite word of a static record, the largest n_nodes, a larger struct_size, NULL (clear)
    assert call(rec=with_word(5, np.nan, kind=0)) == api.YART_OK
    assert call(rec=np.zeros(((1 << 20) - 1, 24), np.float32)) == api.YART_OK
    assert call(struct_size=64) == api.YART_OK
    assert call(null_motion=True) == api.YART_OK and call(null_motion=True) == api.YART_OK
    assert call() == api.YART_OK and L.yart_hip_temporal_reset(h) == api.YART_OK
    L.yart_hip_temporal_destroy(h)
    # the Python surface
    acc = api.TemporalAccumulator(4, 4)
    acc.set_motion(good)
    acc.set_motion(None)
    with pytest.raises(api.YartError, match="kind"):
        acc.set_motion(kind2)
    with pytest.raises(AssertionError):
        acc.set_motion(good.astype(np.float64))
    acc.close()
    with pytest.raises(AssertionError, match="kind"):
        temporal.motion_records(kind2)
    with pytest.raises(AssertionError, match="finite"):
        temporal.motion_records(with_word(3, np.nan))


def test_numpy_statement_on_hand_worked_pixels():
    """temporal_reference(motion=) on test_temporal's 1- and 2-pixel frames: P', n' and the tap decisions are worked out here."""
    from yart_amd.temporal import TemporalHistory
    f = np.float32
    cam = tt.hand_camera(1)                             # one pixel of 4 x 4 world units whose centre is the origin, eye (0, 0, 5)
    kw = dict(alpha_min=0.0, max_history=8, normal_cos_min=0.9, plane_tolerance=0.01)

    def second(motion, first_over=None, x=0.0, **over):
        """frame 1: colour 8, variance 2, node 7 at the origin; frame 2: colour 4, variance 4 -> (colour, variance, length), history"""
        hist = TemporalHistory(1, 1)
        tt.run_hand(hist, cam, tt.hand_frame(1, 8.0, 2.0, [0.0], **(first_over or {})), **kw)
        out, var, ln = tt.run_hand(hist, cam, tt.hand_frame(1, 4.0, 4.0, [x], **over), motion=motion, **kw)
        return (out[0, 0, 0], var[0, 0], ln[0, 0]), hist
    blended, fresh = (6, 1.5, 2), (4, 4, 1)             # test_temporal: the tap counts (8 + (4 - 8) / 2, 4 / 4 + 2 / 4) or not

    def motion_for(node, rec, n_nodes=8):
        m = np.zeros((n_nodes, 24), f)
        m[node] = rec
        return m
    # the plane moved +1 along its normal: P = (0, 0, 1), depth 4. Without a motion 1 > 0.01 * 4; with M = translate(0, 0, -1):
    # P' = (0, 0, 0), which projects to (0, 0), and dot(n', P_hist - P') = 0
    up = np.eye(4)[:3].copy()
    up[2, 3] = -1.0
    assert (np.array(up, np.float64) @ [0, 0, 1, 1]).tolist() == [0, 0, 0]
    assert second(None, z=1.0)[0] == fresh
    got, hist = second(motion_for(7, moving_record(up)), z=1.0)
    assert got == blended
    assert hist.position[0, 0].tolist() == [0, 0, 1] and hist.normal[0, 0].tolist() == [0, 0, 1]      # the CURRENT values
    # not moving: the node's record is static (its other words may be anything), or the node has no record
    static = moving_record(up)
    static[:12] = np.nan
    static.view(np.uint32)[15] = 0
    assert second(motion_for(7, static), z=1.0)[0] == fresh
    assert second(motion_for(6, moving_record(up)), z=1.0)[0] == fresh                   # another node's record
    assert second(motion_for(6, moving_record(up), n_nodes=7), z=1.0)[0] == fresh        # ids[0] = 7 is not below n_nodes = 7
    assert second(motion_for(0, moving_record(up)), z=1.0, node=-1, first_over=dict(node=-1))[0] == fresh   # uint32(-1) is not either
    assert second(motion_for(7, moving_record(up), n_nodes=8), z=1.0)[0] == blended
    # a static pixel is untouched even where a multiplication by the identity would not be: P.x = -0.0 stays in the record
    got, hist = second(motion_for(6, moving_record()), x=-0.0)
    assert got == blended and bits(hist.position)[0, 0, 0] == 0x80000000
    got, hist = second(motion_for(7, moving_record()), x=-0.0)           # (moving by the identity: P' = +0, and the record keeps P)
    assert got == blended and bits(hist.position)[0, 0, 0] == 0x80000000
    # the object turned: n = (1, 0, 0) now; Nm takes x to z: n' = (0, 0, 1): 1 >= 0.9, and dot(n', P_hist - P') = 0.
    # Without the motion dot(n, n_hist) = 0 < 0.9
    turn = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    assert (turn @ [1.0, 0.0, 0.0]).tolist() == [0, 0, 1]
    assert second(None, normal=(1.0, 0.0, 0.0))[0] == fresh
    assert second(motion_for(7, moving_record(nm=turn)), normal=(1.0, 0.0, 0.0))[0] == blended
    # ... and n' is what the plane test uses: with M = translate(0, 0, -1) as well, and the point at (0, 0, 1)
    assert second(motion_for(7, moving_record(up, turn)), normal=(1.0, 0.0, 0.0), z=1.0)[0] == blended
    # n' = 0.5 * n: 0.5 < 0.9 fails the normal test; P' off the history's plane by 0.5 > 0.01 * 5 fails the plane test
    assert second(motion_for(7, moving_record(nm=0.5 * np.eye(3))))[0] == fresh
    off = np.eye(4)[:3].copy()
    off[2, 3] = 0.5
    assert second(motion_for(7, moving_record(off)))[0] == fresh
    off[2, 3] = 0.03125                                  # 0.03125 <= 0.01 * 5
    assert second(motion_for(7, moving_record(off)))[0] == blended
    # P' overflows: 3e38 * 16 = inf: not reprojectable; so does n'
    big = np.eye(4)[:3].copy()
    big[0, 0] = 3e38
    assert second(motion_for(7, moving_record(big)), x=0.0)[0] == blended                # 3e38 * 0 = 0
    hist = TemporalHistory(1, 1)
    tt.run_hand(hist, cam, tt.hand_frame(1, 8.0, 2.0, [0.0]), **kw)
    wide = tt.hand_frame(1, 4.0, 4.0, [16.0])
    out, var, ln = tt.run_hand(hist, cam, wide, motion=motion_for(7, moving_record(big)), **kw)
    assert (out[0, 0, 0], var[0, 0], ln[0, 0]) == fresh
    back = np.eye(4)[:3].copy()
    back[0, 3] = -16.0                                   # the control: translate(-16, 0, 0) brings that point to the origin
    hist = TemporalHistory(1, 1)
    tt.run_hand(hist, cam, tt.hand_frame(1, 8.0, 2.0, [0.0]), **kw)
    out, var, ln = tt.run_hand(hist, cam, wide, motion=motion_for(7, moving_record(back)), **kw)
    assert (out[0, 0, 0], var[0, 0], ln[0, 0]) == blended
    assert second(motion_for(7, moving_record(nm=3e38 * np.eye(3))), normal=(0.0, 0.5, 4.0))[0] == fresh     # 3e38 * 4 = inf
    # sliding within the plane, two pixels of 3 x 3 with centres x = -1.5 and 1.5; colours 8 and 24 in frame 1. The object moved
    # +3 in x: M = translate(-3, 0, 0). Pixel 1: P' = (-1.5, 0, 0) -> jx = 0: tap 0 at weight 1 (tap 1 at weight 0 does not
    # count): h = 8, out = 8 + (4 - 8) / 2 = 6. Without the motion it takes pixel 1's own history: h = 24, out = 14 — the ghost.
    # Pixel 0: P' = (-4.5, 0, 0) -> jx = -1: tap -1 is outside and tap 0 has weight 0: a new history
    cam2 = tt.hand_camera(2)
    slide = np.eye(4)[:3].copy()
    slide[0, 3] = -3.0
    for motion, want in ((None, [(6, 1.5, 2), (14, 2.5, 2)]), (motion_for(7, moving_record(slide)), [fresh, (6, 1.5, 2)])):
        hist = TemporalHistory(2, 1)
        first = tt.hand_frame(2, 8.0, 2.0, [-1.5, 1.5])
        first["rgba"][0, 1, :3], first["variance"][0, 1] = 24.0, 6.0
        tt.run_hand(hist, cam2, first, **kw)
        out, var, ln = tt.run_hand(hist, cam2, tt.hand_frame(2, 4.0, 4.0, [-1.5, 1.5]), motion=motion, **kw)
        assert [(out[0, x, 0], var[0, x], ln[0, x]) for x in (0, 1)] == want        # v: 4 / 4 + 2 / 4, 4 / 4 + 6 / 4


def _build_sim(path):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", path,
                           os.path.join(ROOT, "tests", "temporalmotionsim", "temporalmotionsim.cpp"),
                           os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def motionsim(built, tmp_path_factory):
    """tests/temporalmotionsim/temporalmotionsim.cpp: csrc/temporal.hpp, both forms with a Motion, compiled for the host"""
    exe = str(tmp_path_factory.mktemp("temporalmotionsim") / "temporalmotionsim")
    r = _build_sim(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_sim(exe, tmp, frames, motions, demodulate, moments, in_place, params=None, resets=()):
    """frames: dicts as frames_of makes them; motions: per frame None or the records, all of one n_nodes"""
    from yart_amd import api
    prm = params_of(moments, params)
    h, w = frames[0]["rgba"].shape[:2]
    n = w * h
    n_nodes = max([1] + [len(m) for m in motions if m is not None])
    fin, fout = os.path.join(tmp, "tm.in"), os.path.join(tmp, "tm.out")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(frames), 1 if demodulate else 0, 1 if in_place else 0, prm["max_history"],
                          prm.get("min_moment_history", 0), n_nodes], np.uint32).tobytes())
        f.write(np.array([prm["alpha_min"], prm["normal_cos_min"], prm["plane_tolerance"]], np.float32).tobytes())
        for k, (fr, m) in enumerate(zip(frames, motions)):
            assert m is None or len(m) == n_nodes
            f.write(np.array([1 if k in resets else 0, 0 if m is None else 1], np.uint32).tobytes())
            f.write(bytes(api.make_camera(fr["camera"])))
            for name in ("rgba", "variance", "position", "normal", "depth", "coverage", "ids", "albedo"):
                f.write(fr[name].tobytes())
            if m is not None:
                f.write(np.ascontiguousarray(m, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    words = np.fromfile(fout, np.uint32).reshape(len(frames), n * 6)
    return [(words[k, :n * 4].view(np.float32).reshape(h, w, 4), words[k, n * 4:n * 5].view(np.float32).reshape(h, w),
             words[k, n * 5:].reshape(h, w)) for k in range(len(frames))]


@pytest.mark.parametrize("w,h", CPU_SIZES)
def test_host_statement_equals_the_numpy_statement_on_bits(motionsim, tmp_path, w, h):
    """csrc/temporal.hpp on the host, with the motion accessor, == the NumPy statement with motion=, bit for bit: all four sequences,
    both forms, demodulation on and off, out of place and in place, every frame."""
    for seq in SEQUENCES:
        frames = frames_of(w, h, seq)
        for moments in (False, True):
            for dm in (False, True):
                want = reference(w, h, seq, dm, moments)
                for in_place in (False, True):
                    got = run_sim(motionsim, str(tmp_path), frames, [f["motion"] for f in frames], dm, moments, in_place)
                    for k in range(FRAMES):
                        assert_same(got[k], want[k], f"{w}x{h} {seq} moments {moments} demodulate {dm} in_place {in_place} frame {k}")


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_the_inputs_need_the_motion(w, h):
    """A condition on the inputs of the bit comparisons, on the NumPy statement at their parameters: in every sequence the last
    frame with the motion differs from the one without it, all three nodes are seen, and with the motion at least a tenth of node
    1's pixels reach the cap while some (none in `normal`) start anew."""
    for seq in SEQUENCES:
        fr = frames_of(w, h, seq)
        assert {0, 1, 2} <= set(np.unique(fr[0]["ids"][..., 0]).tolist()), seq
        for moments in (False, True):
            a, b = reference(w, h, seq, False, moments)[-1], reference(w, h, seq, False, moments, with_motion=False)[-1]
            assert (bits(a[0]) != bits(b[0])).any() and (a[2] != b[2]).any(), (seq, moments)
            on_one = fr[-1]["ids"][..., 0] == 1
            assert (a[2][on_one] == PARAMS["max_history"]).sum() >= 0.1 * on_one.sum() >= 1, (seq, moments)
            assert seq == "normal" or (a[2][on_one] == 1).any(), (seq, moments)     # (`normal`: every pixel keeps its history)


@pytest.mark.parametrize("moments", [False, True])
def test_nothing_changes_for_static_pixels(motionsim, tmp_path, moments):
    """test_temporal.py's own inputs (frames_of; node ids > 500000 there), every sequence of its: a motion whose records are all
    kind 0 (their other words arbitrary, NaN among them) and a 3-record motion of moving records, for which every id is out of
    range, give the bits of motion=None in both forms — the NumPy statement against its own result without a motion, and the host
    statement against that; a frame without a motion (what a call after a cleared motion is) goes through the entry that takes
    none. The device's side of this, yart_hip_temporal_set_motion(NULL) included, is test_device_static_pixels_and_a_cleared_motion."""
    from yart_amd.temporal import TemporalHistory
    rng = np.random.RandomState(5)
    all_static = rng.normal(0, 3, (5, 24)).astype(np.float32)
    all_static[1, :4] = np.nan
    all_static.view(np.uint32)[:, 15] = 0
    out_of_range = np.stack([moving_record(rng.normal(0, 1, (3, 4)), rng.normal(0, 1, (3, 3))) for _ in range(3)])
    prm = params_of(moments, dict(tt.PARAMS, **({"min_moment_history": 2} if moments else {})))
    w, h = 37, 23
    for seq in ("subpixel", "move"):
        frames = [dict(f, motion=None) for f in tt.frames_of(w, h, seq)]
        assert min(int(f["ids"][..., 0].view(np.uint32).min()) for f in frames) >= 500000       # far beyond both motions' records
        for dm in (False, True):
            hist = TemporalHistory(w, h)
            want = [statement(hist, f, dm, moments, prm, None) for f in frames]
            assert (want[-1][2] > 1).mean() > 0.1
            for motion in (all_static, out_of_range):
                hist = TemporalHistory(w, h)
                for k, f in enumerate(frames):
                    assert_same(statement(hist, f, dm, moments, prm, motion), want[k], f"numpy {seq} demodulate {dm} frame {k}")
                for motions in ([motion] * 3, [motion, None, motion]):
                    got = run_sim(motionsim, str(tmp_path), frames, motions, dm, moments, False, params=prm)
                    for k in range(len(frames)):
                        assert_same(got[k], want[k], f"host {seq} demodulate {dm} frame {k}")


def feature(w, h, seq, with_motion):
    """the last frame of a `full` sequence (node 1 fills the image) at the default parameters, plain form: (frame, variance, length)"""
    return reference(w, h, seq, False, False, with_motion=with_motion, params=DEFAULTS, full=True)[FRAMES - 1]


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_a_plane_moving_along_its_normal_keeps_its_history(w, h):
    """`normal`, default parameters, frame 3: without the motion every pixel has length 1 (the plane test rejects every tap: 0.3 >
    0.01 * depth), with it every pixel has length 4. This statement gives 851 / 851 and 8777 / 8777 pixels, both ways."""
    assert (frames_of(w, h, "normal", True)[FRAMES - 1]["ids"][..., 0] == 1).all()
    without, with_ = feature(w, h, "normal", False)[2], feature(w, h, "normal", True)[2]
    print(f"normal {w}x{h}: length 1 without the motion at {(without == 1).sum()} / {w * h}, length 4 with it at {(with_ == 4).sum()} / {w * h}")
    assert (without == 1).all()
    assert (with_ == 4).all()


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_a_plane_sliding_in_itself_does_not_ghost(w, h):
    """`inplane`, default parameters, frame 3, the pixels at least 14 px from the left border and 8 px from the bottom one (the
    history front comes in from there at 3 and 1.11 px a frame): length 4 with and without the motion. With it |acc - c| <= 1e-5 *
    max|c| per channel — bilinear taps reproduce an affine pattern up to rounding; without it the history is another point's and the
    error exceeds 1e-3 * max|c| at every such pixel, in every channel.
    This statement gives, relative to max|c|: with the motion at most 1.5e-7 (37 x 23) and 2.1e-7 (131 x 67); without it at least
    2.8e-2 and 7.5e-3 (the smallest channel's smallest error; at most 6.9e-2 and 1.9e-2)."""
    fr = frames_of(w, h, "inplane", True)[FRAMES - 1]
    c = fr["rgba"][..., :3].astype(np.float64)
    checked = np.zeros((h, w), bool)
    checked[:h - 8, 14:] = True
    top = np.abs(c).max()
    for with_motion in (False, True):
        acc, _, length = feature(w, h, "inplane", with_motion)
        assert (length[checked] == 4).all(), with_motion
        err = np.abs(acc[..., :3].astype(np.float64) - c)[checked] / top
        print(f"inplane {w}x{h} motion {with_motion}: relative error {err.min():.3e} .. {err.max():.3e} over {int(checked.sum())} pixels")
        if with_motion:
            assert (err <= 1e-5).all(), err.max()
        else:
            assert (err > 1e-3).all(), err.min()


@pytest.mark.parametrize("w,h", FEATURE_SIZES)
def test_a_turning_plane_keeps_its_history(w, h):
    """`turn`, default parameters, frame 3: 40 degrees a frame is more than acos(normal_cos_min) = 36.9: without the motion no pixel of
    node 1 has a history, with it some have."""
    assert (frames_of(w, h, "turn", True)[FRAMES - 1]["ids"][..., 0] == 1).all()
    without, with_ = feature(w, h, "turn", False)[2], feature(w, h, "turn", True)[2]
    print(f"turn {w}x{h}: length > 1 without the motion at {(without > 1).sum()}, with it at {(with_ > 1).sum()} of {w * h} pixels")
    assert (without == 1).all()
    assert (with_ > 1).any()


def test_node_motion():
    """node_motion on random rigid chains of depth 3: M takes a point of this frame's world space to where the float64 chains put
    it in the previous frame's, within 1e-5 relative; Nm is M's linear part within 1e-5; a moved parent marks its children kind 1,
    untouched chains are kind 0 with all-zero records; the chain is W_parent * fwd (csrc/traverse.hpp objectRay applies the inv
    matrices root first)."""
    from yart_amd.temporal import node_motion
    from yart_amd.yscn import Node, trs
    rng = np.random.RandomState(11)

    def rigid():
        return trs(tuple(rng.uniform(-2, 2, 3)), tuple(rng.normal(0, 1, 3)), float(rng.uniform(-3, 3)))

    def world(nodes, k):
        m = np.eye(4)
        while k >= 0:
            m = np.asarray(nodes[k].fwd, np.float64) @ m
            k = nodes[k].parent
        return m
    for moved in (1, 2, 3):
        # 0 root; 1 - 2 - 3 a chain under it; 4 - 5 another; 6 under the root
        prev = [Node(-1, -1)] + [Node(p, 0, *rigid()) for p in (0, 1, 2, 0, 4, 0)]
        cur = [Node(n.parent, n.mesh, n.fwd.copy(), n.inv.copy()) for n in prev]
        cur[moved] = Node(prev[moved].parent, 0, *rigid())
        rec = node_motion(prev, cur)
        assert rec.shape == (7, 24) and rec.dtype == np.float32
        kind = rec.view(np.uint32)[:, 15]
        assert kind.tolist() == [0] + [1 if k >= moved else 0 for k in (1, 2, 3)] + [0, 0, 0]
        assert not rec[kind == 0].view(np.uint32).any()
        assert not rec[:, [19, 23]].view(np.uint32).any()
        for k in np.flatnonzero(kind):
            m = rec[k, :12].reshape(3, 4).astype(np.float64)
            nm = rec[k, 12:].reshape(3, 4)[:, :3].astype(np.float64)
            obj = np.append(rng.uniform(-3, 3, (50, 3)), np.ones((50, 1)), 1)
            p_cur, p_prev = obj @ world(cur, k).T, obj @ world(prev, k).T
            got = p_cur @ m.T
            assert (np.linalg.norm(got - p_prev[:, :3], axis=1) <= 1e-5 * np.linalg.norm(p_prev[:, :3], axis=1)).all()
            assert np.abs(nm - m[:, :3]).max() <= 1e-5
    # uniform scale keeps n' unit: Nm = L^-T * |det L|^(1/3) is the rotation
    prev = [Node(-1, -1), Node(0, 0, *trs((1, 2, 3), (0, 0, 1), 0.5, 2.0))]
    cur = [Node(-1, -1), Node(0, 0, *trs((0, 2, 3), (0, 1, 1), 0.9, 0.5))]
    nm = node_motion(prev, cur)[1, 12:].reshape(3, 4)[:, :3].astype(np.float64)
    assert np.abs(nm @ nm.T - np.eye(3)).max() <= 1e-6
    # (parent, fwd) pairs and dicts are node lists too
    as_pairs = node_motion([(n.parent, n.fwd) for n in prev], [dict(parent=n.parent, fwd=n.fwd) for n in cur])
    assert np.array_equal(bits(as_pairs), bits(node_motion(prev, cur)))


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: every comparison on bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


def accumulator(api, w, h, moments, params=None):
    return api.TemporalAccumulator(w, h, device=0, moments=moments, **params_of(moments, params))


def device_frame(acc, fr, demodulate, in_place=False, **kw):
    frame, var = fr["rgba"].copy(), fr["variance"].copy()
    got = acc.accumulate(fr["camera"], frame, var, aovs_of(fr, demodulate), demodulate=demodulate,
                         out=frame if in_place else None, out_variance=var if in_place else None, **kw)
    if not in_place:
        assert np.array_equal(bits(frame), bits(fr["rgba"])) and np.array_equal(bits(var), bits(fr["variance"]))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_device_accumulate_equals_the_numpy_statement_on_bits(gpu_api, w, h):
    """k_tp_accumulate<., true> through api.TemporalAccumulator.accumulate(motion=) — the host entries — == the NumPy statement,
    bit for bit: frame, variance and length of all four frames, all four sequences, both forms, demodulation on and off, and with
    the outputs aliasing the inputs."""
    for seq in SEQUENCES:
        for moments in (False, True):
            for dm, in_place in ((False, False), (True, False), (True, True)):
                want = reference(w, h, seq, dm, moments)
                acc = accumulator(gpu_api, w, h, moments)
                for k, fr in enumerate(frames_of(w, h, seq)):
                    got = device_frame(acc, fr, dm, in_place, motion=fr["motion"])
                    tag = f"temporal motion {w}x{h} {seq} moments {moments} demodulate {dm} in_place {in_place} frame {k}"
                    bit_identical_or_drift(got[0], want[k][0], tag)
                    assert_same(got, want[k], tag)
                acc.close()


def run_torch_child(call):
    code = ("import torch\ntorch.cuda.set_device(0)\nfrom tests import test_temporal_motion as t\nt." + call + "\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def child_accumulate_into():
    import torch
    from yart_amd import api
    for w, h in GPU_SIZES:
        for seq in SEQUENCES:
            for moments in (False, True):
                dm = seq in ("mixed", "turn")
                want = reference(w, h, seq, dm, moments)
                dev = accumulator(api, w, h, moments)
                side = torch.cuda.Stream()
                for k, fr in enumerate(frames_of(w, h, seq)):
                    t = {name: torch.from_numpy(fr[name].copy()).cuda() for name in fr if isinstance(fr[name], np.ndarray) and name != "motion"}
                    torch.cuda.synchronize()
                    with torch.cuda.stream(side):
                        if k == 1:                       # in place, nothing optional
                            out, var = t["rgba"], t["variance"]
                            dev.accumulate_into(out, var, None, fr["camera"], out, var, aovs_of(t, dm), demodulate=dm, motion=fr["motion"])
                            got = (out.cpu().numpy(), var.cpu().numpy(), want[k][2])
                        else:
                            out, var = torch.zeros_like(t["rgba"]), torch.zeros_like(t["variance"])
                            ln = torch.zeros((h, w), dtype=torch.int32, device="cuda")
                            dev.accumulate_into(out, var, ln, fr["camera"], t["rgba"], t["variance"], aovs_of(t, dm), demodulate=dm,
                                                motion=fr["motion"])
                            got = (out.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy().view(np.uint32))
                            for name in t:
                                assert np.array_equal(bits(t[name].cpu().numpy()), bits(fr[name])), name + " was written"
                    assert_same(got, want[k], f"accumulate_into {w}x{h} {seq} moments {moments} frame {k}")
                dev.close()


@pytest.mark.gpu
def test_accumulate_into_equals_the_numpy_statement_on_bits(gpu_api):
    """api.TemporalAccumulator.accumulate_into(motion=) — the device entries — on torch tensors, on a non-default stream (the
    records are uploaded on it), at every size: the NumPy statement's bits, all four sequences, both forms; inputs untouched when
    out != in; in place, and without the optional outputs, too."""
    run_torch_child("child_accumulate_into()")


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [False, True])
def test_the_motion_is_consumed(gpu_api, moments):
    """`inplane` at 37 x 23: frame 1 is accumulated with its motion, frame 2 without a setter call: frame 2 equals the statement
    with motion=None for it, on bits, and not the one with frame 2's motion. The same after a motion is set and the handle then
    reset, after a motion is set and then refused, and when the accumulate call that follows the setter is itself refused (it did
    not pass its argument checks, so the motion waits for the next one)."""
    from yart_amd.temporal import TemporalHistory
    api = gpu_api
    w, h = 37, 23
    fr = frames_of(w, h, "inplane")
    prm = params_of(moments)

    def states(motions, start=0):
        hist = TemporalHistory(w, h)
        return [statement(hist, f, False, moments, prm, m) for f, m in zip(fr[start:], motions)]
    want = states([None, fr[1]["motion"], None])
    assert (bits(want[2][0]) != bits(states([None, fr[1]["motion"], fr[2]["motion"]])[2][0])).any()
    acc = accumulator(api, w, h, moments)
    device_frame(acc, fr[0], False)
    assert_same(device_frame(acc, fr[1], False, motion=fr[1]["motion"]), want[1], "frame 1, with its motion")
    assert_same(device_frame(acc, fr[2], False), want[2], "frame 2, no setter call")
    # set, then reset: the next frame is a first frame and the one after it has no motion
    acc.set_motion(fr[2]["motion"])
    acc.reset()
    want = states([None, None], start=1)
    assert (bits(want[1][0]) != bits(states([None, fr[2]["motion"]], start=1)[1][0])).any()
    assert_same(device_frame(acc, fr[1], False), want[0], "first frame after the reset")
    assert_same(device_frame(acc, fr[2], False), want[1], "second frame after the reset")
    # set, then a refused motion: nothing is pending
    acc.reset()
    device_frame(acc, fr[1], False)
    acc.set_motion(fr[2]["motion"])
    bad = fr[2]["motion"].copy()
    bad.view(np.uint32)[0, 15] = 7
    with pytest.raises(api.YartError, match="kind"):
        acc.set_motion(bad)
    assert_same(device_frame(acc, fr[2], False), want[1], "after a refused motion")
    # a refused accumulate call does not consume: the motion applies to the next call that passes its checks
    acc.reset()
    device_frame(acc, fr[1], False)
    acc.set_motion(fr[2]["motion"])
    with pytest.raises(api.YartError, match="alpha_min"):
        device_frame(acc, fr[2], False, alpha_min=2.0)
    assert_same(device_frame(acc, fr[2], False), states([None, fr[2]["motion"]], start=1)[1], "after a refused accumulate call")
    acc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [False, True])
def test_device_static_pixels_and_a_cleared_motion(gpu_api, moments):
    """test_temporal.py's `move` inputs at 37 x 23 (node ids > 500000) on the device: an all-static motion, a 3-record motion for
    which every id is out of range, and a motion set and then cleared with NULL each give the bits of the statement without a motion."""
    rng = np.random.RandomState(5)
    all_static = rng.normal(0, 3, (5, 24)).astype(np.float32)
    all_static.view(np.uint32)[:, 15] = 0
    out_of_range = np.stack([moving_record(rng.normal(0, 1, (3, 4)), rng.normal(0, 1, (3, 3))) for _ in range(3)])
    from yart_amd.temporal import TemporalHistory
    w, h = 37, 23
    prm = params_of(moments, dict(tt.PARAMS, **({"min_moment_history": 2} if moments else {})))
    frames = tt.frames_of(w, h, "move")
    hist = TemporalHistory(w, h)
    want = [statement(hist, dict(f), True, moments, prm, None) for f in frames]
    for case in ("static", "range", "cleared"):
        acc = accumulator(gpu_api, w, h, moments, prm)
        for k, f in enumerate(frames):
            if case == "cleared":
                acc.set_motion(out_of_range if k != 1 else all_static)
                acc.set_motion(None)
                got = device_frame(acc, f, True)
            else:
                got = device_frame(acc, f, True, motion=all_static if case == "static" else out_of_range)
            assert_same(got, want[k], f"{case} frame {k}")
        acc.close()


RENDER_SIZE, RENDER_SPP, RENDER_FRAMES, RENDER_STEP = (48, 32), 4, 3, 0.5
MOVED_NODE = 2


def render_scene(k):
    """The cornell room (node 1) with two cubes of edge 3 under the root: node 2, centred on the camera's axis so that only its front
    face is seen, 0.5 nearer to the camera in every frame (plane_tolerance * depth is about 0.1 there), and node 3, static."""
    from yart_amd import scenes
    from yart_amd.yscn import Material, trs
    s, p = scenes.cornell(RENDER_SIZE[0], RENDER_SIZE[1], RENDER_SPP, 4)
    b = scenes.MeshBuilder()
    b.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), s.add_material(Material(base=(0.3, 0.5, 0.8), roughness=0.8)))
    cube = s.add_mesh(b.build())
    assert s.add_node(cube, 0, *trs((0.0, 5.0, 3.0 + RENDER_STEP * k), scale=3.0)) == MOVED_NODE
    s.add_node(cube, 0, *trs((-3.0, 8.0, 2.0), (0, 1, 0), 0.4, 1.5))
    s.create_area_lights()
    return s, p


def erode(mask):
    m = mask.copy()
    m[1:] &= mask[:-1]
    m[:-1] &= mask[1:]
    m[:, 1:] &= mask[:, :-1]
    m[:, :-1] &= mask[:, 1:]
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    return m


def child_render_denoised():
    from yart_amd import api
    from yart_amd.temporal import TemporalHistory, node_motion, temporal_reference
    w, h = RENDER_SIZE
    acc, plain = api.TemporalAccumulator(w, h, device=0), api.TemporalAccumulator(w, h, device=0)
    hist, hist_plain = TemporalHistory(w, h), TemporalHistory(w, h)
    prev, inside = None, np.ones((h, w), bool)
    for k in range(RENDER_FRAMES):
        s, p = render_scene(k)
        scene = api.DeviceScene(s, device=0)
        motion = None if prev is None else node_motion(prev, s.nodes)
        if motion is not None:
            assert motion.view(np.uint32)[:, 15].tolist() == [0, 0, 1, 0]
        noisy, clean, g = scene.render_denoised(p, temporal=acc, motion=motion)
        _, _, g0 = scene.render_denoised(p, temporal=plain)
        scene.close()
        buf = {name: g[name].cpu().numpy() for name in ("variance", "position", "normal", "depth", "coverage", "ids", "albedo")}
        frame = noisy.cpu().numpy()
        for name in buf:
            assert np.array_equal(bits(g0[name].cpu().numpy()), bits(buf[name])), name
        args = (p, frame, buf["variance"], buf["position"], buf["normal"], buf["depth"], buf["coverage"], buf["ids"], buf["albedo"])
        want = temporal_reference(hist, *args, demodulate=True, motion=motion)
        want0 = temporal_reference(hist_plain, *args, demodulate=True)
        for got, ref, tag in ((g, want, "with the motion"), (g0, want0, "without it")):
            dev = (got["accumulated"].cpu().numpy(), got["accumulated_variance"].cpu().numpy(), got["length"].cpu().numpy().view(np.uint32))
            assert_same(dev, ref, f"render_denoised frame {k} {tag}")
        want_clean = api.denoise_var(want[0], want[1], buf["albedo"], buf["normal"], buf["depth"], demodulate=True)
        assert np.array_equal(bits(clean.cpu().numpy()), bits(want_clean)), "denoised frame"
        inside &= (buf["ids"][..., 0] == MOVED_NODE) & (buf["coverage"] == 1.0)
        if prev is not None:                            # the move is more than the plane test lets through
            assert RENDER_STEP > 2 * 0.01 * float(buf["depth"][inside].max())
        prev = s.nodes
    checked = erode(erode(inside))
    share, share0 = (want[2][checked] == RENDER_FRAMES).mean(), (want0[2][checked] > 1).mean()
    print(f"render: {int(checked.sum())} checked pixels; length {RENDER_FRAMES} with the motion at {share:.3f}, length > 1 without it at {share0:.3f}")
    assert checked.sum() >= 30
    assert share > 0.5 and share0 == 0.0                # on the statement: the device's lengths are its bits (above)
    dev_len, dev_len0 = g["length"].cpu().numpy().view(np.uint32), g0["length"].cpu().numpy().view(np.uint32)
    assert (dev_len[checked] == RENDER_FRAMES).mean() > 0.5 and not (dev_len0[checked] > 1).any()
    acc.close()
    plain.close()


@pytest.mark.gpu
def test_render_denoised_with_node_motion(gpu_api):
    """End to end: the cornell room with two cubes at 48 x 32 and 4 spp, three frames, the scene re-created per frame with one cube
    0.5 nearer to the camera; DeviceScene.render_denoised(temporal=acc, motion=node_motion(previous nodes, these)). The accumulated
    frame, variance and length are the NumPy statement's on the same rendered buffers, on bits, with the motion and without it. On
    the pixels of the moved node with coverage 1 in all three frames, after two 4-neighbour erosions: more than half reach length
    3 with the motion, none exceeds 1 without it — on the statement and on the device."""
    run_torch_child("child_render_denoised()")
