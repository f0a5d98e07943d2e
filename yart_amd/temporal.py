"""Temporal accumulation with camera reprojection (``yart_hip_temporal_*``) stated in NumPy float32.

:func:`temporal_reference` is written from the definition in the header comment of ``include/yart_hip.h`` (current pixel,
projection, tap validation, blend, new history record), vectorised over the pixels with an explicit loop over the four taps,
every operation a float32 operation in the order the definition gives. It is what the tests hold the device kernel (and
``csrc/temporal.hpp`` compiled for the host) to, bit for bit. :func:`camera_basis` restates the derived camera quantities
(``csrc/host_scene.hpp`` makeCamera) the projection starts from. No libm: only + - * /, sqrt (correctly rounded), floor and
comparisons.

:func:`temporal_moments_reference` states the moments form (``yart_hip_temporal_accumulate_moments_*``): the same pass with the
luminance moments and the sum of squared frame weights accumulated next to the colour, the temporal variance estimate they give,
and the second pass that estimates the variance of the short pixels from their 7 x 7 neighbourhood.

Both take ``motion``: the per-node motion records of ``yart_hip_temporal_set_motion`` — how each scene node moved since the
previous frame — which :func:`node_motion` builds from the node lists of the two frames' scenes; and ``pixel_motion``: the
per-pixel records of ``yart_hip_temporal_set_pixel_motion`` — where each pixel's surface point was, and what its normal was, in
the previous frame —, which ``yart_amd.scene_motion.scene_motion_reference`` states: the motion of deforming meshes.

And ``clip``: the setting of ``yart_hip_temporal_set_clip`` — the fetched history is clipped to the statistics of the frame's
demodulated colour over a small window before the blend (:func:`_clip_history`), against the ghosting a change of the lighting
leaves in a history whose taps are all geometrically valid.
"""
from __future__ import annotations

import numpy as np

# include/yart_hip.h: YART_TEMPORAL_DEFAULT_* (chosen by profiles/temporal_sweep.txt) and YART_TEMPORAL_DEMODULATE
DEFAULT_ALPHA_MIN = 0.1
DEFAULT_MAX_HISTORY = 8
DEFAULT_NORMAL_COS_MIN = 0.8
DEFAULT_PLANE_TOLERANCE = 0.01
FLAG_DEMODULATE = 1
# include/yart_hip.h: YART_TEMPORAL_DEFAULT_MIN_MOMENT_HISTORY (SVGF's value; profiles/temporal_moments_sweep.txt) and the half
# width of the spatial estimate's window
DEFAULT_MIN_MOMENT_HISTORY = 4
SPATIAL_RADIUS = 3
# include/yart_hip.h: YartTemporalMotion — floats per record, the word that holds kind, the kinds, and the (exclusive) node limit
MOTION_WORDS = 24
MOTION_KIND_WORD = 15
MOTION_STATIC, MOTION_MOVING = 0, 1
MOTION_MAX_NODES = 1 << 20
# include/yart_hip.h: YartTemporalPixelMotion — floats per record and the word that holds kind
PIXEL_MOTION_WORDS = 8
PIXEL_MOTION_KIND_WORD = 3
# include/yart_hip.h: YART_TEMPORAL_DEFAULT_CLIP_* (chosen by profiles/temporal_clip_sweep.txt) and the limits of YartTemporalClip
DEFAULT_CLIP_RADIUS = 1
DEFAULT_CLIP_GAMMA = 0.5
CLIP_MAX_RADIUS = 3

_F = np.float32
_FLT_MAX = np.float32(3.4028235e38)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(_F)


def _luma(d):
    return (d[..., 0] * _F(0.2126) + d[..., 1] * _F(0.7152)) + d[..., 2] * _F(0.0722)


def camera_fields(cam):
    """(width, height, focal, sensor, position, target, up) of a camera given in the vocabulary of ``api.make_camera`` (a dict
    with size / focal / sensor / eye / target / up) or as an ``api.CameraDesc``."""
    if isinstance(cam, dict):
        w, h = int(cam["size"][0]), int(cam["size"][1])
        return (w, h, _F(cam.get("focal", 35.0)), np.asarray(cam.get("sensor", (36.0, 24.0)), _F), np.asarray(cam["eye"], _F),
                np.asarray(cam["target"], _F), np.asarray(cam.get("up", (0, 1, 0)), _F))
    return (int(cam.width), int(cam.height), _F(cam.focal_length), np.asarray(list(cam.sensor), _F),
            np.asarray(list(cam.position), _F), np.asarray(list(cam.target), _F), np.asarray(list(cam.up), _F))


def camera_basis(cam):
    """Camera::calcDerivedProperties after moveAndLookAt as csrc/host_scene.hpp makeCamera forms it, in float32:
    dict(position, top_left (topLeftPixel), dU (pixelDeltaU), dV (pixelDeltaV))."""
    w, h, focal, sensor, position, target, up = camera_fields(cam)
    with np.errstate(all="ignore"):
        aspect = _F(w) / _F(h)
        forward = (target - position).astype(_F)
        if _dot(up, up) == 0:
            up = np.array([0, 1, 0], _F)
        sensor_aspect = sensor[0] / sensor[1]
        cropped = sensor[0] / (sensor_aspect if sensor_aspect > aspect else aspect)
        focus = np.sqrt(_dot(forward, forward))
        vh = focus * cropped / focal
        vw = vh * aspect
        up = (up / np.sqrt(_dot(up, up))).astype(_F)
        back = -forward
        wv = (back / np.sqrt(_dot(back, back))).astype(_F)
        u = _cross(up, wv)
        v = _cross(wv, u)
        viewport_u = (u * vw).astype(_F)
        viewport_v = ((-v) * vh).astype(_F)
        top = ((position - wv * focus) - (viewport_u + viewport_v) * _F(0.5)).astype(_F)
        du = (viewport_u / _F(w)).astype(_F)
        dv = (viewport_v / _F(h)).astype(_F)
        tl = (top + (du + dv) * _F(0.5)).astype(_F)
    return dict(position=position.astype(_F), top_left=tl, dU=du, dV=dv)


def motion_records(motion):
    """``motion`` as the (n_nodes, 24) float32 array of records, checked as ``yart_hip_temporal_set_motion`` checks it."""
    rec = np.ascontiguousarray(motion)
    assert rec.dtype == np.float32, "motion records are float32 (kind is a uint32 stored as bits)"
    rec = rec.reshape(-1, MOTION_WORDS)
    assert 1 <= len(rec) < MOTION_MAX_NODES, "n_nodes is 0 or not below 2^20"
    kind = rec[:, MOTION_KIND_WORD].view(np.uint32)
    assert (kind <= MOTION_MOVING).all(), "a record's kind is neither 0 nor 1"
    words = np.delete(rec[kind == MOTION_MOVING], MOTION_KIND_WORD, axis=1)
    assert np.isfinite(words).all(), "a word of a moving node's record is not finite"
    return rec


def pixel_motion_records(pixel_motion, width, height):
    """``pixel_motion`` as the (H, W, 8) float32 array of records"""
    rec = np.ascontiguousarray(pixel_motion)
    assert rec.dtype == np.float32, "pixel motion records are float32 (kind is a uint32 stored as bits)"
    assert rec.size == width * height * PIXEL_MOTION_WORDS, "pixel motion: 8 floats per pixel"
    return rec.reshape(height, width, PIXEL_MOTION_WORDS)


def _node_field(node, name, index):
    if isinstance(node, dict):
        return node[name]
    return getattr(node, name) if hasattr(node, name) else node[index]


def node_motion(nodes_prev, nodes_cur):
    """The per-node motion records from the node lists of the previous and the current frame's scene (``yscn.Scene.nodes``, or
    anything with ``parent`` and ``fwd`` — attributes, keys, or (parent, fwd) pairs —, a parent before its children): the
    (n_nodes, 24) float32 array ``TemporalAccumulator.accumulate(..., motion=)`` and the references take.
    In float64: W_k = W_parent(k) · fwd_k is node k's object-to-world transform — csrc/traverse.hpp objectRay takes a world ray
    to object space with the chain's ``inv`` root first (row-major matrices, column vectors: ymath.hpp mulPoint), so object to
    world is the ``fwd`` chain with the root on the left. M = W_prev · W_cur^-1 takes a point attached to the node from this
    frame's world space to the previous frame's; with L its linear part, Nm = L^-T · |det L|^(1/3) takes the normal — exact (a
    unit n' for a unit n) for rigid motion and uniform scale; any other motion leaves n' non-unit, which shifts the normal test.
    kind = 0 (static, the other words 0) exactly when the node's ``fwd`` chain up to the root is the same in both lists, word
    for word; else 1."""
    assert len(nodes_prev) == len(nodes_cur), "the two frames' scenes do not have the same nodes"
    n = len(nodes_cur)
    rec = np.zeros((n, MOTION_WORDS), _F)
    kind = rec[:, MOTION_KIND_WORD].view(np.uint32)
    world, same = [[None] * n, [None] * n], [None] * n
    for k in range(n):
        parent = int(_node_field(nodes_cur[k], "parent", 0))
        assert parent == int(_node_field(nodes_prev[k], "parent", 0)) and parent < k, "node %d: another or a later parent" % k
        fwd = [np.asarray(_node_field(nodes[k], "fwd", 1), _F).reshape(4, 4) for nodes in (nodes_prev, nodes_cur)]
        same[k] = bool((fwd[0].view(np.uint32) == fwd[1].view(np.uint32)).all()) and (parent < 0 or same[parent])
        for j in (0, 1):
            world[j][k] = fwd[j].astype(np.float64) if parent < 0 else world[j][parent] @ fwd[j].astype(np.float64)
        if same[k]:
            continue
        m = world[0][k] @ np.linalg.inv(world[1][k])
        lin = m[:3, :3]
        rec[k, :12] = m[:3].reshape(12)
        rec[k, 12:].reshape(3, 4)[:, :3] = np.linalg.inv(lin).T * abs(np.linalg.det(lin)) ** (1.0 / 3.0)
        kind[k] = MOTION_MOVING
    return rec


def clip_of(clip):
    """``clip`` as ``yart_hip_temporal_set_clip`` takes it: None (off), or (radius, gamma) checked as the entry checks them;
    True: the defaults."""
    if clip is None or clip is False:
        return None
    if clip is True:
        return DEFAULT_CLIP_RADIUS, DEFAULT_CLIP_GAMMA
    radius, gamma = clip
    assert int(radius) == radius and 1 <= int(radius) <= CLIP_MAX_RADIUS, "clip: radius is outside 1 .. 3"
    assert np.isfinite(_F(gamma)) and _F(gamma) >= 0, "clip: gamma is not finite or is negative"
    return int(radius), float(gamma)


class TemporalHistory:
    """The state of a ``YartTemporal`` handle: the history records of the last accumulated frame — ``colour`` (H, W, 3),
    ``variance`` (H, W), ``position`` (H, W, 3), ``length`` (H, W) uint32, ``normal`` (H, W, 3), ``node`` (H, W) uint32 — and
    that frame's camera; ``camera`` None: empty (a new handle, or after ``reset``). In the moments form also ``moments``
    (H, W, 3): m1, m2 and w2 of the accumulated luminance. ``form``: "plain" or "moments" from the first frame after a reset."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.reset()

    def reset(self):
        self.camera = None
        self.colour = self.variance = self.position = self.length = self.normal = self.node = None
        self.moments = self.form = None


def temporal_reference(history, cam, rgba, variance, position, normal, depth, coverage, ids, albedo=None,
                       alpha_min=DEFAULT_ALPHA_MIN, max_history=DEFAULT_MAX_HISTORY, normal_cos_min=DEFAULT_NORMAL_COS_MIN,
                       plane_tolerance=DEFAULT_PLANE_TOLERANCE, demodulate=None, motion=None, pixel_motion=None, clip=None):
    """One frame: ``history`` (a :class:`TemporalHistory`, updated in place), ``cam`` the frame's camera (see
    :func:`camera_fields`), ``rgba`` (H, W, 4), ``variance`` (H, W), ``position`` / ``normal`` (H, W, 3), ``depth`` / ``coverage``
    (H, W), ``ids`` (H, W, 4) int32, ``albedo`` (H, W, 3) or None. ``demodulate``: None = whenever an albedo buffer is given.
    ``motion``: None, or the (n_nodes, 24) float32 per-node motion records of this frame (``kind`` as bits in column 15; see
    :func:`node_motion`): a pixel whose ``ids[0]`` is below n_nodes and whose record's kind is 1 is projected, and its taps are
    validated, with P' = M P and n' = Nm n; every other pixel is untouched by it.
    ``pixel_motion`` (not together with ``motion``): None, or the (H, W, 8) float32 per-pixel records of
    ``yart_hip_temporal_set_pixel_motion`` (``yart_amd.scene_motion.scene_motion_reference``): a pixel whose record's kind (the
    bits of word 3) is 1 takes P' from words 0 .. 2 and n' from words 4 .. 6; every other pixel is untouched by it.
    ``clip``: None, True (the defaults) or (radius, gamma), the setting of ``yart_hip_temporal_set_clip``: the fetched history is
    clipped to mean +- gamma * standard deviation of the frame's demodulated colour over the (2 radius + 1)^2 window.
    Returns (accumulated frame (H, W, 4) float32, its variance (H, W) float32, history length (H, W) uint32)."""
    return _accumulate(history, cam, rgba, variance, position, normal, depth, coverage, ids, albedo, alpha_min, max_history,
                       normal_cos_min, plane_tolerance, demodulate, None, motion, pixel_motion, clip)


def temporal_moments_reference(history, cam, rgba, variance, position, normal, depth, coverage, ids, albedo=None,
                               alpha_min=DEFAULT_ALPHA_MIN, max_history=DEFAULT_MAX_HISTORY,
                               normal_cos_min=DEFAULT_NORMAL_COS_MIN, plane_tolerance=DEFAULT_PLANE_TOLERANCE,
                               min_moment_history=DEFAULT_MIN_MOMENT_HISTORY, demodulate=None, motion=None, pixel_motion=None,
                               clip=None):
    """One frame of the moments form; arguments and results as :func:`temporal_reference`, and ``min_moment_history`` (>= 2).
    The history additionally carries ``moments``; a history is in one form from its first frame to the next ``reset``."""
    assert int(min_moment_history) >= 2
    return _accumulate(history, cam, rgba, variance, position, normal, depth, coverage, ids, albedo, alpha_min, max_history,
                       normal_cos_min, plane_tolerance, demodulate, int(min_moment_history), motion, pixel_motion, clip)


def _clip_history(clip, c, alb, any_tap, hc, hm, moments):
    """The clip of the definition: the history colour ``hc`` (and h1, h2 of ``hm`` in the moments form) of the pixels with a
    counting tap set, clipped to the statistics of the frame's demodulated colour ``c`` over the window -> (hc, hm)."""
    radius, gamma = clip[0], _F(clip[1])
    h, w = c.shape[:2]
    counting = np.isfinite(c).all(-1)
    if alb is not None:
        counting &= np.isfinite(alb).all(-1)
    y = _luma(c)
    s1, s2 = np.zeros((h, w, 3), _F), np.zeros((h, w, 3), _F)
    sy1, sy2 = np.zeros((h, w), _F), np.zeros((h, w), _F)
    cnt = np.zeros((h, w), np.uint32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qy, qx = ys + dy, xs + dx
            cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            counts = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & counting[cy, cx]
            cq, yq = c[cy, cx], y[cy, cx]
            s1 = np.where(counts[..., None], s1 + cq, s1).astype(_F)
            s2 = np.where(counts[..., None], s2 + cq * cq, s2).astype(_F)
            sy1 = np.where(counts, sy1 + yq, sy1).astype(_F)
            sy2 = np.where(counts, sy2 + yq * yq, sy2).astype(_F)
            cnt = np.where(counts, cnt + np.uint32(1), cnt).astype(np.uint32)
    kf = cnt.astype(_F)
    applies = any_tap & (cnt >= 2)

    def clipped(value, t1, t2, k, applies):
        mu, e2 = t1 / k, t2 / k
        var = e2 - mu * mu
        var = np.where(var > _F(0.0), var, _F(0.0)).astype(_F)
        sd = np.sqrt(var)
        lo, hi = mu - gamma * sd, mu + gamma * sd
        to = np.where(value < lo, lo, np.where(value > hi, hi, value)).astype(_F)
        applies = applies & np.isfinite(mu) & np.isfinite(e2) & np.isfinite(sd)
        return np.where(applies, to, value).astype(_F), applies
    hc, _ = clipped(hc, s1, s2, kf[..., None], applies[..., None])
    if moments:
        h1, applied = clipped(hm[..., 0], sy1, sy2, kf, applies)
        moved = applied & (h1 != hm[..., 0])
        h2 = np.where(moved, hm[..., 1] + (h1 * h1 - hm[..., 0] * hm[..., 0]), hm[..., 1]).astype(_F)
        hm = np.stack([h1, h2, hm[..., 2]], -1).astype(_F)
    return hc, hm


def _accumulate(history, cam, rgba, variance, position, normal, depth, coverage, ids, albedo, alpha_min, max_history,
                normal_cos_min, plane_tolerance, demodulate, min_moment_history, motion=None, pixel_motion=None, clip=None):
    """Pass 1 of both forms (``min_moment_history`` None: the plain form), then pass 2 of the moments form."""
    moments = min_moment_history is not None
    clip = clip_of(clip)
    form = "moments" if moments else "plain"
    assert history.camera is None or history.form == form, "the history is in the other form: reset it first"
    if demodulate is None:
        demodulate = albedo is not None
    if demodulate and albedo is None:
        raise ValueError("demodulate needs an albedo buffer")
    h, w = history.height, history.width
    assert camera_fields(cam)[:2] == (w, h)
    assert 0.0 <= alpha_min <= 1.0 and max_history >= 1
    rgba = np.asarray(rgba, _F).reshape(h, w, 4)
    variance = np.asarray(variance, _F).reshape(h, w)
    P = np.asarray(position, _F).reshape(h, w, 3)
    n = np.asarray(normal, _F).reshape(h, w, 3)
    depth = np.asarray(depth, _F).reshape(h, w)
    coverage = np.asarray(coverage, _F).reshape(h, w)
    node = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(h, w, 4)[..., 0]).view(np.uint32)
    alpha_min, normal_cos_min, plane_tolerance = _F(alpha_min), _F(normal_cos_min), _F(plane_tolerance)
    max_history = np.uint32(max_history)
    with np.errstate(all="ignore"):
        # -- current pixel ------------------------------------------------------------------------------------------------
        if demodulate:
            alb = np.asarray(albedo, _F).reshape(h, w, 3)
            d = np.where(alb > _F(1e-3), alb, _F(1.0)).astype(_F)
        else:
            alb, d = None, np.ones((h, w, 3), _F)
        c = (rgba[..., :3] / d).astype(_F)
        ld = _luma(d)
        ld2 = ld * ld
        v = variance / ld2
        usable = np.isfinite(c).all(-1) & np.isfinite(variance) & (variance >= 0) & np.isfinite(v)
        if alb is not None:
            usable &= np.isfinite(alb).all(-1)
        reproj = usable & (coverage == _F(1.0)) & np.isfinite(P).all(-1) & np.isfinite(n).all(-1) & np.isfinite(depth)
        Pq, nq = P, n                 # what is projected and what the taps are tested with: P', n' of a moving pixel
        if motion is not None:
            rec = motion_records(motion)
            in_range = node < np.uint32(len(rec))
            r = rec[np.where(in_range, node, np.uint32(0))]
            moving = in_range & (r[..., MOTION_KIND_WORD].view(np.uint32) == np.uint32(MOTION_MOVING))
            Pm = np.stack([_dot(r[..., 4 * i:4 * i + 3], P) + r[..., 4 * i + 3] for i in range(3)], -1).astype(_F)
            nm = np.stack([_dot(r[..., 12 + 4 * i:15 + 4 * i], n) for i in range(3)], -1).astype(_F)
            reproj &= ~moving | (np.isfinite(Pm).all(-1) & np.isfinite(nm).all(-1))
            Pq = np.where(moving[..., None], Pm, P).astype(_F)
            nq = np.where(moving[..., None], nm, n).astype(_F)
        if pixel_motion is not None:
            assert motion is None, "one motion at a time: per node or per pixel"
            r = pixel_motion_records(pixel_motion, w, h)
            moving = r[..., PIXEL_MOTION_KIND_WORD].view(np.uint32) == np.uint32(MOTION_MOVING)
            Pm, nm = r[..., 0:3], r[..., 4:7]
            reproj &= ~moving | (np.isfinite(Pm).all(-1) & np.isfinite(nm).all(-1))
            Pq = np.where(moving[..., None], Pm, P).astype(_F)
            nq = np.where(moving[..., None], nm, n).astype(_F)
        acc = np.zeros((h, w, 3), _F)
        acc_v = np.zeros((h, w), _F)
        wsum = np.zeros((h, w), _F)
        min_len = np.full((h, w), 0xffffffff, np.uint32)
        any_tap = np.zeros((h, w), bool)
        acc_m = np.zeros((h, w, 3), _F)
        if history.camera is not None:
            # -- projection into the previous camera ----------------------------------------------------------------------
            k = camera_basis(history.camera)
            nrm = _cross(k["dU"], k["dV"])
            num = _dot((k["top_left"] - k["position"]).astype(_F), nrm)
            duu, dvv = _dot(k["dU"], k["dU"]), _dot(k["dV"], k["dV"])
            rel = (Pq - k["position"]).astype(_F)
            s = num / _dot(rel, nrm)
            ok = reproj & (s > 0) & (s <= _FLT_MAX)
            X = ((k["position"] + rel * s[..., None]) - k["top_left"]).astype(_F)
            jx = _dot(X, k["dU"]) / duu
            jy = _dot(X, k["dV"]) / dvv
            ok &= (jx >= _F(-1.0)) & (jx < _F(w)) & (jy >= _F(-1.0)) & (jy < _F(h))
            flx, fly = np.floor(jx), np.floor(jy)
            x0 = np.where(ok, flx, 0).astype(np.int64)
            y0 = np.where(ok, fly, 0).astype(np.int64)
            fx, fy = jx - flx, jy - fly
            gx, gy = _F(1.0) - fx, _F(1.0) - fy
            tol = plane_tolerance * depth
            for t in range(4):
                qx, qy = x0 + (t & 1), y0 + (t >> 1)
                wt = (fx if t & 1 else gx) * (fy if t >> 1 else gy)
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                ln = history.length[cy, cx]
                nh, ph = history.normal[cy, cx], history.position[cy, cx]
                counts = inside & (wt > 0) & (ln >= 1) & (history.node[cy, cx] == node)
                counts &= _dot(nq, nh) >= normal_cos_min
                counts &= np.abs(_dot(nq, (ph - Pq).astype(_F))) <= tol
                acc = np.where(counts[..., None], acc + wt[..., None] * history.colour[cy, cx], acc).astype(_F)
                acc_v = np.where(counts, acc_v + wt * history.variance[cy, cx], acc_v).astype(_F)
                if moments:
                    acc_m = np.where(counts[..., None], acc_m + wt[..., None] * history.moments[cy, cx], acc_m).astype(_F)
                wsum = np.where(counts, wsum + wt, wsum).astype(_F)
                min_len = np.where(counts & (ln < min_len), ln, min_len)
                any_tap |= counts
        # -- blend ------------------------------------------------------------------------------------------------------------
        hc = acc / wsum[..., None]
        hv = acc_v / wsum
        hm = acc_m / wsum[..., None]
        if clip is not None:
            hc, hm = _clip_history(clip, c, alb, any_tap, hc, hm, moments)
        N = np.where(min_len >= max_history, max_history, min_len + np.uint32(1)).astype(np.uint32)
        N = np.where(any_tap, N, np.uint32(1)).astype(np.uint32)
        inv = _F(1.0) / N.astype(_F)
        a = np.where(inv > alpha_min, inv, alpha_min).astype(_F)
        b = _F(1.0) - a
        out_c = np.where(any_tap[..., None], hc + a[..., None] * (c - hc), c).astype(_F)
        out_v = np.where(any_tap, (a * a) * v + (b * b) * hv, v).astype(_F)
        if moments:
            # -- the luminance moments, the sum of squared frame weights, and the temporal estimate ---------------------------
            y = _luma(c)
            yy = y * y
            m1 = np.where(any_tap, hm[..., 0] + a * (y - hm[..., 0]), y).astype(_F)
            m2 = np.where(any_tap, hm[..., 1] + a * (yy - hm[..., 1]), yy).astype(_F)
            w2 = np.where(any_tap, (a * a) * _F(1.0) + (b * b) * hm[..., 2], _F(1.0)).astype(_F)
            vt = m2 - m1 * m1
            vt = np.where(vt > _F(0.0), vt, _F(0.0)).astype(_F)
            long_ = (N >= np.uint32(min_moment_history)) & (w2 < _F(1.0))
            out_v = np.where(long_, vt * (w2 / (_F(1.0) - w2)), out_v).astype(_F)
        out = np.empty((h, w, 4), _F)
        out[..., :3] = out_c * d
        out[..., 3] = rgba[..., 3]
        out_var = (out_v * ld2).astype(_F)
        length = N.copy()
        # -- pixels that are passed through, and the new history record -------------------------------------------------------
        bad = ~usable
        out[bad] = rgba[bad]
        out_var[bad] = variance[bad]
        length[bad] = 0
        history.colour = np.where(bad[..., None], _F(0), out_c).astype(_F)
        history.variance = np.where(bad, _F(0), out_v).astype(_F)
        history.position = np.where(bad[..., None], _F(0), P).astype(_F)
        history.normal = np.where(bad[..., None], _F(0), n).astype(_F)
        history.node = np.where(bad, np.uint32(0), node).astype(np.uint32)
        history.length = length.copy()
        history.camera = cam
        history.form = form
        if moments:
            history.moments = np.where(bad[..., None], _F(0), np.stack([m1, m2, w2], -1)).astype(_F)
            # -- pass 2: the short pixels' variance from their neighbourhood in the image pass 1 wrote ------------------------
            short = ~bad & ~long_
            tol = plane_tolerance * depth
            s1, s2 = np.zeros((h, w), _F), np.zeros((h, w), _F)
            cnt = np.zeros((h, w), np.uint32)
            ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            hn, hp = history.normal, history.position
            for dy in range(-SPATIAL_RADIUS, SPATIAL_RADIUS + 1):
                for dx in range(-SPATIAL_RADIUS, SPATIAL_RADIUS + 1):
                    qy, qx = ys + dy, xs + dx
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    counts = short & inside & (history.length[cy, cx] >= 1) & (history.node[cy, cx] == history.node)
                    counts &= _dot(hn, hn[cy, cx]) >= normal_cos_min
                    counts &= np.abs(_dot(hn, (hp[cy, cx] - hp).astype(_F))) <= tol
                    s1 = np.where(counts, s1 + history.moments[cy, cx, 0], s1).astype(_F)
                    s2 = np.where(counts, s2 + history.moments[cy, cx, 1], s2).astype(_F)
                    cnt = np.where(counts, cnt + np.uint32(1), cnt).astype(np.uint32)
            kf = cnt.astype(_F)
            e1, e2 = s1 / kf, s2 / kf
            vs = e2 - e1 * e1
            vs = np.where(vs > _F(0.0), vs, _F(0.0)).astype(_F)
            spatial = short & (cnt >= 2)
            v2 = (vs * (kf / (cnt - np.uint32(1)).astype(_F))) * history.moments[..., 2]
            history.variance = np.where(spatial, v2, history.variance).astype(_F)
            out_var = np.where(spatial, v2 * ld2, out_var).astype(_F)
    return out, out_var, length
