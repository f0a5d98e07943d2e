"""Temporal accumulation with camera reprojection (``yart_hip_temporal_*``) stated in NumPy float32.

:func:`temporal_reference` is written from the definition in the header comment of ``include/yart_hip.h`` (current pixel,
projection, tap validation, blend, new history record), vectorised over the pixels with an explicit loop over the four taps,
every operation a float32 operation in the order the definition gives. It is what the tests hold the device kernel (and
``csrc/temporal.hpp`` compiled for the host) to, bit for bit. :func:`camera_basis` restates the derived camera quantities
(``csrc/host_scene.hpp`` makeCamera) the projection starts from. No libm: only + - * /, sqrt (correctly rounded), floor and
comparisons.
"""
from __future__ import annotations

import numpy as np

# include/yart_hip.h: YART_TEMPORAL_DEFAULT_* (chosen by profiles/temporal_sweep.txt) and YART_TEMPORAL_DEMODULATE
DEFAULT_ALPHA_MIN = 0.1
DEFAULT_MAX_HISTORY = 8
DEFAULT_NORMAL_COS_MIN = 0.8
DEFAULT_PLANE_TOLERANCE = 0.01
FLAG_DEMODULATE = 1

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


class TemporalHistory:
    """The state of a ``YartTemporal`` handle: the history records of the last accumulated frame — ``colour`` (H, W, 3),
    ``variance`` (H, W), ``position`` (H, W, 3), ``length`` (H, W) uint32, ``normal`` (H, W, 3), ``node`` (H, W) uint32 — and
    that frame's camera; ``camera`` None: empty (a new handle, or after ``reset``)."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.reset()

    def reset(self):
        self.camera = None
        self.colour = self.variance = self.position = self.length = self.normal = self.node = None


def temporal_reference(history, cam, rgba, variance, position, normal, depth, coverage, ids, albedo=None,
                       alpha_min=DEFAULT_ALPHA_MIN, max_history=DEFAULT_MAX_HISTORY, normal_cos_min=DEFAULT_NORMAL_COS_MIN,
                       plane_tolerance=DEFAULT_PLANE_TOLERANCE, demodulate=None):
    """One frame: ``history`` (a :class:`TemporalHistory`, updated in place), ``cam`` the frame's camera (see
    :func:`camera_fields`), ``rgba`` (H, W, 4), ``variance`` (H, W), ``position`` / ``normal`` (H, W, 3), ``depth`` / ``coverage``
    (H, W), ``ids`` (H, W, 4) int32, ``albedo`` (H, W, 3) or None. ``demodulate``: None = whenever an albedo buffer is given.
    Returns (accumulated frame (H, W, 4) float32, its variance (H, W) float32, history length (H, W) uint32)."""
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
        acc = np.zeros((h, w, 3), _F)
        acc_v = np.zeros((h, w), _F)
        wsum = np.zeros((h, w), _F)
        min_len = np.full((h, w), 0xffffffff, np.uint32)
        any_tap = np.zeros((h, w), bool)
        if history.camera is not None:
            # -- projection into the previous camera ----------------------------------------------------------------------
            k = camera_basis(history.camera)
            nrm = _cross(k["dU"], k["dV"])
            num = _dot((k["top_left"] - k["position"]).astype(_F), nrm)
            duu, dvv = _dot(k["dU"], k["dU"]), _dot(k["dV"], k["dV"])
            rel = (P - k["position"]).astype(_F)
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
                nq, pq = history.normal[cy, cx], history.position[cy, cx]
                counts = inside & (wt > 0) & (ln >= 1) & (history.node[cy, cx] == node)
                counts &= _dot(n, nq) >= normal_cos_min
                counts &= np.abs(_dot(n, (pq - P).astype(_F))) <= tol
                acc = np.where(counts[..., None], acc + wt[..., None] * history.colour[cy, cx], acc).astype(_F)
                acc_v = np.where(counts, acc_v + wt * history.variance[cy, cx], acc_v).astype(_F)
                wsum = np.where(counts, wsum + wt, wsum).astype(_F)
                min_len = np.where(counts & (ln < min_len), ln, min_len)
                any_tap |= counts
        # -- blend ------------------------------------------------------------------------------------------------------------
        hc = acc / wsum[..., None]
        hv = acc_v / wsum
        N = np.where(min_len >= max_history, max_history, min_len + np.uint32(1)).astype(np.uint32)
        N = np.where(any_tap, N, np.uint32(1)).astype(np.uint32)
        inv = _F(1.0) / N.astype(_F)
        a = np.where(inv > alpha_min, inv, alpha_min).astype(_F)
        b = _F(1.0) - a
        out_c = np.where(any_tap[..., None], hc + a[..., None] * (c - hc), c).astype(_F)
        out_v = np.where(any_tap, (a * a) * v + (b * b) * hv, v).astype(_F)
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
    return out, out_var, length
