"""Per-pixel sample moments (include/yart_hip.h: YartMomentBuffers, yart_hip_render_moments) — the definition in NumPy.

``moments_reference`` is what the device kernels (csrc/moment_kernels.inc) and the host statement (csrc/moments.hpp) are
compared with, on bits: float32 for the per-sample values, float64 for the running sums, every operation rounded on its own
in the order the header comment writes it, samples in ascending order."""
from __future__ import annotations

import numpy as np

_LUMA = (np.float32(0.2126), np.float32(0.7152), np.float32(0.0722))


def luma(w):
    """csrc/estimator.hpp ``luma``: dot(w, (0.2126f, 0.7152f, 0.0722f)) as ymath.hpp associates it, in float32."""
    w = np.asarray(w, np.float32)
    with np.errstate(all="ignore"):
        return ((w[..., 0] * _LUMA[0] + w[..., 1] * _LUMA[1]).astype(np.float32) + w[..., 2] * _LUMA[2]).astype(np.float32)


def moments_reference(L, exposure_scale):
    """``L``: [..., S, C >= 3] per-sample radiance (before exposure; a fourth component is ignored), samples ascending along
    axis -2. Returns (mean [..., 3] float32, variance [...] float32, count [...] uint32): the mean of the accepted samples,
    the variance of the pixel's mean luminance estimate, the number of accepted samples."""
    L = np.asarray(L, np.float32)
    shape = L.shape[:-2]
    n = np.zeros(shape, np.uint32)
    sums = np.zeros(shape + (3,), np.float64)
    s1 = np.zeros(shape, np.float64)
    s2 = np.zeros(shape, np.float64)
    e = np.float32(exposure_scale)
    with np.errstate(all="ignore"):
        for s in range(L.shape[-2]):
            w = (L[..., s, :3] * e).astype(np.float32)
            y = luma(w)
            ok = (w >= 0).all(-1) & np.isfinite(y)          # (NaN >= 0 is False; -0.0 >= 0 is True)
            yd = y.astype(np.float64)
            sums = np.where(ok[..., None], sums + w.astype(np.float64), sums)
            s1 = np.where(ok, s1 + yd, s1)
            s2 = np.where(ok, s2 + yd * yd, s2)
            n = n + ok.astype(np.uint32)
        nd = n.astype(np.float64)
        mean = np.where((n > 0)[..., None], (sums / nd[..., None]).astype(np.float32), np.float32(0)).astype(np.float32)
        v = ((s2 - (s1 * s1) / nd) / (nd - 1.0)) / nd
        v = np.where(v < 0, 0.0, v)
        var = np.where(n >= 2, v.astype(np.float32), np.float32(0)).astype(np.float32)
    return mean, var, n
