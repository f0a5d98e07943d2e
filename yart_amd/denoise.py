"""The edge-avoiding à-trous filter of ``yart_hip_denoise_atrous_*`` stated in NumPy float32.

:func:`atrous_reference` is written from the definition in the header comment of ``include/yart_hip.h`` (prepare pass,
iterations, finish pass), vectorised over the pixels with an explicit loop over the 25 taps, every operation a float32
operation in the order the definition gives. It is what the tests hold the device kernels (and ``csrc/denoise.hpp`` compiled
for the host) to, bit for bit — the role ``api.reduce_aov_samples`` plays for the feature buffers. ``expf`` / ``logf`` are
injectable so that a test can pass the machine's libm; NumPy's own ``exp`` / ``log`` may differ from it in the last bit.
"""
from __future__ import annotations

import numpy as np

# include/yart_hip.h: YART_DENOISE_DEFAULT_* (chosen by profiles/denoise_sigma_sweep.txt) and YART_DENOISE_DEMODULATE
DEFAULT_ITERATIONS = 5
DEFAULT_SIGMA_COLOR = 0.5
DEFAULT_SIGMA_NORMAL = 0.5
DEFAULT_SIGMA_DEPTH = 0.3
FLAG_DEMODULATE = 1
MAX_ITERATIONS = 8

_K = (np.float32(0.375), np.float32(0.25), np.float32(0.0625))
_F = np.float32


def _inv_sigma2(sigma):
    s = _F(sigma)
    return _F(1.0) / (s * s)


def atrous_reference(rgba, albedo=None, normal=None, depth=None, iterations=DEFAULT_ITERATIONS,
                     sigma_color=DEFAULT_SIGMA_COLOR, sigma_normal=DEFAULT_SIGMA_NORMAL, sigma_depth=DEFAULT_SIGMA_DEPTH,
                     demodulate=None, expf=np.exp, logf=np.log):
    """``rgba`` (H, W, 4), ``albedo`` / ``normal`` (H, W, 3) or None, ``depth`` (H, W) or None -> the filtered (H, W, 4) float32
    frame. ``demodulate``: None = whenever an albedo buffer is given. ``expf`` / ``logf``: float32 array -> float32 array of
    the same shape."""
    if demodulate is None:
        demodulate = albedo is not None
    rgba = np.asarray(rgba, _F)
    h, w = rgba.shape[:2]
    assert rgba.shape == (h, w, 4) and 0 <= iterations <= MAX_ITERATIONS
    if demodulate and albedo is None:
        raise ValueError("demodulate needs an albedo buffer")
    if iterations == 0:
        return rgba.copy()
    with np.errstate(all="ignore"):
        # -- prepare ------------------------------------------------------------------------------------------------------
        if demodulate:
            alb = np.asarray(albedo, _F).reshape(h, w, 3)
            d = np.where(alb > _F(1e-3), alb, _F(1.0)).astype(_F)
        else:
            alb, d = None, np.ones((h, w, 3), _F)
        c = (rgba[..., :3] / d).astype(_F)
        valid = np.isfinite(c).all(-1)
        if alb is not None:
            valid &= np.isfinite(alb).all(-1)
        n = lz = None
        if normal is not None:
            n = np.asarray(normal, _F).reshape(h, w, 3)
            valid &= np.isfinite(n).all(-1)
        if depth is not None:
            z = np.asarray(depth, _F).reshape(h, w)
            valid &= np.isfinite(z)
            lz = np.asarray(logf(np.where(z > _F(1e-30), z, _F(1e-30)).astype(_F)), _F).reshape(h, w)
        use_c = _F(sigma_color) > 0
        use_n = n is not None and _F(sigma_normal) > 0
        use_l = lz is not None and _F(sigma_depth) > 0
        icol = _inv_sigma2(sigma_color) if use_c else None
        inrm = _inv_sigma2(sigma_normal) if use_n else None
        idep = _inv_sigma2(sigma_depth) if use_l else None
        # -- iterations ---------------------------------------------------------------------------------------------------
        for i in range(iterations):
            s = 1 << i
            icol_i = (icol * _F(1 << (2 * i))).astype(_F) if use_c else None
            acc = np.zeros((h, w, 3), _F)
            wsum = np.zeros((h, w), _F)
            for dy in range(-2, 3):
                oy = s * dy
                py = slice(max(0, -oy), min(h, h - oy))           # the pixels p whose tap row lies inside the image
                if py.start >= py.stop:
                    continue
                qy = slice(py.start + oy, py.stop + oy)
                for dx in range(-2, 3):
                    ox = s * dx
                    px = slice(max(0, -ox), min(w, w - ox))
                    if px.start >= px.stop:
                        continue
                    qx = slice(px.start + ox, px.stop + ox)
                    hk = _K[abs(dy)] * _K[abs(dx)]
                    cp, cq = c[py, px], c[qy, qx]
                    e = None

                    def add(e, t):
                        return t if e is None else (e + t).astype(_F)
                    if use_c:
                        df = (cq - cp).astype(_F)
                        dc = ((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]).astype(_F)
                        e = add(e, (dc * icol_i).astype(_F))
                    if use_n:
                        df = (n[qy, qx] - n[py, px]).astype(_F)
                        dn = ((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]).astype(_F)
                        e = add(e, (dn * inrm).astype(_F))
                    if use_l:
                        dl = (lz[qy, qx] - lz[py, px]).astype(_F)
                        e = add(e, ((dl * dl) * idep).astype(_F))
                    if e is None:
                        e = np.zeros(cp.shape[:2], _F)
                    e = np.where(valid[py, px], e, _F(0.0)).astype(_F)
                    wt = (hk * np.asarray(expf((-e).astype(_F)), _F).reshape(e.shape)).astype(_F)
                    take = valid[qy, qx]
                    acc[py, px] = np.where(take[..., None], acc[py, px] + (wt[..., None] * cq).astype(_F), acc[py, px])
                    wsum[py, px] = np.where(take, wsum[py, px] + wt, wsum[py, px])
            c = np.where((wsum == 0)[..., None], _F(0.0), acc / wsum[..., None]).astype(_F)
        # -- finish -------------------------------------------------------------------------------------------------------
        out = np.empty((h, w, 4), _F)
        out[..., :3] = c * d
        out[..., 3] = rgba[..., 3]
    return out
