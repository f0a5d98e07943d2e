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


# include/yart_hip.h: YART_DENOISE_VAR_DEFAULT_* (chosen by profiles/denoise_var_sweep.txt)
DEFAULT_VAR_ITERATIONS = 3
DEFAULT_VAR_SIGMA_LUMA = 2.0
DEFAULT_VAR_SIGMA_NORMAL = 0.25
DEFAULT_VAR_SIGMA_DEPTH = 0.1

_K3 = (np.float32(0.5), np.float32(0.25))
_LUMA = (np.float32(0.2126), np.float32(0.7152), np.float32(0.0722))


def _luma(c):
    return ((c[..., 0] * _LUMA[0] + c[..., 1] * _LUMA[1]).astype(_F) + c[..., 2] * _LUMA[2]).astype(_F)


def _taps(h, w, oy, ox):
    """Slices (py, px, qy, qx): the pixels p whose tap q = p + (ox, oy) lies inside the image; None if there are none."""
    py = slice(max(0, -oy), min(h, h - oy))
    px = slice(max(0, -ox), min(w, w - ox))
    if py.start >= py.stop or px.start >= px.stop:
        return None
    return py, px, slice(py.start + oy, py.stop + oy), slice(px.start + ox, px.stop + ox)


def atrous_var_reference(rgba, variance, albedo=None, normal=None, depth=None, iterations=DEFAULT_VAR_ITERATIONS,
                         sigma_luma=DEFAULT_VAR_SIGMA_LUMA, sigma_normal=DEFAULT_VAR_SIGMA_NORMAL,
                         sigma_depth=DEFAULT_VAR_SIGMA_DEPTH, demodulate=None, expf=np.exp, logf=np.log):
    """The variance-guided form (``yart_hip_denoise_atrous_var_*``), written from its definition in ``include/yart_hip.h``:
    :func:`atrous_reference` with ``variance`` (H, W) — the variance of each pixel's mean luminance, ``render_moments`` — as a
    fourth input. The colour term of a tap is |luma difference| over sigma_luma times the local standard deviation (3 x 3
    Gaussian of the variance), and the variance is filtered along with the colour. Returns the filtered (H, W, 4) frame."""
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
        var = np.asarray(variance, _F).reshape(h, w)
        valid = np.isfinite(c).all(-1) & np.isfinite(var) & (var >= 0)
        if alb is not None:
            valid &= np.isfinite(alb).all(-1)
        ld = _luma(d)
        v = (var / (ld * ld).astype(_F)).astype(_F)
        n = lz = None
        if normal is not None:
            n = np.asarray(normal, _F).reshape(h, w, 3)
            valid &= np.isfinite(n).all(-1)
        if depth is not None:
            z = np.asarray(depth, _F).reshape(h, w)
            valid &= np.isfinite(z)
            lz = np.asarray(logf(np.where(z > _F(1e-30), z, _F(1e-30)).astype(_F)), _F).reshape(h, w)
        use_c = _F(sigma_luma) > 0
        use_n = n is not None and _F(sigma_normal) > 0
        use_l = lz is not None and _F(sigma_depth) > 0
        inrm = _inv_sigma2(sigma_normal) if use_n else None
        idep = _inv_sigma2(sigma_depth) if use_l else None
        # -- iterations ---------------------------------------------------------------------------------------------------
        for i in range(iterations):
            s = 1 << i
            den = ly = None
            if use_c:
                gv = np.zeros((h, w), _F)
                gk = np.zeros((h, w), _F)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        t = _taps(h, w, dy, dx)
                        if t is None:
                            continue
                        py, px, qy, qx = t
                        kk = _K3[abs(dy)] * _K3[abs(dx)]
                        take = valid[qy, qx]
                        gv[py, px] = np.where(take, gv[py, px] + (kk * v[qy, qx]).astype(_F), gv[py, px])
                        gk[py, px] = np.where(take, gk[py, px] + kk, gk[py, px])
                g = np.where(gk == 0, _F(0.0), gv / gk).astype(_F)
                den = ((_F(sigma_luma) * np.sqrt(g).astype(_F)).astype(_F) + _F(1e-6)).astype(_F)
                ly = _luma(c)
            acc = np.zeros((h, w, 3), _F)
            wsum = np.zeros((h, w), _F)
            vacc = np.zeros((h, w), _F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    t = _taps(h, w, s * dy, s * dx)
                    if t is None:
                        continue
                    py, px, qy, qx = t
                    hk = _K[abs(dy)] * _K[abs(dx)]
                    cq = c[qy, qx]
                    e = None

                    def add(e, t):
                        return t if e is None else (e + t).astype(_F)
                    if use_c:
                        e = add(e, (np.abs((ly[qy, qx] - ly[py, px]).astype(_F)) / den[py, px]).astype(_F))
                    if use_n:
                        df = (n[qy, qx] - n[py, px]).astype(_F)
                        dn = ((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]).astype(_F)
                        e = add(e, (dn * inrm).astype(_F))
                    if use_l:
                        dl = (lz[qy, qx] - lz[py, px]).astype(_F)
                        e = add(e, ((dl * dl) * idep).astype(_F))
                    if e is None:
                        e = np.zeros(cq.shape[:2], _F)
                    e = np.where(valid[py, px], e, _F(0.0)).astype(_F)
                    wt = (hk * np.asarray(expf((-e).astype(_F)), _F).reshape(e.shape)).astype(_F)
                    take = valid[qy, qx]
                    acc[py, px] = np.where(take[..., None], acc[py, px] + (wt[..., None] * cq).astype(_F), acc[py, px])
                    wsum[py, px] = np.where(take, wsum[py, px] + wt, wsum[py, px])
                    vacc[py, px] = np.where(take, vacc[py, px] + ((wt * wt).astype(_F) * v[qy, qx]).astype(_F), vacc[py, px])
            c = np.where((wsum == 0)[..., None], _F(0.0), acc / wsum[..., None]).astype(_F)
            v = np.where(wsum == 0, _F(0.0), vacc / (wsum * wsum).astype(_F)).astype(_F)
        # -- finish -------------------------------------------------------------------------------------------------------
        out = np.empty((h, w, 4), _F)
        out[..., :3] = c * d
        out[..., 3] = rgba[..., 3]
    return out
