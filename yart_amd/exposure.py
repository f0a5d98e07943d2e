"""Auto-exposure (``yart_hip_exposure_*``) stated in NumPy float32.

:func:`exposure_reference` (meter, resolve, state step) and :func:`apply_reference` (gain, AgX, 8-bit encoding) are written from
the definition in the header comment of ``include/yart_hip.h``, every operation a float32 operation in the order the definition
gives (the resolve's sum in Python floats, which are binary64). They are what the tests hold the device kernels and
``csrc/exposure.hpp`` compiled for the host to, bit for bit. ``log2f`` / ``expf`` / ``powf`` are injectable so that a test can
pass the machine's libm; NumPy's own may differ from it in the last bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

_F = np.float32
BINS = 256
FLAG_EMPTY = 1
# include/yart_hip.h: YART_EXPOSURE_DEFAULT_* — conventions, not tuned
DEFAULTS = dict(ev_min=-16.0, ev_max=16.0, trim_low=0.10, trim_high=0.10, key=0.18, compensation_ev=0.0, gain_ev_min=-16.0,
                gain_ev_max=16.0, speed_up=3.0, speed_down=1.0, window=None)
LOOKS = {"none": 0, "golden": 1, "punchy": 2}


def look_index(look) -> int:
    """None -> -1 (no tonemapper), a name of LOOKS or the index itself."""
    if look is None:
        return -1
    return LOOKS[look] if isinstance(look, str) else int(look)


def params_of(**over) -> dict:
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, f"exposure: unknown parameters {sorted(unknown)}"
    return dict(DEFAULTS, **over)


@dataclass
class ExposureState:
    """YartExposureState and the record's ``valid``: a new handle's."""
    cur_ev: np.float32 = _F(0.0)
    target_ev: np.float32 = _F(0.0)
    mean_ev: np.float32 = _F(0.0)
    gain: np.float32 = _F(1.0)
    n_counted: int = 0
    n_ignored: int = 0
    frames: int = 0
    flags: int = 0
    valid: bool = False

    def asdict(self):
        return dict(cur_ev=self.cur_ev, target_ev=self.target_ev, mean_ev=self.mean_ev, gain=self.gain, n_counted=self.n_counted,
                    n_ignored=self.n_ignored, frames=self.frames, flags=self.flags)


def _scalar(fn, x):
    return _F(np.asarray(fn(np.asarray([x], _F)), _F).reshape(-1)[0])


def window_of(params, w, h):
    win = params.get("window")
    if win is None or tuple(win) == (0, 0, 0, 0):
        return 0, 0, w, h
    x0, y0, x1, y1 = (int(v) for v in win)
    assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h, "exposure: the metering window is empty or outside the frame"
    return x0, y0, x1, y1


def histogram_reference(frame, params, log2f=np.log2):
    """Meter: (hist uint32[256], n_ignored, bins (h, w) of the window with 256 for an ignored pixel)."""
    frame = np.asarray(frame, _F)
    h, w = frame.shape[:2]
    x0, y0, x1, y1 = window_of(params, w, h)
    px = frame[y0:y1, x0:x1]
    ev_min, ev_max = _F(params["ev_min"]), _F(params["ev_max"])
    bins_per_ev = _F(256.0) / (ev_max - ev_min)
    with np.errstate(all="ignore"):
        r, g, b = px[..., 0], px[..., 1], px[..., 2]
        Y = ((_F(0.2126) * r + _F(0.7152) * g) + _F(0.0722) * b).astype(_F)
        counted = np.isfinite(r) & np.isfinite(g) & np.isfinite(b) & (Y > 0)
        ev = np.asarray(log2f(np.where(counted, Y, _F(1.0)).astype(_F)), _F).reshape(Y.shape)
        t = ((ev - ev_min) * bins_per_ev).astype(_F)
        bins = np.where(t < 0, 0, np.where(t >= _F(256.0), 255, np.clip(t, 0, 255).astype(np.uint32))).astype(np.uint32)
    bins = np.where(counted, bins, BINS).astype(np.uint32)
    hist = np.bincount(bins.reshape(-1), minlength=BINS + 1).astype(np.uint32)
    return hist[:BINS].copy(), int(hist[BINS]), bins


def resolve_reference(hist, params):
    """Resolve: (N, K, S, mean_ev) of a histogram; mean_ev is None when N == 0. k_b of every bin is returned as a list."""
    N = int(np.asarray(hist, np.uint64).sum())
    lo = int(math.floor(float(_F(params["trim_low"])) * float(N)))
    hi = N - int(math.floor(float(_F(params["trim_high"])) * float(N)))
    ev_min, ev_max = _F(params["ev_min"]), _F(params["ev_max"])
    bin_width = (ev_max - ev_min) / _F(256.0)
    S, c, ks = 0.0, 0, []
    for b in range(BINS):
        n = int(hist[b])
        kb = max(0, min(c + n, hi) - max(c, lo))
        centre = ev_min + (_F(b) + _F(0.5)) * bin_width
        assert centre.dtype == _F
        S += float(kb) * float(centre)
        c += n
        ks.append(kb)
    K = hi - lo
    mean = _F(S / float(K)) if N else None
    return N, K, S, mean, ks


def exposure_reference(state: ExposureState, frame, params, dt, log2f=np.log2, expf=np.exp):
    """One meter call on ``state`` (changed in place): ``frame`` (H, W, 4) float32, ``params`` a dict as ``params_of`` makes it,
    ``dt`` seconds. ``log2f`` / ``expf``: float32 array -> float32 array of the same shape. Returns the call's histogram."""
    hist, ignored, _ = histogram_reference(frame, params, log2f)
    N, K, S, mean, _ = resolve_reference(hist, params)
    state.n_counted, state.n_ignored = N, ignored
    if N == 0:
        state.flags = FLAG_EMPTY
        return hist
    with np.errstate(all="ignore"):
        key_ev = _scalar(log2f, params["key"])
        dt = _F(dt)
        a_up = _F(1.0) - _scalar(expf, -(dt * _F(params["speed_up"])))
        a_down = _F(1.0) - _scalar(expf, -(dt * _F(params["speed_down"])))
        want = (key_ev - mean) + _F(params["compensation_ev"])
        lo, hi = _F(params["gain_ev_min"]), _F(params["gain_ev_max"])
        t = lo if lo > want else want                      # max(gain_ev_min, want)
        target = hi if hi < t else t                       # min(gain_ev_max, ...)
        if not state.valid:
            state.cur_ev, state.valid = target, True
        else:
            d = target - state.cur_ev
            state.cur_ev = state.cur_ev + d * (a_up if d > 0 else a_down)
        assert state.cur_ev.dtype == _F
        state.mean_ev, state.target_ev = mean, target
        state.gain = _scalar(expf, state.cur_ev * _F(0.6931472))
    state.frames += 1
    state.flags = 0
    return hist


# csrc/tonemap.hpp, expression by expression
_AGX = [_F(v) for v in (0.842479062253094, 0.0784335999999992, 0.0792237451477643, 0.0423282422610123, 0.878468636469772,
                        0.0791661274605434, 0.0423756549057051, 0.0784336, 0.879142973793104)]
_INV = [_F(v) for v in (1.19687900512017, -0.0980208811401368, -0.0990297440797205, -0.0528968517574562, 1.15190312990417,
                        -0.0989611768448433, -0.0529716355144438, -0.0980434501171241, 1.15107367264116)]
_LOOK = {0: ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.0), 1: ((1.0, 0.9, 0.5), (0.8, 0.8, 0.8), 0.8), 2: ((1.0, 1.0, 1.0), (1.35, 1.35, 1.35), 1.4)}


def _mul3x3(m, v):
    return [((_F(0.0) + m[3 * i] * v[0]) + m[3 * i + 1] * v[1]) + m[3 * i + 2] * v[2] for i in range(3)]


def agx_reference(c, look, log2f=np.log2, powf=np.power):
    """AgX (csrc/tonemap.hpp agxTonemap) of three float32 channel arrays -> three float32 channel arrays."""
    slope, power, sat = _LOOK[look]
    lo, hi = _F(-12.47393), _F(4.026069)
    f = lambda a: np.asarray(a, _F)
    val = _mul3x3(_AGX, c)
    out = []
    for v in val:
        l = f(log2f(f(v))).reshape(v.shape)
        l = np.where(lo > l, lo, l)
        l = np.where(hi < l, hi, l)
        out.append(f(f(l - lo) / (hi - lo)))
    val = []
    for x in out:                                           # agxContrast
        x2 = x * x
        x4 = x2 * x2
        val.append((((((((x4 * _F(15.5)) * x2) - ((x4 * _F(40.14)) * x)) + (x4 * _F(31.96))) - ((x2 * _F(6.868)) * x)) + (x2 * _F(0.4298))) +
                    (x * _F(0.1191))) - _F(0.00232))
    luma = (val[0] * _F(0.2126) + val[1] * _F(0.7152)) + val[2] * _F(0.0722)
    graded = []
    for i in range(3):
        b = val[i] * _F(slope[i]) + _F(0.0)
        p = f(powf(f(b), np.full(b.shape, power[i], _F))).reshape(b.shape)
        graded.append(luma + _F(sat) * (p - luma))
    val = _mul3x3(_INV, graded)
    res = []
    for v in val:
        v = np.where(_F(0.0) > v, _F(0.0), v)
        v = np.where(_F(1.0) < v, _F(1.0), v)
        res.append(f(powf(f(v), np.full(v.shape, 2.2, _F))).reshape(v.shape))
    assert all(r.dtype == _F for r in res)
    return res


def ppm_byte_reference(v, powf=np.power):
    """csrc/tonemap.hpp ppmByte of a float32 array -> uint8."""
    v = np.asarray(v, _F)
    gamma = _F(1.0) / _F(2.2)
    m = np.asarray(powf(v, np.full(v.shape, gamma, _F)), _F).reshape(v.shape)
    m = np.where(m < 0, _F(0.0), np.where(_F(1.0) < m, _F(1.0), m)).astype(_F)
    scaled = (m * _F(255.999)).astype(_F)
    return np.where(np.isnan(m), 0, np.nan_to_num(scaled).astype(np.uint8)).astype(np.uint8)


def apply_reference(frame, gain, look, log2f=np.log2, powf=np.power):
    """Apply: ``frame`` (H, W, 4) float32, ``gain`` the state's, ``look`` None / a name / -1 .. 2 -> (ldr (H, W, 4) float32,
    rgb8 (H, W, 3) uint8). ``powf``: two float32 arrays -> float32 array."""
    frame = np.asarray(frame, _F)
    look = look_index(look)
    gain = _F(gain)
    with np.errstate(all="ignore"):
        c = [(frame[..., i] * gain).astype(_F) for i in range(3)]
        ldr = np.empty_like(frame)
        if look >= 0:
            m = agx_reference(c, look, log2f, powf)
            ldr[..., 3] = _F(1.0)
        else:
            m = c
            ldr[..., 3] = frame[..., 3]
        for i in range(3):
            ldr[..., i] = m[i]
        rgb8 = np.stack([ppm_byte_reference(ldr[..., i], powf) for i in range(3)], axis=-1)
    return ldr, rgb8
