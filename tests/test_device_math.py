"""The device's math, function by function, against the libm and the IEEE arithmetic of the machine the test runs on (`-m gpu`).

Every frame test asserts bit identity with the reference; that rests on the device evaluating glibc's sinf / cosf / logf / expf /
log2f / powf algorithms (csrc/ymath.hpp `libm_emul`, csrc/libm_pow.hpp) and on IEEE-exact fp32 divide and sqrt (-ffp-contract=off
-fhip-fp32-correctly-rounded-divide-sqrt). Here each function is evaluated on the GPU through yart_hip_probe_math[_pairs]
(k_probe_math calls the inline functions the render kernels call) over its whole reachable domain, and compared bit for bit
(NaN == NaN) in C by tests/libm_ref/libm_ref.c with this machine's libm — the libm the compiled reference calls. The bar is zero
mismatches everywhere; no input is pinned.

Domains (full density unless a stride is named):
  sinf, cosf and their `2pi` forms   every float of [+0, 0x1.921fb6p+2] (2 pi rounded up), 1.09e9 inputs each; the 2pi forms also
                                     against ysinf / ycosf themselves
  sinf, cosf outside it              [2 pi, 120) and its mirror image at every 64th float, +-4096 bit patterns around 0x1p-12,
                                     0x1.921FB6p-1 and 120 (both signs), |x| >= 120 at every 4096th up to FLT_MAX, +-0, +-inf, NaN
  logf                               every float of [+0, 1]; (1, FLT_MAX] at every 64th, negative values, +-inf, NaN
  expf                               every float with 0x1p-40 <= |x| <= 104, both signs; +-0, denormals, |x| > 104 at every
                                     4096th, +-inf, NaN
  log2f                              (0, FLT_MAX] at every 16th, windows around FLT_MIN, 0x1.66p-1 and 1, +-0, negative, inf, NaN
  powf(x, y), y of csrc/tonemap.hpp  every float x of [0x1p-20, 0x1p+8]; the whole line (negative, inf, NaN too) at every 256th
  a / b, sqrtf, reverseBits32        2^22 random pairs, an edge table, 1 / x over the binade [1, 2), sqrtf over [1, 4) and over
                                     every denormal, x / 255 for x = 0..255; 2^20 random words and the one-bit words

Measured on the MI355X machine (8 checker threads), seconds per test: sin / cos [0, 2 pi] 0.10-0.27 per quarter (2.7e8 inputs),
the 2pi forms 0.15-0.18 per quarter (two device functions each), logf 0.11-0.15 per quarter, expf 0.07-0.08 per half, log2f 0.24,
powf 0.17-0.19 per exponent, divide 0.05, sqrt 0.03, everything else under 0.05; the 38 tests together 5.1 s. The
estimate had been 1-3 s per test; the parts are kept so that a slower host's libm still leaves each test at a few seconds."""
import time

import numpy as np
import pytest

from tests.libmref import LibmRef, describe, f32_bits

pytestmark = pytest.mark.gpu

H = float.fromhex
CHUNK = 1 << 26                      # inputs per probe call: 256 MB of results
TWO_PI_UP = H("0x1.921fb6p+2")            # float(2 pi) rounded up: every caller passes 2 pi u or side / sides * 2 pi (integrator.hpp, bsdf.hpp)
FLT_MAX_BITS, FLT_MIN_BITS, INF_BITS, SIGN = 0x7f7fffff, 0x00800000, 0x7f800000, 0x80000000
SPECIALS = np.array([0, SIGN, INF_BITS, SIGN | INF_BITS, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 1, SIGN | 1, 0x007fffff,
                     SIGN | 0x007fffff, FLT_MIN_BITS, SIGN | FLT_MIN_BITS, FLT_MAX_BITS, SIGN | FLT_MAX_BITS], np.uint32)
TONEMAP_EXPONENTS = (1.0, 0.8, 1.35, 2.2, 1.0 / 2.2)   # csrc/tonemap.hpp: agxLook powers (none, golden, punchy), the 2.2 and 1 / 2.2 gammas


@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return LibmRef(tmp_path_factory.mktemp("libm_ref"))


@pytest.fixture(scope="module")
def buffers():
    return np.empty(CHUNK, np.uint32), np.empty(CHUNK, np.uint32)


class Tally:
    def __init__(self, tag):
        self.tag, self.inputs, self.bad, self.first, self.t0 = tag, 0, 0, [], time.perf_counter()

    def add(self, n, bad, first, fn):
        self.inputs += n
        self.bad += bad
        if first and len(self.first) < 16:
            self.first.append(describe(fn, first))

    def finish(self):
        print(f"{self.tag}: inputs={self.inputs} mismatches={self.bad} seconds={time.perf_counter() - self.t0:.2f}")
        assert self.bad == 0, f"{self.tag}: {self.bad} of {self.inputs} device results differ from this machine's libm\n" + "\n".join(self.first)


def sweep_range(api, ref, buffers, tally, fn, lo, hi, y=0.0, equal_to=None):
    """fn at every bit pattern of [lo, hi] against libm; with equal_to also against that device function, bit for bit."""
    out, other = buffers
    for first in range(lo, hi + 1, CHUNK):
        n = min(CHUNK, hi + 1 - first)
        api.probe_math(fn, first, n, y=y, out=out[:n])
        tally.add(n, *ref.check(fn, out[:n], first_bits=first, count=n, y=y), fn)
        if equal_to is not None:
            api.probe_math(equal_to, first, n, y=y, out=other[:n])
            tally.add(n, *ref.check("copy", out[:n], a=other[:n]), f"{fn} vs {equal_to}: copy")


def sweep_values(api, ref, tally, fn, a, b=None):
    """fn at explicit operands (uint32 bit patterns) against libm, in chunks."""
    a = np.ascontiguousarray(a, np.uint32)
    for i in range(0, a.size, CHUNK):
        ca = a[i:i + CHUNK]
        cb = None if b is None else np.ascontiguousarray(b[i:i + CHUNK], np.uint32)
        got = api.probe_math(fn, a=ca, b=cb)
        tally.add(ca.size, *ref.check(fn, got, a=ca, b=cb), fn)


def strided(lo, hi, stride, both_signs=False):
    """lo, lo + stride, ... and hi itself, as bit patterns; with both_signs the same with the sign bit set, too."""
    v = np.append(np.arange(lo, hi, stride, dtype=np.uint32), np.uint32(hi))
    return np.concatenate([v, v | np.uint32(SIGN)]) if both_signs else v


def window(x, both_signs=True):
    c = f32_bits(x)
    return strided(c - 4096, c + 4096, 1, both_signs)


def part_of(lo, hi, part, parts):
    """[lo, hi] cut into `parts` contiguous pieces: the bounds of piece `part`."""
    n = hi + 1 - lo
    return lo + n * part // parts, lo + n * (part + 1) // parts - 1


# ------------------------------------------------------------------------------------------------------------- sin / cos
@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("fn", ["sinf", "cosf"])
def test_sincos_reachable_domain(gpu_api, ref, buffers, fn, part):
    """ysinf / ycosf over every float of [+0, 2 pi]: the three branches (|x| < 2^-12, < pi / 4, reduced) and every quadrant."""
    t = Tally(f"{fn} [0, 2pi] part {part}/4")
    sweep_range(gpu_api, ref, buffers, t, fn, *part_of(0, f32_bits(TWO_PI_UP), part, 4))
    t.finish()


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("fn", ["sinf2pi", "cosf2pi"])
def test_sincos_2pi_forms_reachable_domain(gpu_api, ref, buffers, fn, part):
    """The shortened forms the BSDF samplers call, over the same range: equal to libm, and to ysinf / ycosf bit for bit."""
    t = Tally(f"{fn} [0, 2pi] part {part}/4")
    sweep_range(gpu_api, ref, buffers, t, fn, *part_of(0, f32_bits(TWO_PI_UP), part, 4), equal_to=fn[:4])
    t.finish()


@pytest.mark.parametrize("fn", ["sinf", "cosf"])
def test_sincos_outside_reachable_domain(gpu_api, ref, fn):
    """[2 pi, 120) and its mirror image, the windows around the branch constants, and the |x| >= 120 tail (glibc's reduce_large in
    integers, csrc/ymath.hpp reduceLarge) with +-0, +-inf and NaN. No caller reaches the tail; it agrees all the same."""
    t = Tally(f"{fn} [2pi, 120) both signs, every 64th")
    sweep_values(gpu_api, ref, t, fn, strided(f32_bits(TWO_PI_UP), f32_bits(120.0) - 1, 64, True))
    sweep_values(gpu_api, ref, t, fn, strided(1, f32_bits(TWO_PI_UP), 64) | np.uint32(SIGN))          # [-2 pi, -0)
    t.finish()
    t = Tally(f"{fn} windows around 0x1p-12, 0x1.921FB6p-1, 120")
    for c in (H("0x1p-12"), H("0x1.921FB6p-1"), 120.0):
        sweep_values(gpu_api, ref, t, fn, window(c))
    t.finish()
    t = Tally(f"{fn} |x| >= 120 tail, every 4096th, and the special values")
    sweep_values(gpu_api, ref, t, fn, strided(f32_bits(120.0), FLT_MAX_BITS, 4096, True))
    sweep_values(gpu_api, ref, t, fn, SPECIALS)
    t.finish()


# ------------------------------------------------------------------------------------------------------------------- log
@pytest.mark.parametrize("part", range(4))
def test_logf_unit_interval(gpu_api, ref, buffers, part):
    """ylogf over every float of [+0, 1] (sampler values, sampler.hpp: clamped to kOneMinusEpsilon): +0 -> -inf, the denormal
    branch, the x == 1 early return."""
    t = Tally(f"logf [0, 1] part {part}/4")
    sweep_range(gpu_api, ref, buffers, t, "logf", *part_of(0, f32_bits(1.0), part, 4))
    t.finish()


def test_logf_outside_unit_interval(gpu_api, ref):
    t = Tally("logf (1, FLT_MAX] every 64th, negative values, specials")
    sweep_values(gpu_api, ref, t, "logf", strided(f32_bits(1.0) + 1, FLT_MAX_BITS, 64))
    sweep_values(gpu_api, ref, t, "logf", strided(SIGN, SIGN | INF_BITS, 4096))
    sweep_values(gpu_api, ref, t, "logf", SPECIALS)
    t.finish()


# ------------------------------------------------------------------------------------------------------------------- exp
# the two inputs for which the emulation, before r = fma(InvLn2N, x, -kd) (csrc/ymath.hpp expf_), was one ulp below libm:
# (input bits, libm bits). They are asserted like every other input; named here so that a regression is recognised.
EXP_FORMERLY_WRONG = ((0x4202422f, 0x56fc9f1c), (0xc27c65d9, 0x11fa2993))


@pytest.mark.parametrize("part", range(2))
@pytest.mark.parametrize("sign", ["positive", "negative"])
def test_expf_dense(gpu_api, ref, buffers, sign, part):
    """yexpf over every float with 0x1p-40 <= |x| <= 104: across glibc's |x| >= 88 special-casing, its overflow (x > 0x1.62e42ep6)
    and underflow (x < -0x1.9fe368p6) thresholds and the subnormal results between them (matAttenuation can produce any of these)."""
    s = SIGN if sign == "negative" else 0
    lo, hi = part_of(f32_bits(H("0x1p-40")), f32_bits(104.0), part, 2)
    t = Tally(f"expf {sign} 2^-40 <= |x| <= 104 part {part}/2")
    sweep_range(gpu_api, ref, buffers, t, "expf", s | lo, s | hi)
    t.finish()


def test_expf_special_values(gpu_api, ref):
    t = Tally("expf +-0, denormals, |x| < 2^-40, |x| > 104 every 4096th, inf, NaN, the two formerly wrong inputs")
    sweep_values(gpu_api, ref, t, "expf", strided(0, FLT_MIN_BITS, 64, True))
    sweep_values(gpu_api, ref, t, "expf", strided(FLT_MIN_BITS, f32_bits(H("0x1p-40")), 4096, True))
    sweep_values(gpu_api, ref, t, "expf", strided(f32_bits(104.0), FLT_MAX_BITS, 4096, True))
    sweep_values(gpu_api, ref, t, "expf", SPECIALS)
    t.finish()
    xs = np.array([x for x, _ in EXP_FORMERLY_WRONG], np.uint32)
    want = np.array([r for _, r in EXP_FORMERLY_WRONG], np.uint32)
    np.testing.assert_array_equal(ref.eval("expf", xs), want, "this machine's libm gives other values than recorded for the two inputs")
    np.testing.assert_array_equal(gpu_api.probe_math("expf", a=xs), want)


# ------------------------------------------------------------------------------------------------------------ log2 / pow
def test_log2f(gpu_api, ref):
    t = Tally("log2f (0, FLT_MAX] every 16th, windows, specials")
    sweep_values(gpu_api, ref, t, "log2f", strided(1, FLT_MAX_BITS, 16))
    for c in (1.0, H("0x1.66p-1"), H("0x1p-126")):          # the early return, the table's origin (OFF = 0x3f330000), the denormal branch
        sweep_values(gpu_api, ref, t, "log2f", window(c))
    sweep_values(gpu_api, ref, t, "log2f", strided(0, 4096, 1, True))
    sweep_values(gpu_api, ref, t, "log2f", strided(SIGN, SIGN | INF_BITS, 4096))
    sweep_values(gpu_api, ref, t, "log2f", SPECIALS)
    t.finish()


@pytest.mark.parametrize("y", TONEMAP_EXPONENTS, ids=lambda y: f"y={np.float32(y)}")
def test_powf_tonemap_exponents(gpu_api, ref, buffers, y):
    """ypowf(x, y) for the exponents of the tonemap stage: every float x of [2^-20, 2^8], the whole line at every 256th."""
    t = Tally(f"powf(x, {np.float32(y)}) x in [2^-20, 2^8]")
    sweep_range(gpu_api, ref, buffers, t, "powf", f32_bits(H("0x1p-20")), f32_bits(H("0x1p+8")), y=y)
    t.finish()
    t = Tally(f"powf(x, {np.float32(y)}) every 256th float of the line, specials")
    line = strided(0, 0xffffffff, 256)
    sweep_values(gpu_api, ref, t, "powf", line, np.full(line.size, f32_bits(y), np.uint32))
    sweep_values(gpu_api, ref, t, "powf", SPECIALS, np.full(SPECIALS.size, f32_bits(y), np.uint32))
    t.finish()


# ------------------------------------------------------------------------------------------- divide, sqrt, bit reversal
def _edge_pairs():
    """Operand pairs for a / b: specials in either slot, denormal operands, quotients in the denormal range and within an ulp
    of FLT_MIN and FLT_MAX, x / 255."""
    rng = np.random.default_rng(20250)
    vals = np.concatenate([SPECIALS, np.array([f32_bits(v) for v in (1.0, -1.0, 1.5, 3.0, 255.0, H("0x1p-75"), H("0x1p+100"), H("0x1.fffffep-1"))], np.uint32),
                           rng.integers(1, FLT_MIN_BITS, 16, dtype=np.uint32)])                       # ... and 16 denormals
    a, b = [np.repeat(vals, vals.size)], [np.tile(vals, vals.size)]
    # denormal operands against anything; quotients that land in the denormal range: a in [2^-126, 2^-100), b in [2, 2^40)
    n = 1 << 16
    den = rng.integers(1, FLT_MIN_BITS, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << 31)
    anyv = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    a += [den, anyv]; b += [anyv, den]
    small = (rng.integers(1, 27, n, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    big = (rng.integers(128, 167, n, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    a.append(small); b.append(big)
    # quotients within an ulp of FLT_MIN / FLT_MAX: a = float(limit * b) and its neighbours
    for limit, blo, bhi in ((float(np.float32(2.0 ** -126)), 1.0, 2.0 ** 20), (float(np.finfo(np.float32).max), 2.0 ** -20, 1.0)):
        bb = rng.uniform(blo, bhi, 4096).astype(np.float32)
        aa = (bb.astype(np.float64) * limit).astype(np.float32).view(np.uint32)
        for d in (-2, -1, 0, 1, 2):
            a.append((aa.astype(np.int64) + d).astype(np.uint32)); b.append(bb.view(np.uint32))
    a.append(np.arange(256, dtype=np.float32).view(np.uint32)); b.append(np.full(256, f32_bits(255.0), np.uint32))
    return np.concatenate(a), np.concatenate(b)


def test_fp32_divide(gpu_api, ref):
    """a / b as the kernels are compiled, against the CPU's IEEE divide: a flushed denormal or a one-ulp quotient is a failure."""
    rng = np.random.default_rng(1)
    t = Tally("a / b: 2^22 random pairs + edge table")
    sweep_values(gpu_api, ref, t, "div", rng.integers(0, 2 ** 32, 1 << 22, dtype=np.uint32), rng.integers(0, 2 ** 32, 1 << 22, dtype=np.uint32))
    a, b = _edge_pairs()
    q = ref.eval("div", a, b)
    assert ((q & 0x7f800000) == 0).sum() > 60000 and (q == FLT_MIN_BITS).any() and (q == FLT_MAX_BITS).any() and (q == INF_BITS).any()
    sweep_values(gpu_api, ref, t, "div", a, b)
    t.finish()
    t = Tally("1 / x, every float of [1, 2)")
    x = np.arange(f32_bits(1.0), f32_bits(2.0), dtype=np.uint32)
    sweep_values(gpu_api, ref, t, "div", np.full(x.size, f32_bits(1.0), np.uint32), x)
    t.finish()


def test_fp32_sqrt(gpu_api, ref, buffers):
    rng = np.random.default_rng(2)
    t = Tally("sqrtf: every float of [1, 4), every denormal, 2^22 random words, specials")
    sweep_range(gpu_api, ref, buffers, t, "sqrt", f32_bits(1.0), f32_bits(4.0) - 1)
    sweep_range(gpu_api, ref, buffers, t, "sqrt", 0, FLT_MIN_BITS + 4096)      # (no root is denormal: the denormal operands instead)
    sweep_values(gpu_api, ref, t, "sqrt", rng.integers(0, 2 ** 32, 1 << 22, dtype=np.uint32))
    sweep_values(gpu_api, ref, t, "sqrt", SPECIALS)
    t.finish()


def test_reverse_bits(gpu_api, ref):
    """reverseBits32 on the device (__brev) against the host's bit-trick form."""
    rng = np.random.default_rng(3)
    one = np.uint32(1) << np.arange(32, dtype=np.uint32)
    t = Tally("reverseBits32: 2^20 random words, one-bit and all-but-one-bit words")
    sweep_values(gpu_api, ref, t, "brev", np.concatenate([rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint32), one, ~one,
                                                         np.array([0, 0xffffffff], np.uint32)]))
    t.finish()


def test_probe_math_rejects_bad_arguments(gpu_api):
    import ctypes
    L = gpu_api.lib()
    out = (ctypes.c_float * 4)()
    assert L.yart_hip_probe_math(99, 0, 4, 0.0, out) == gpu_api.YART_E_INVALID
    assert L.yart_hip_probe_math(0, 0, 0, 0.0, out) == gpu_api.YART_E_INVALID
    assert L.yart_hip_probe_math(0, 0, 4, 0.0, None) == gpu_api.YART_E_INVALID
    assert L.yart_hip_probe_math(0, 0xfffffffe, 4, 0.0, out) == gpu_api.YART_E_INVALID          # runs past the last bit pattern
    assert L.yart_hip_probe_math(gpu_api.MATH_FNS["div"], 0, 4, 0.0, out) == gpu_api.YART_E_INVALID
    assert L.yart_hip_probe_math_pairs(0, 4, None, None, out) == gpu_api.YART_E_INVALID
    assert L.yart_hip_probe_math_pairs(gpu_api.MATH_FNS["div"], 4, out, None, out) == gpu_api.YART_E_INVALID
    assert L.yart_hip_probe_math(0, 0, 4, 0.0, out) == gpu_api.YART_OK
