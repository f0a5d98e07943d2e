"""The device's libm emulation on the host, and the checker the GPU sweeps rely on (no GPU needed).

csrc/ymath.hpp `libm_emul` (glibc 2.35's sinf / cosf / logf / expf algorithms as the kernels evaluate them) compiles for the host
too; `hostsim libm` runs it against this machine's libm over the domains tests/test_device_math.py sweeps on the GPU — at a stride,
with the windows around every branch constant and the special values at full density. tests/libm_ref/libm_ref.c is the reference
and the comparison of those GPU sweeps; its comparison is tested here on buffers with planted differences."""
import json
import subprocess

import numpy as np
import pytest

from tests.libmref import LibmRef, f32_bits


def test_libm_emulation_equals_this_machines_libm(hostsim):
    """Zero differences, bit for bit (NaN == NaN). A failure here names the inputs; it also is the first sign of a machine whose glibc
    selects other libm variants (the YART_ALLOW_LIBM_DRIFT scenario of tests/conftest.py), before any frame test runs."""
    r = subprocess.run([hostsim, "libm"], capture_output=True, text=True)
    assert r.returncode == 0, ("the device's libm emulation (csrc/ymath.hpp) differs from this machine's libm — an edit of the emulation, or "
                               "a glibc that selects other libm variants (then no frame can be bit-identical here; YART_ALLOW_LIBM_DRIFT=1 "
                               "relaxes the frame tests):\n" + r.stderr)
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["libm"] == "ok" and info["checked"] > 10_000_000


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return LibmRef(tmp_path_factory.mktemp("libm_ref"))


def test_comparison_reports_exactly_the_planted_differences(ref):
    """A flipped low bit, a NaN against a number and +0 against -0 count; two different NaNs do not. Array form (8 threads)."""
    n = 200_000
    assert ref.threads(n) == 8 and ref.threads(100) == 1 and ref.threads(1 << 40) == 8
    rng = np.random.default_rng(7)
    a = rng.integers(0, 0x7f800000, n, dtype=np.uint32)         # finite, non-negative values
    a[150_000] = 0x00000000
    a[199_999] = 0x7fc00000
    dev = a.copy()
    dev[17] ^= 1                                                 # one flipped low bit
    dev[70_001] = 0x7fc00000                                     # a NaN against a number
    dev[150_000] = 0x80000000                                    # -0 against +0
    dev[199_999] = 0x7f800001                                    # another NaN against a NaN: equal
    bad, first = ref.check("copy", dev, a=a)
    assert bad == 3
    assert first == [(int(a[17]), 0, int(a[17]) ^ 1, int(a[17])), (int(a[70_001]), 0, 0x7fc00000, int(a[70_001])),
                     (0, 0, 0x80000000, 0)]
    assert ref.check("copy", a, a=a) == (0, [])


def test_comparison_range_form_and_report_cap(ref):
    """Range form against a real libm call; more than 64 differences: the count is exact, the list is the first 64 in input order."""
    first_bits, n = f32_bits(0.5), 300_000
    xs = np.arange(first_bits, first_bits + n, dtype=np.uint32)
    want = ref.eval("sinf", xs)
    # it is the sine: libm's sinf is within one ulp of the correctly rounded value (not always equal to it)
    exact = np.sin(xs.view(np.float32).astype(np.float64)).astype(np.float32).view(np.uint32)
    assert np.abs(want.astype(np.int64) - exact.astype(np.int64)).max() <= 1
    assert ref.check("sinf", want, first_bits=first_bits, count=n) == (0, [])
    dev = want.copy()
    planted = np.arange(5, n, 1000)                              # 300 differences, over every thread's slice
    dev[planted] ^= 1
    bad, first = ref.check("sinf", dev, first_bits=first_bits, count=n)
    assert bad == len(planted) and len(first) == 64
    assert [m[0] for m in first] == [first_bits + int(i) for i in planted[:64]]
    assert all(m[2] == m[3] ^ 1 for m in first)


def test_reference_divide_sqrt_and_bit_reversal(ref):
    """The helper's IEEE operations against numpy's float32 (correctly rounded on the CPU) and a bit reversal by strings."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 2 ** 32, 4096, dtype=np.uint32)
    b = rng.integers(0, 2 ** 32, 4096, dtype=np.uint32)
    with np.errstate(all="ignore"):
        q = (a.view(np.float32) / b.view(np.float32)).view(np.uint32)
        s = np.sqrt(a.view(np.float32)).view(np.uint32)
    assert ref.check("div", q, a=a, b=b)[0] == 0
    assert ref.check("sqrt", s, a=a)[0] == 0
    rev = np.array([int(format(int(v), "032b")[::-1], 2) for v in a[:256]], np.uint32)
    np.testing.assert_array_equal(ref.eval("brev", a[:256]), rev)
    # denormal results and operands are kept: 0x1p-126 / 2 and sqrt of the smallest denormal
    assert ref.eval("div", np.array([0x00800000], np.uint32), np.array([f32_bits(2.0)], np.uint32))[0] == 0x00400000
    assert ref.eval("sqrt", np.array([1], np.uint32))[0] == f32_bits(2.0 ** -74.5)
