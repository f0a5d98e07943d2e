"""tests/libm_ref/libm_ref.c for the tests: this machine's libm (the libm the compiled reference calls) and IEEE fp32 divide / sqrt,
compiled per test session with gcc and bound with ctypes. The comparison with a buffer of device results happens in C; Python sees
a mismatch count and the first <= 64 mismatches."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "libm_ref", "libm_ref.c")
# enum of libm_ref.c == enum YartMathFn of include/yart_hip.h == yart_amd.api.MATH_FNS; "copy": the reference result is operand a
FNS = {"sinf": 0, "cosf": 1, "sinf2pi": 2, "cosf2pi": 3, "logf": 4, "expf": 5, "log2f": 6, "powf": 7, "div": 8, "sqrt": 9,
       "brev": 10, "copy": 100}
BAD_ARGUMENT = 2 ** 64 - 1


class Mismatch(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("device", C.c_uint32), ("libm", C.c_uint32)]


def f32_bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def _words(v):
    v = np.asarray(v)
    if v.dtype != np.uint32:
        v = v.astype(np.float32).view(np.uint32)
    return np.ascontiguousarray(v).reshape(-1)


class LibmRef:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libm_ref.so")
        subprocess.run(["gcc", "-O1", "-fno-builtin", "-shared", "-fPIC", "-o", so, SRC, "-lm", "-lpthread"], check=True)
        self.L = C.CDLL(so)
        self.L.libm_ref_check.restype = C.c_uint64
        self.L.libm_ref_check.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(Mismatch), C.c_void_p]
        self.L.libm_ref_threads.argtypes = [C.c_uint64]

    def check(self, fn, device, first_bits=0, count=None, y=0.0, a=None, b=None):
        """Compares ``device`` (uint32 bit patterns) with fn over the range first_bits .. first_bits + count - 1 (second operand y) or
        over the operand arrays a (, b). Returns (mismatches, [(a bits, b bits, device bits, libm bits), ...] — the first <= 64)."""
        device = _words(device)
        wa = None if a is None else _words(a)
        wb = None if b is None else _words(b)
        n = int(count) if wa is None else wa.size
        assert device.size >= n and (wb is None or wb.size == n)
        first = (Mismatch * 64)()
        ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        bad = self.L.libm_ref_check(FNS[fn], int(first_bits), n, f32_bits(y), ptr(wa), ptr(wb), ptr(device), first, None)
        assert bad != BAD_ARGUMENT, "libm_ref_check: bad argument"
        return int(bad), [(m.a, m.b, m.device, m.libm) for m in first[:min(bad, 64)]]

    def eval(self, fn, a, b=None):
        """fn over the operand arrays -> uint32 bit patterns (small inputs: the tests' own tables)."""
        wa = _words(a)
        wb = None if b is None else _words(b)
        out = np.empty(wa.size, np.uint32)
        ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        bad = self.L.libm_ref_check(FNS[fn], 0, wa.size, 0, ptr(wa), ptr(wb), None, None, ptr(out))
        assert bad != BAD_ARGUMENT, "libm_ref_check: bad argument"
        return out

    def threads(self, n):
        return int(self.L.libm_ref_threads(int(n)))


def describe(fn, first):
    """The mismatches of LibmRef.check as text (hex-float operands, both results' bits)."""
    rows = []
    for a, b, dev, ref in first[:16]:
        x = float(np.uint32(a).view(np.float32))
        rows.append(f"{fn}({x.hex()} = 0x{a:08x}" + (f", 0x{b:08x}" if fn in ("powf", "div") else "") + f"): device 0x{dev:08x}, libm 0x{ref:08x}")
    return "\n".join(rows)
