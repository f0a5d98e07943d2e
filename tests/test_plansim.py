"""csrc/render_host.hpp on the host alone (tests/plansim): the wave schedule every entry point walks and the tables of
YartAovBuffers / YartMomentBuffers with their check-and-copy, lay-out and clear helpers — built plain and under
ASan + UBSan (a stand-alone program: host code only, no device, nothing loaded into Python)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FLAGS = {"plain": ["-O2"],
         "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.mark.parametrize("build", list(FLAGS))
def test_plansim(tmp_path, build):
    exe = str(tmp_path / "plansim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                       ["-o", exe, os.path.join(ROOT, "tests", "plansim", "plansim.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    # samples 1..70 x five first-wave sizes x five maximum sizes
    assert lines[0] == f"schedule {70 * 5 * 5} cases" and lines[-2] == "plansim ok", r.stdout
