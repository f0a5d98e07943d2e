"""What tests/test_{scene,mesh,lighting,texture}_update_host.py share: building their simulators (tests/*sim/*.cpp, stand-alone host
programs over the library's host headers) and the head of a run — save the two scenes, run, and check what every simulator prints."""
import os
import re
import subprocess

from tests.conftest import ROOT


def build_sim(exe, sources, sanitized=False):
    """sources (paths below tests/) and the generated LUT data -> the program `exe`; sanitized: under -fsanitize=address,undefined (a
    stand-alone program: nothing is preloaded)"""
    mode = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else \
           ["-O2", "-ffp-contract=off"]
    sources = [os.path.join(ROOT, "tests", s) for s in sources] + [os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp")]
    r = subprocess.run(["g++", "-std=c++17"] + mode + ["-o", exe] + sources + ["-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_sim(exe, tmp_path, s0, s1, tags, *args):
    """exe old.yscn new.yscn [args] -> its output: it ends in OK with status 0, no comparison is DIFFERENT and every tag has its
    EQUAL line"""
    a, b = os.path.join(tmp_path, "old.yscn"), os.path.join(tmp_path, "new.yscn")
    s0.save(a)
    s1.save(b)
    r = subprocess.run([exe, a, b] + [str(v) for v in args], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-2000:]
    assert "DIFFERENT" not in r.stdout
    for tag in tags:
        assert re.search(rf"^EQUAL {tag} ", r.stdout, re.M), tag
    return r.stdout
