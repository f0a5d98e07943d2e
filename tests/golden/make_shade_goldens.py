"""Regenerates tests/golden/shading/ — the shading suites of tests/shadesuite.py with the compiled reference's records for them.

Runs only where the compiled reference can be built (oracle/_ref/yart_ref):
    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_shade_goldens.py

Per suite (tests/shadesuite.py SUITES):
    <suite>.yscn / .txt     the scene and the render parameters (unused by the shading code; the checkers' command lines take them)
    <suite>.cases           the case records, 128 bytes each (oracle/shaderec.hpp)
    <suite>.rec             the result records of `yart_ref shade`, 128 bytes each: the reference's own Texture, LUT functions, BSDF,
                            Light and PowerLightSampler per case
    <suite>.events          the oracle restatement's event mask per case (u32, bit k = shadesuite.EVENTS[k]) from `yart_oracle shade`
    <suite>.events.json     the number of cases that met each event
and for the `lights` suite lights.state2.yscn / lights.state2.rec: the scene in the second state of its maps and emissions (what
the device test moves the first one to through yart_hip_scene_update_lighting) and the reference's records of the same cases there.
The table of mutations in README.md is made by hand from tests of mutated copies (see there); this script prints the event
counts and the NaN share of every suite in the README's form.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import shadesuite  # noqa: E402
from yart_amd import scenes  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "yart_ref")
ORACLE = os.path.join(ROOT, "oracle", "_build", "yart_oracle")
OUT = os.path.join(HERE, "shading")
LARGEST_FIXTURE = 294348


def nan_share(rec):
    w = rec.view(np.uint32)
    return float((((w & 0x7f800000) == 0x7f800000) & ((w & 0x007fffff) != 0)).mean())


def main():
    os.makedirs(OUT, exist_ok=True)
    rows = []
    for name in shadesuite.SUITES:
        s, p, cases = shadesuite.build(name)
        base = os.path.join(OUT, name)
        s.save(base + ".yscn")
        scenes.write_params(base + ".txt", p)
        cases.tofile(base + ".cases")
        subprocess.run([REF, "shade", base + ".yscn", base + ".txt", base + ".cases", base + ".rec"], check=True, capture_output=True)
        tmp = base + ".oracle.tmp"
        r = subprocess.run([ORACLE, "shade", base + ".yscn", base + ".txt", base + ".cases", tmp], check=True, capture_output=True, text=True)
        counts = json.loads(r.stdout.strip().splitlines()[-1])
        rec, orc = np.fromfile(base + ".rec", np.uint32), np.fromfile(tmp, np.uint32)
        nan = ((rec & 0x7f800000) == 0x7f800000) & ((rec & 0x007fffff) != 0)
        same = bool(np.array_equal(rec[~nan], orc[~nan]))
        os.replace(tmp + ".events", base + ".events")
        for ext in ("", ".probs", ".tables.json"):
            os.remove(tmp + ext)
        with open(base + ".events.json", "w") as f:
            json.dump(counts, f, indent=1)
            f.write("\n")
        files = [".yscn", ".txt", ".cases", ".rec", ".events", ".events.json"]
        if name == "lights":
            s2 = shadesuite.lights_scene(1)
            s2.save(base + ".state2.yscn")
            subprocess.run([REF, "shade", base + ".state2.yscn", base + ".txt", base + ".cases", base + ".state2.rec"], check=True, capture_output=True)
            files += [".state2.yscn", ".state2.rec"]
        size = sum(os.path.getsize(base + f) for f in files)
        for f in files:
            assert os.path.getsize(base + f) <= LARGEST_FIXTURE, (name, f, os.path.getsize(base + f))
        share = nan_share(np.fromfile(base + ".rec", np.uint32))
        print(f"{name}: {len(cases)} cases, {size} bytes in {len(files)} files, NaN share {100 * share:.3f} %, oracle == reference: {same}")
        rows.append((name, counts))
    for name, c in rows:
        print(f"| {name} | {c['cases']} | " + ", ".join(f"{e} {c[e]}" for e in shadesuite.TARGETS[name]) + " |")


if __name__ == "__main__":
    main()
