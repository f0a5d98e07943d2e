"""Regenerates tests/golden/rays/ — the ray suites of tests/raysuite.py with the compiled reference's records for them.

Runs only where the compiled reference can be built (oracle/_ref/yart_ref):
    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_ray_goldens.py

Per suite (tests/raysuite.py SUITES):
    <suite>.yscn / .txt     the scene and the render parameters (sampler: spp, tile)
    <suite>.rays            the ray records, 48 bytes each (oracle/rayrec.hpp)
    <suite>.rec             the result records of `yart_ref hits`, 80 bytes each: the reference's own testNode per ray
    <suite>.events          the oracle restatement's event mask per ray (u16, bit k = raysuite.EVENTS[k]) from `yart_oracle hits`
    <suite>.events.json     the number of rays that met each event
The table of mutations in README.md is made by hand from tests of mutated copies (see there); this script prints the event
counts in the README's form.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import raysuite  # noqa: E402
from yart_amd import scenes  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "yart_ref")
ORACLE = os.path.join(ROOT, "oracle", "_build", "yart_oracle")
OUT = os.path.join(HERE, "rays")


def main():
    os.makedirs(OUT, exist_ok=True)
    rows = []
    for name in raysuite.SUITES:
        s, p, rays = raysuite.build(name)
        base = os.path.join(OUT, name)
        s.save(base + ".yscn")
        scenes.write_params(base + ".txt", p)
        rays.tofile(base + ".rays")
        subprocess.run([REF, "hits", base + ".yscn", base + ".txt", base + ".rays", base + ".rec"], check=True)
        tmp = base + ".oracle.tmp"
        r = subprocess.run([ORACLE, "hits", base + ".yscn", base + ".txt", base + ".rays", tmp], check=True, capture_output=True, text=True)
        counts = json.loads(r.stdout.strip().splitlines()[-1])
        same = open(tmp, "rb").read() == open(base + ".rec", "rb").read()
        os.replace(tmp + ".events", base + ".events")
        os.remove(tmp)
        with open(base + ".events.json", "w") as f:
            json.dump(counts, f, indent=1)
            f.write("\n")
        rec = np.fromfile(base + ".rec", raysuite.REC)
        print(f"{name}: {len(rays)} rays, {s.n_triangles} triangles, {int(rec['hit'].sum())} hits, oracle == reference: {same}")
        for f in (".yscn", ".rays", ".rec"):
            assert os.path.getsize(base + f) <= 294348, (name, f, os.path.getsize(base + f))
        rows.append((name, counts))
    print("| suite | rays | " + " | ".join(raysuite.EVENTS) + " |")
    print("|---|---|" + "---|" * len(raysuite.EVENTS))
    for name, c in rows:
        print(f"| {name} | {c['rays']} | " + " | ".join(("**%d**" if e in raysuite.TARGETS[name] else "%d") % c[e] for e in raysuite.EVENTS) + " |")


if __name__ == "__main__":
    main()
