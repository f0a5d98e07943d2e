#!/usr/bin/env python3
"""Writes tests/golden/bvh/trees.json and events.json: the compiled reference's trees of the aimed meshes of tests/bvhsuite.py.

Per group one .yscn is built in a scratch directory (every case a mesh, one trivial material, one node per mesh) and handed to
`yart_ref kat`, whose "bvh" section builds every mesh's BVH with the reference's own builder in one run and reports per mesh the
node count, the FNV-1a of the node words and the FNV-1a of the index array (the render parameters the mode asks for are the
Cornell golden's; the section does not depend on them). The scenes are not kept: the generators
reproduce them. A case on which the reference dies is a reason to drop it from its generator (and to name it in
tests/golden/bvh/README.md), not to record something else.

events.json holds, per group, the number of cases that meet each event of bvhsuite.EVENTS and the two depths — counted on the host
builder's trees after each has been checked against its record, i.e. on the reference's trees. `--table` prints them as the
markdown table of the README.

    python tools/make_bvh_goldens.py [--ref oracle/_ref/yart_ref] [--keep DIR] [--table]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bvhsuite  # noqa: E402


def host_trees(groups):
    from yart_amd import api
    return {g: [api.bvh_build(pos, faces, device=None, threads=1)[:2] + (pos, faces) for _, pos, faces in bvhsuite.group_cases(g)] for g in groups}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "yart_ref"))
    ap.add_argument("--keep", default=None, help="directory for the groups' .yscn files (default: a temporary one, removed)")
    ap.add_argument("--table", action="store_true", help="print the event table")
    a = ap.parse_args()
    out_dir = os.path.dirname(bvhsuite.TREES)
    os.makedirs(out_dir, exist_ok=True)
    records = {}
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        os.makedirs(work, exist_ok=True)
        for group in bvhsuite.GROUPS + ("refused",):
            records[group] = bvhsuite.reference_records(a.ref, group, work)
            tris = sum(len(f) for _, _, f in bvhsuite.group_cases(group))
            print(f"{group}: {len(records[group])} cases, {tris} triangles", flush=True)
    with open(bvhsuite.TREES, "w") as f:
        f.write("{\n" + ",\n".join(f' "{g}": {{\n' + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in r.items()) + "\n }"
                                   for g, r in records.items()) + "\n}\n")
    trees = host_trees(bvhsuite.GROUPS)
    differ = [(g, name) for g in bvhsuite.GROUPS for (name, _, _), t in zip(bvhsuite.group_cases(g), trees[g])
              if bvhsuite.record_of(t[0], t[1]) != records[g][name]]
    if differ:
        print(f"the host builder differs from the reference on {len(differ)} cases, e.g. {differ[:5]}: events.json not written")
        return 1
    events = bvhsuite.count_events(trees)
    with open(os.path.join(out_dir, "events.json"), "w") as f:
        json.dump(events, f, indent=1)
        f.write("\n")
    if a.table:
        names = bvhsuite.EVENTS + bvhsuite.DEPTHS
        print("| group | cases | " + " | ".join(names) + " |")
        print("|---|---|" + "---|" * len(names))
        for g in bvhsuite.GROUPS:
            print(f"| {g} | {len(records[g])} | " + " | ".join(str(events[g][e]) for e in names) + " |")
        print("| all | | " + " | ".join(str(sum(events[g][e] for g in bvhsuite.GROUPS)) if e in bvhsuite.EVENTS
                                        else str(max(events[g][e] for g in bvhsuite.GROUPS)) for e in names) + " |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
