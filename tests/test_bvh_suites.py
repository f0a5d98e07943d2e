"""Both BVH builders on the aimed meshes of tests/bvhsuite.py against the compiled reference's own trees.

tests/golden/bvh/trees.json holds, per case, what `yart_ref kat` reported for the reference's tree in its "bvh" section: the node count, the FNV-1a of
the node words and the FNV-1a of the index array (tools/make_bvh_goldens.py). Every frame depends on the tree being the reference's
byte for byte — it fixes the traversal order and with it the sampler state of every later bounce —, and a wrong tree does not crash:
it renders a frame that differs in some pixels of some scenes.

CPU: the records follow from the recipe (with the compiled reference present); the host builder (csrc/bvh_build.hpp, one thread and
five) gives the recorded tree for every case; the patterns cases hold what they claim (the recorded permutation is the reference's
five-line loop run on the prescribed bits in Python); the events the groups are aimed at are met by at least 8 cases each
(tests/golden/bvh/README.md has the table, events.json the numbers).
GPU: the device builder (csrc/bvh_build_device.inc) gives the recorded tree for every case, alone and through
DeviceScene.update_meshes with one scratch serving meshes of different sizes; what it refuses, it refuses cleanly. The GPU tests read
tests/golden/bvh/ and the generators only."""
import json
import os

import numpy as np
import pytest

from tests import bvhsuite

FLOOR = 8
REF_BIN = os.path.join(bvhsuite.ROOT, "oracle", "_ref", "yart_ref")


@pytest.fixture(scope="module")
def records():
    return bvhsuite.load_records()


@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    return api


@pytest.fixture(scope="module")
def host_trees(api):
    """{group: [(nodes, idx)] in the order of the group's cases} from the host builder on one thread, built once"""
    return {g: [api.bvh_build(pos, faces, device=None, threads=1)[:2] for _, pos, faces in bvhsuite.group_cases(g)]
            for g in bvhsuite.GROUPS + ("refused",)}


def _explain(group, k, nodes, idx, tmp_path):
    """where a builder's tree first differs from the reference's own arrays (needs the compiled reference)"""
    if not os.path.exists(REF_BIN):
        return "(the compiled reference is not here: no arrays to compare)"
    bvhsuite.reference_records(REF_BIN, group, str(tmp_path))
    rn, ri = bvhsuite.reference_tree(REF_BIN, os.path.join(str(tmp_path), f"{group}.yscn"), k, str(tmp_path))
    return "builder against reference: " + bvhsuite.first_difference(nodes, idx, rn, ri)


def test_records_follow_from_the_recipe(ref_bin, records, tmp_path):
    """tools/make_bvh_goldens.py's recipe, run again, gives trees.json: the goldens cannot drift from the generators or the driver"""
    assert set(records) == set(bvhsuite.GROUPS + ("refused",))
    for group in records:
        again = bvhsuite.reference_records(ref_bin, group, str(tmp_path))
        assert list(again) == list(records[group]), f"{group}: the case names differ"
        bad = [name for name in again if again[name] != records[group][name]]
        assert not bad, f"{group}: {len(bad)} records differ from what the reference gives now, e.g. {bad[:5]}"


def test_the_cases_are_what_the_generators_promise(records):
    """deterministic, finite, named once; the recorded names are the generators'"""
    for group in bvhsuite.GROUPS:
        cases = bvhsuite.group_cases(group)
        assert [n for n, _, _ in cases] == list(records[group]) and len({n for n, _, _ in cases}) == len(cases)
        for name, pos, faces in cases:
            assert pos.dtype == np.float32 and faces.dtype == np.uint32 and faces.shape[1] == 3 and faces.max() < len(pos), name
            assert np.isfinite(pos).all(), name
            if group != "refused":
                assert np.isfinite(bvhsuite.centroids(pos, faces)).all(), f"{name}: (v0 + v1) + v2 overflows: the device refuses that by design"
    sizes = {len(f) for name, _, f in bvhsuite.patterns() if name.startswith("n")}
    assert sizes == set(bvhsuite.SIZES_REGISTER + bvhsuite.SIZES_WAVE + bvhsuite.SIZES_BLOCK)
    assert max(len(f) for g in bvhsuite.GROUPS for _, _, f in bvhsuite.group_cases(g)) <= 5100
    assert os.path.getsize(bvhsuite.TREES) < 1 << 20


@pytest.mark.parametrize("group", bvhsuite.GROUPS + ("refused",))
def test_host_builder_gives_the_reference_tree(api, records, host_trees, tmp_path, group):
    """api.bvh_build(device=None, threads=1) == the record, for every case; threads=5 == threads=1 on bytes, hence == the record"""
    for k, (name, pos, faces) in enumerate(bvhsuite.group_cases(group)):
        nodes, idx = host_trees[group][k]
        got = bvhsuite.record_of(nodes, idx)
        assert got == records[group][name], f"{group}/{name}: host builder {got} against the record {records[group][name]}; " + \
            _explain(group, k, nodes, idx, tmp_path)
        n5, i5, _ = api.bvh_build(pos, faces, device=None, threads=5)
        assert np.array_equal(n5, nodes) and np.array_equal(i5, idx), f"{group}/{name}: 5 threads: " + bvhsuite.first_difference(n5, i5, nodes, idx)


def test_hostsim_bvhsum_gives_the_records(hostsim, records, tmp_path):
    """`hostsim bvhsum` — the host builder behind the mode the mutation table of tests/golden/bvh/README.md is made with — writes the
    records of every group's scene (threads 1 and 5), in the form of the "bvh" section of `yart_ref kat`"""
    import subprocess
    for group in bvhsuite.GROUPS + ("refused",):
        cases = bvhsuite.group_cases(group)
        path, out = str(tmp_path / f"{group}.yscn"), str(tmp_path / f"{group}.json")
        bvhsuite.scene_of(cases).save(path)
        for threads in (1, 5):
            r = subprocess.run([hostsim, "bvhsum", path, str(threads), out], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            with open(out) as f:
                v = json.load(f)["bvh"]
            assert [v[3 * k:3 * k + 3] for k in range(len(cases))] == [records[group][n] for n, _, _ in cases], (group, threads)


def test_patterns_hold_what_they_claim(records, host_trees):
    """For every patterns case the recorded permutation is the reference's loop run on the bits in Python, and the root's left child
    has popcount(L) triangles (read from the host builder's tree where its hash is the record's, i.e. from the reference's tree)."""
    specs = bvhsuite.pattern_specs()
    for k, (name, pos, faces) in enumerate(bvhsuite.patterns()):
        bits, bits2 = specs[name]
        want, m = bvhsuite.expected_permutation(bits, bits2)
        assert m == int(np.count_nonzero(bits)) and 0 < m < len(bits), name
        assert bvhsuite.fnv1a(want.tobytes()) == records["patterns"][name][2], f"{name}: the recorded permutation is not the loop's on the bits"
        nodes, idx = host_trees["patterns"][k]
        assert bvhsuite.record_of(nodes, idx) == records["patterns"][name], name
        _, total, _ = bvhsuite.tree_shape(nodes)
        assert nodes[0, 7] == 0 and total[nodes[0, 6]] == m and total[0] == len(bits), f"{name}: the root's left child has {total[nodes[0, 6]]} triangles, not {m}"
        assert records["patterns"][name][0] == (3 if bits2 is None else 7 - 2 * sum(len({bool(bits2[t]) for t in part}) == 1 for part in (want[:m], want[m:]))), name


def test_partition_loop_edge_inputs():
    """the Python loop itself, on inputs whose result is known in closed form: nothing left rotates by one, everything left moves
    nothing, sorted input rotates its right part by one (position m is examined in place), one right element in front goes to the end"""
    n = 9
    assert bvhsuite.partition_loop(range(n), [False] * n) == (list(range(1, n)) + [0], 0)
    assert bvhsuite.partition_loop(range(n), [True] * n) == (list(range(n)), n)
    assert bvhsuite.partition_loop(range(n), [k < 4 for k in range(n)]) == ([0, 1, 2, 3, 5, 6, 7, 8, 4], 4)
    assert bvhsuite.partition_loop(range(n), [k != 0 for k in range(n)]) == ([n - 1] + list(range(1, n - 1)) + [0], n - 1)


def test_events_meet_their_floors(records, host_trees):
    """Counted on the reference's trees (the host builder's, each checked against its record first): every event of
    bvhsuite.EVENTS is met by at least 8 cases of the suite, the costs-all-non-finite event by at least 8 of `extremes`; the counts
    are events.json's (the README's table), and the two depths are at least the measured values recorded there — a generator that
    loses an event or a depth fails here. Where a count falls short, add inputs."""
    trees = {}
    for group in bvhsuite.GROUPS:
        trees[group] = []
        for (name, pos, faces), (nodes, idx) in zip(bvhsuite.group_cases(group), host_trees[group]):
            assert bvhsuite.record_of(nodes, idx) == records[group][name], f"{group}/{name}"
            trees[group].append((nodes, idx, pos, faces))
    counts = bvhsuite.count_events(trees)
    with open(os.path.join(os.path.dirname(bvhsuite.TREES), "events.json")) as f:
        recorded = json.load(f)
    for group in bvhsuite.GROUPS:
        print(group, counts[group])
    for e in bvhsuite.EVENTS:
        if e != "non_finite_costs":
            assert sum(counts[g][e] for g in bvhsuite.GROUPS) >= FLOOR, f"{e}: met by fewer than {FLOOR} cases"
    assert counts["extremes"]["non_finite_costs"] >= FLOOR
    for group in bvhsuite.GROUPS:
        for e in bvhsuite.EVENTS:
            assert counts[group][e] == recorded[group][e], f"{group}: {e}: {counts[group][e]} cases, events.json says {recorded[group][e]}"
        for e in bvhsuite.DEPTHS:
            assert counts[group][e] >= recorded[group][e], f"{group}: {e} is {counts[group][e]}, was {recorded[group][e]}"


def test_lattice_points_are_reached():
    """The lattice cases' centroids are the builders' own split positions `bsize * (float(k) / 20)` exactly wherever a float sum can
    give them (fl(fl(3 x) / 3)); the first and the last point, which set the bins, always are."""
    for p in (0, 3, -7):
        for npts in (21, 41):
            pts = bvhsuite.lattice_points(npts, p)
            hit = [bvhsuite.reach(c)[1] for c in pts]
            assert hit[0] and hit[-1] and sum(hit) >= npts * 2 // 3, (p, npts, hit)
            for c, ok in zip(pts, hit):
                x = bvhsuite.reach(c)[0]
                got = bvhsuite._cent1(x, x, x)
                assert (got == c) == ok and abs(float(got) - float(c)) <= 2 * float(np.spacing(c)) , (p, npts, c, got)


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu_api(api):
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


def _device_case(api, group, name, pos, faces, want):
    nodes, idx, _ = api.bvh_build(pos, faces, device=0)
    got = bvhsuite.record_of(nodes, idx)
    if got != want:
        hn, hi, _ = api.bvh_build(pos, faces, device=None, threads=1)
        return f"{group}/{name} ({len(faces)} triangles): device {got} against the record {want}; device against host builder: " + \
            bvhsuite.first_difference(nodes, idx, hn, hi)
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("group", bvhsuite.GROUPS)
def test_device_builder_gives_the_reference_tree(gpu_api, records, group):
    """api.bvh_build(device=0) == the record (node count and both hashes) for every case of the group"""
    bad = []
    for name, pos, faces in bvhsuite.group_cases(group):
        msg = _device_case(gpu_api, group, name, pos, faces, records[group][name])
        if msg:
            bad.append(msg)
    assert not bad, f"{len(bad)} cases differ:\n" + "\n".join(bad[:10])


def _forty(records):
    """40 patterns and handover cases of varied sizes"""
    pool = [("patterns", c) for c in bvhsuite.patterns()] + [("handover", c) for c in bvhsuite.handover()]
    pick = np.random.RandomState(77).permutation(len(pool))
    chosen, sizes = [], set()
    for k in pick:                                             # distinct sizes first
        n = len(pool[k][1][2])
        if n not in sizes and len(chosen) < 40:
            sizes.add(n); chosen.append(pool[k])
    assert len(chosen) == 40 and {g for g, _ in chosen} == {"patterns", "handover"}
    return chosen


@pytest.mark.gpu
def test_sizes_down_then_up_and_one_scratch_for_many_meshes(gpu_api, records):
    """40 cases in descending, then ascending size within one process: the recorded trees. Then twelve of them as the meshes of one
    scene, each first in another state (its triangles' positions in reverse order), moved to the case's positions by one
    update_meshes call — one Scratch serves meshes of different sizes, large before small and small before large: mesh_records equal
    those of a fresh scene, and the scene's trees are the recorded ones."""
    api = gpu_api
    chosen = sorted(_forty(records), key=lambda gc: -len(gc[1][2]))
    for group, (name, pos, faces) in chosen + chosen[::-1]:
        msg = _device_case(api, group, name, pos, faces, records[group][name])
        assert msg is None, msg
    some = [chosen[k] for k in (0, 39, 3, 30, 8, 20, 1, 35, 12, 25, 5, 38)]
    target = bvhsuite.scene_of([c for _, c in some])
    start = bvhsuite.scene_of([(n, np.ascontiguousarray(p.reshape(-1, 3, 3)[::-1].reshape(-1, 3)), f) for _, (n, p, f) in some])
    A = api.DeviceScene(start, device=0)
    B = api.DeviceScene(target, device=0)
    differs = 0
    for m in range(len(some)):
        a, b = A.mesh_records(m), B.mesh_records(m)
        differs += a["nodes"].tobytes() != b["nodes"].tobytes() or a["leaves"].tobytes() != b["leaves"].tobytes()
    assert differs >= 6, "the first state must have other trees"
    A.update_meshes({m: target.meshes[m].positions for m in range(len(some))})
    assert A.last_update["launches"] >= 8, f"the device builder ran: {A.last_update}"
    for m, (group, (name, pos, faces)) in enumerate(some):
        a, b = A.mesh_records(m), B.mesh_records(m)
        assert a["mesh"].tobytes() == b["mesh"].tobytes(), f"mesh {m} ({name}): MeshDev"
        for key in ("nodes", "leaves", "shade", "positions"):
            assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), f"mesh {m} ({name}): {key}"
        for S in (A, B):
            nodes, idx = S.bvh(m)
            assert bvhsuite.record_of(nodes, idx) == records[group][name], f"mesh {m} ({name})"
    A.close()
    B.close()


@pytest.mark.gpu
def test_refusals_stay_clean(gpu_api, records):
    """A vertex at +inf, and three finite vertices of 3e38 whose centroid sum overflows: yart_hip_bvh_build_device answers with an error
    (and builds the next mesh as if nothing had been). A scene that holds the overflowing mesh still comes up, with the host builder's
    tree — the reference's, which builds that mesh without complaint (tests/golden/bvh/README.md)."""
    api = gpu_api
    pos, faces = bvhsuite.soup(50, 7)
    pos[17, 1] = np.inf
    with pytest.raises(api.YartError):
        api.bvh_build(pos, faces, device=0)
    opos, ofaces = bvhsuite.overflow_mesh()
    assert np.isfinite(opos).all() and not np.isfinite(bvhsuite.centroids(opos, ofaces)).all()
    with pytest.raises(api.YartError):
        api.bvh_build(opos, ofaces, device=0)
    name, pos, faces = bvhsuite.handover()[0]
    assert _device_case(api, "handover", name, pos, faces, records["handover"][name]) is None
    want = records["refused"]["overflowing_centroid"]
    hn, hi, _ = api.bvh_build(opos, ofaces, device=None, threads=1)
    assert bvhsuite.record_of(hn, hi) == want
    S = api.DeviceScene(bvhsuite.scene_of([("overflowing_centroid", opos, ofaces)]), device=0)
    nodes, idx = S.bvh(0)
    assert bvhsuite.record_of(nodes, idx) == want, bvhsuite.first_difference(nodes, idx, hn, hi)
    S.close()
