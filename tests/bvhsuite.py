"""Aimed meshes for the two BVH builders (csrc/bvh_build.hpp on the host, csrc/bvh_build_device.inc on the device), one generator
per group, and what the tests need to read a tree: the reference's partition loop, the event counts, the FNV-1a of the kat files.

A case is a (name, positions (nv, 3) float32, faces (nf, 3) uint32) triple. Everything is deterministic (np.random.RandomState(seed),
nothing else) and every coordinate is finite. The expected trees are the compiled reference's, recorded in
tests/golden/bvh/trees.json by tools/make_bvh_goldens.py; tests/test_bvh_suites.py compares both builders with them.

  patterns   a root whose partition is a prescribed left / right sequence: what the device's closed-form partition restates
  handover   soups whose root and child sizes sit on the thresholds between the device's three split paths and its leaves
  lattice    centroids on the bin boundaries k / 20 * 2^p (and half-way between), on each axis in turn and on all three at once
  extremes   areas that overflow, extents whose 20 / size overflows, denormals, collapsing offsets, flat and linear meshes
  chains     scenes.chain_mesh, and chains of clusters of identical triangles (deep trees built by the level kernels)
"""
from __future__ import annotations

import functools
import json
import os
import subprocess

import numpy as np

GROUPS = ("patterns", "handover", "lattice", "extremes", "chains")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = os.path.join(ROOT, "tests", "golden", "bvh", "trees.json")
KAT_PARAMS = os.path.join(ROOT, "tests", "golden", "cornell.txt")

MAX_LEAF = 20                 # MAX_LEAF_SIZE of the reference
LOCAL_SPAN, BIG_SPAN = 256, 2048      # kLocalSpan, kBigSpan of the device builder
THRESHOLDS = (20, 21, 255, 256, 257, 2047, 2048, 2049)
F = np.float32


def _faces(n):
    return np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def soup(n, seed, extent=4.0, size=0.3, centre=(0.0, 0.0, 0.0)):
    rng = np.random.RandomState(seed)
    c = (rng.rand(n, 1, 3) - 0.5) * extent + np.asarray(centre, np.float64)
    return (c + (rng.rand(n, 3, 3) - 0.5) * size).astype(F).reshape(-1, 3), _faces(n)


def centroids(pos, faces):
    """((v0 + v1) + v2) / 3 in float32, as the reference and both builders compute it"""
    v = np.asarray(pos, F)[np.asarray(faces)[:, :3].astype(np.int64)]
    with np.errstate(over="ignore", invalid="ignore"):
        return ((v[:, 0] + v[:, 1]) + v[:, 2]) / F(3.0)


# ---------------------------------------------------------------------------------------------------------------- patterns
# One small triangle, narrower along x than along y: where a root could split on x or on y between two pairs of clusters one unit
# apart (the two-level variants), the children of the x split have the smaller boxes (their areas differ by tx - ty), so x wins.
_TRI = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.1], [0.0, 0.2, 0.0]], F)
SIZES_REGISTER = (21, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)     # splitNodeSmall
SIZES_WAVE = (257, 320, 321, 1023, 1025, 2047)                                 # splitNode<64>
SIZES_BLOCK = (2048, 2049, 3071, 3072, 3073, 4097)                             # splitNode<1024>


def partition_loop(idx, left):
    """The reference's loop (core/bvh.hpp, subdivide) on a list of triangle indices; left[t]: triangle t goes left. -> (list, m)"""
    idx = list(idx)
    i, j = 0, len(idx) - 1
    while i <= j:
        if left[idx[i]]:
            i += 1
        else:
            idx[i], idx[j] = idx[j], idx[i]
            j -= 1
    return idx, i


def expected_permutation(bits, bits2=None):
    """The index array the reference leaves for a patterns case: the loop on the root's bits, then (two-level variants) on each
    child's bits along y; clusters of one centroid are not permuted (at most 20: a leaf; more: every cost is NaN, the split is
    `c < 0` on x, everything goes left without a swap)."""
    idx, m = partition_loop(range(len(bits)), bits)
    if bits2 is not None:
        out = []
        for part in (idx[:m], idx[m:]):
            assert len(part) > MAX_LEAF
            kinds = {bool(bits2[t]) for t in part}
            out += partition_loop(part, bits2)[0] if len(kinds) == 2 else part
        idx = out
    return np.array(idx, np.uint32), m


def pattern_mesh(bits, bits2=None):
    bits = np.asarray(bits, bool)
    off = np.zeros((len(bits), 1, 3), F)
    off[:, 0, 0] = np.where(bits, F(-2.0), F(-1.0))
    if bits2 is not None:
        off[:, 0, 1] = np.where(np.asarray(bits2, bool), F(-2.0), F(-1.0))
    return (_TRI[None] + off).astype(F).reshape(-1, 3), _faces(len(bits))


def _with_count(n, m, seed, at_m=None):
    """n bits of which exactly m are L, at random; at_m: what position m holds"""
    rng = np.random.RandomState(seed)
    bits = np.zeros(n, bool)
    bits[rng.permutation(n)[:m]] = True
    if at_m is not None and m < n and bits[m] != at_m:           # exchange it with an element of the wanted kind
        other = np.nonzero(bits == at_m)[0]
        k = other[rng.randint(len(other))]
        bits[k], bits[m] = bits[m], bits[k]
    return bits


def sequences(n):
    """(tag, bits) for a root of n triangles; True = L"""
    L, R = True, False
    a = lambda *parts: np.concatenate([np.full(c, v, bool) for v, c in parts])
    out = [("L_then_last_R", a((L, n - 1), (R, 1))), ("R_then_last_L", a((R, n - 1), (L, 1))),
           ("first_R_then_L", a((R, 1), (L, n - 1))), ("first_L_then_R", a((L, 1), (R, n - 1))),
           ("alt_L", np.arange(n) % 2 == 0), ("alt_R", np.arange(n) % 2 == 1),
           ("sorted", a((L, n // 2), (R, n - n // 2))), ("reversed", a((R, n - n // 2), (L, n // 2))),
           ("one_L_mid", a((R, n // 2), (L, 1), (R, n - n // 2 - 1))), ("one_R_mid", a((L, n // 2), (R, 1), (L, n - n // 2 - 1)))]
    for m in (64, 128, 1024, 2048):
        if m < n:
            out.append((f"m{m}_L_at_m", _with_count(n, m, 7 * n + m, at_m=True)))
            out.append((f"m{m}_R_at_m", _with_count(n, m, 7 * n + m + 1, at_m=False)))
    for pct in (1, 50, 99):
        m = max(1, min(n - 1, int(round(n * pct / 100.0))))
        out.append((f"random_{pct}", _with_count(n, m, 11 * n + pct)))
    return out


# two-level variants: (n, m of the root, what splits the root / the children)
_TWO_LEVEL = ((300, 44, "wave/register"), (400, 200, "wave/register"), (512, 256, "wave/register"), (2047, 256, "wave/register+wave"),
              (1000, 255, "wave/register+wave"), (3000, 1500, "block/wave"), (4094, 2047, "block/wave"), (2305, 257, "block/wave+block"),
              (4000, 1999, "block/wave"), (2560, 512, "block/wave+block"))


@functools.lru_cache(maxsize=None)
def _patterns():
    cases, specs = [], {}
    for n in SIZES_REGISTER + SIZES_WAVE + SIZES_BLOCK:
        for tag, bits in sequences(n):
            name = f"n{n}_{tag}"
            cases.append((name,) + pattern_mesh(bits))
            specs[name] = (bits, None)
    for n, m, _ in _TWO_LEVEL:
        for k, at in enumerate((None, True, False)):
            bits = _with_count(n, m, 13 * n + k, at_m=at)
            for tag2, bits2 in (("alt", np.arange(n) % 2 == 0), ("random", _with_count(n, n // 2, 17 * n + k)),
                                ("few_L", _with_count(n, max(2, n // 50), 19 * n + k))):
                name = f"two_n{n}_m{m}_{k}_{tag2}"
                cases.append((name,) + pattern_mesh(bits, bits2))
                specs[name] = (bits, bits2)
    return cases, specs


def patterns():
    return _patterns()[0]


def pattern_specs():
    """name -> (bits of the root, bits along y or None)"""
    return _patterns()[1]


# ---------------------------------------------------------------------------------------------------------------- handover
def _soups(sizes, seed):
    """well-separated soups side by side along x (extent 1, 40 apart)"""
    parts = [soup(n, seed + 101 * k, extent=1.0, size=0.05, centre=(40.0 * k, 0.0, 0.0))[0] for k, n in enumerate(sizes)]
    return np.concatenate(parts), _faces(sum(sizes))


@functools.lru_cache(maxsize=None)
def handover():
    cases = []
    for i, a in enumerate(THRESHOLDS):
        for j, b in enumerate(THRESHOLDS):
            cases.append((f"pair_{a}_{b}",) + _soups((a, b), 1000 + 8 * i + j))
    for k, n in enumerate(THRESHOLDS):
        cases.append((f"single_{n}",) + soup(n, 2000 + k))
    # three soups: a big node on the second level and none on the third, big nodes further down, the big soup left, right, between
    for k, sizes in enumerate(((2100, 50, 50), (50, 50, 2100), (50, 2100, 50), (5000, 30, 30), (30, 30, 5000), (30, 5000, 30),
                               (2048, 300, 20), (300, 20, 2048), (2047, 2047, 257), (256, 2049, 2049), (4096, 256, 21), (21, 256, 4096))):
        cases.append(("three_" + "_".join(map(str, sizes)),) + _soups(sizes, 3000 + 10 * k))
    # bundles: a node of 20 such triangles is a leaf because a leaf is cheaper ((20 - 0.5) A against 20 A), not because it cannot be
    # split — the only kind of input on which `span <= 20` and `span < 20` part ways; 21 of them must split
    for k, (n, axis) in enumerate(((20, 2), (20, 0), (21, 2), (21, 1), (40, 2), (41, 0), (60, 1), (80, 2), (400, 0), (2060, 2))):
        cases.append((f"bundle_{n}_axis{axis}", bundle(n, axis), _faces(n)))
    for k, (a, n, axis, bundle_first) in enumerate(((257, 20, 2, False), (2048, 20, 0, True), (21, 20, 1, False), (20, 20, 2, True), (256, 40, 0, False))):
        s = soup(a, 3500 + k, extent=1.0, size=0.05, centre=(0.0 if not bundle_first else 40.0, 0.0, 0.0))[0]
        b = bundle(n, axis, centre=(40.0 if not bundle_first else 0.0, 0.0, 0.0))
        cases.append((f"soup_{a}_bundle_{n}_axis{axis}_{'bundle_left' if bundle_first else 'bundle_right'}", np.concatenate([s, b]), _faces(a + n)))
    return cases


def bundle(n, axis, centre=(0.0, 0.0, 0.0)):
    """n triangles of 2 x 2 stacked 0.001 apart along `axis`: every subset has (nearly) the box of the whole"""
    v = np.zeros((n, 3, 3), np.float64)
    a, b = [k for k in range(3) if k != axis]
    v[:, :, a] = np.array([-1.0, 1.0, 0.0])
    v[:, :, b] = np.array([-1.0, -1.0, 1.0])
    v[:, :, axis] = (np.arange(n) * 0.001)[:, None]
    return (v + np.asarray(centre, np.float64)).astype(F).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------- lattice
def _cent1(x0, x1, x2):
    return ((F(x0) + F(x1)) + F(x2)) / F(3.0)


def reach(c):
    """One coordinate for all three vertices of a triangle (it lies in a plane across the axis) such that the centroid the builders
    compute, fl(fl(3 x) / 3), is the float c — or, where no float sum gives c (the floats 3 c are coarser than c above 4/3 of a
    power of two), the nearest centroid that can be had. -> (x, exact)"""
    c = F(c)
    best = None
    x = c
    for _ in range(4):
        x = np.nextafter(x, F(-np.inf))
    for _ in range(9):
        got = _cent1(x, x, x)
        if got == c:
            return x, True
        if best is None or abs(float(got) - float(c)) < abs(float(best[1]) - float(c)):
            best = (x, got)
        x = np.nextafter(x, F(np.inf))
    return best[0], False


def lattice_points(npts, p):
    """the floats `bsize * (float(k) / float(npts - 1))` at bsize = 2^p: for npts = 21 the builders' own split positions"""
    return [F(np.ldexp(1.0, p)) * (F(k) / F(npts - 1)) for k in range(npts)]


def lattice_mesh(npts, p, axis, reps, seed, diagonal=False):
    """reps triangles per lattice point. axis 0..2: planar triangles across that axis, spread at random over [0, 2^p) on the other two.
    diagonal: points (all three vertices equal) on the diagonal, the same lattice on every axis: every axis has the same costs."""
    rng = np.random.RandomState(seed)
    s = np.ldexp(1.0, p)
    tris, inexact = [], 0
    for c in lattice_points(npts, p):
        x, exact = reach(c)
        inexact += not exact
        for _ in range(reps):
            if diagonal:
                v = np.full((3, 3), x, F)
            else:
                o = rng.rand(2) * s
                v = np.zeros((3, 3), F)
                others = [k for k in range(3) if k != axis]
                v[:, axis] = x
                v[:, others[0]] = F(o[0]) + np.array([0.0, 0.01, 0.0]) * s
                v[:, others[1]] = F(o[1]) + np.array([0.0, 0.0, 0.01]) * s
            tris.append(v)
    order = rng.permutation(len(tris))
    pos = np.stack(tris)[order].astype(F).reshape(-1, 3)
    return pos, _faces(len(tris)), inexact


@functools.lru_cache(maxsize=None)
def lattice():
    cases = []
    seed = 4000
    for p in (0, 3, -7):
        for npts in (21, 41):
            for reps in (4, 16):
                for axis in range(3):
                    seed += 1
                    cases.append((f"p{p}_n{npts}_x{reps}_axis{axis}",) + lattice_mesh(npts, p, axis, reps, seed)[:2])
                seed += 1
                cases.append((f"p{p}_n{npts}_x{reps}_diagonal",) + lattice_mesh(npts, p, 0, reps, seed, diagonal=True)[:2])
        for axis in range(3):                                   # a root for the 1024-thread form
            seed += 1
            cases.append((f"p{p}_n21_x110_axis{axis}",) + lattice_mesh(21, p, axis, 110, seed)[:2])
    return cases


# ---------------------------------------------------------------------------------------------------------------- extremes
SCALES = (-140, -130, -100, -40, 40, 60, 62, 63, 64, 80, 100)


def _points(x, rng, spread=1.0):
    """point triangles (three equal vertices) at the given x, y and z at random"""
    n = len(x)
    v = np.zeros((n, 3, 3), F)
    v[:, :, 0] = np.asarray(x, F)[:, None]
    v[:, :, 1] = (rng.rand(n, 1) * spread).astype(F)
    v[:, :, 2] = (rng.rand(n, 1) * spread).astype(F)
    return v.reshape(-1, 3), _faces(n)


@functools.lru_cache(maxsize=None)
def extremes():
    cases = []
    base = {300: soup(300, 5001), 3000: soup(3000, 5002)}
    for n, (pos, faces) in base.items():
        for k in SCALES:
            cases.append((f"soup{n}_scale_2^{k}", np.ldexp(pos, k).astype(F), faces))
        for axis in (0, 2):
            for off in (1e6, 1e7):
                q = pos.copy()
                q[:, axis] = (q[:, axis] + F(off)).astype(F)
                cases.append((f"soup{n}_offset_{off:.0e}_axis{axis}", q, faces))
        flat = pos.copy(); flat[:, 1] = F(0.7)
        cases.append((f"soup{n}_flat_y", flat, faces))
        line = pos.copy(); line[:, 1] = F(0.7); line[:, 2] = F(-0.25)
        cases.append((f"soup{n}_line_x", line, faces))
    for k, (n, steps, axis) in enumerate(((300, 20, 0), (3000, 20, 0), (300, 3, 0), (300, 40, 2), (3000, 200, 1))):
        rng = np.random.RandomState(5100 + k)
        x = F(1.0) + rng.randint(-steps, steps + 1, size=n).astype(F) * F(2.0 ** -24)      # one ulp below 1.0 apart (two above: exact)
        pos, faces = _points(x, rng)
        cases.append((f"ulps_n{n}_pm{steps}_axis{axis}", np.ascontiguousarray(np.roll(pos, axis, axis=1)), faces))
    for name, pos, faces in cases:
        assert np.isfinite(pos).all() and np.isfinite(centroids(pos, faces)).all(), name
    return cases


# ---------------------------------------------------------------------------------------------------------------- chains
def cluster_chain(size, count, sign=1.0, ratio=21.0):
    """`count` clusters of `size` identical triangles at x = sign * ratio^i: every split cuts the last cluster off, so the nodes
    above the clusters form a chain that the level kernels build; a cluster of more than 20 triangles ends as one leaf (every cost
    is NaN: the split is `c < 0` on x — to the left of 0 nothing moves, to the right the loop swaps every element)."""
    x = np.repeat(sign * ratio ** np.arange(count, dtype=np.float64), size).astype(F)
    pos = (_TRI[None] + np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)[:, None, :]).astype(F)
    return pos.reshape(-1, 3), _faces(size * count)


@functools.lru_cache(maxsize=None)
def chains():
    from yart_amd import scenes
    cases = []
    for levels, ratio in ((8, 24.0), (25, 24.0), (31, 24.0), (63, 24.0), (64, 24.0), (65, 24.0), (72, 24.0), (80, 21.0)):
        m = scenes.chain_mesh(levels, [0], ratio=ratio)
        cases.append((f"chain_{levels}_ratio{ratio:.0f}", m.positions.astype(F), np.ascontiguousarray(m.faces[:, :3], np.uint32)))
    for size, count, sign in ((257, 19, 1.0), (257, 8, 1.0), (257, 12, -1.0), (21, 10, 1.0), (64, 6, 1.0), (65, 6, 1.0), (256, 6, 1.0),
                              (300, 10, 1.0), (2048, 2, 1.0), (3000, 1, 1.0), (3000, 1, -1.0), (200, 1, 1.0), (128, 2, -1.0), (1, 28, 1.0)):
        cases.append((f"clusters_{size}x{count}_{'pos' if sign > 0 else 'neg'}",) + cluster_chain(size, count, sign))
    return cases


# ---------------------------------------------------------------------------------------------------------------- refusals
def overflow_mesh():
    """50 ordinary triangles and one whose three finite vertices sum to infinity: the device builder refuses it, the host builds it"""
    pos, faces = soup(50, 6001)
    big = np.array([[3e38, 0.0, 0.0], [3e38, 1.0, 0.0], [3e38, 0.0, 1.0]], F)
    return np.concatenate([pos, big]), _faces(51)


def group_cases(group):
    if group == "refused":
        return [("overflowing_centroid",) + overflow_mesh()]
    return {"patterns": patterns, "handover": handover, "lattice": lattice, "extremes": extremes, "chains": chains}[group]()


# ---------------------------------------------------------------------------------------------------------------- records
def fnv1a(data: bytes) -> int:
    """the hash of the kat files' "bvh" section (oracle/kat_common.hpp)"""
    h = 0xcbf29ce484222325
    for x in data:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def record_of(nodes, idx):
    nodes, idx = np.ascontiguousarray(nodes, np.uint32), np.ascontiguousarray(idx, np.uint32)
    return [int(len(nodes)), fnv1a(nodes.tobytes()), fnv1a(idx.tobytes())]


def load_records():
    with open(TREES) as f:
        return json.load(f)


def scene_of(cases):
    """all cases of a group as the meshes of one scene: one trivial material, one node per mesh"""
    from yart_amd import yscn
    s = yscn.Scene()
    s.add_material(yscn.Material())
    for _, pos, faces in cases:
        nrm = np.zeros((len(pos), 3), F); nrm[:, 2] = 1.0
        f4 = np.concatenate([faces[:, :3], np.zeros((len(faces), 1), np.uint32)], 1)
        s.add_node(s.add_mesh(yscn.Mesh(pos, nrm, None, None, f4)))
    return s


def reference_records(ref_bin, group, workdir):
    """{case: [node count, FNV-1a of the node words, FNV-1a of the index array]} from the compiled reference: the "bvh" section of
    `yart_ref kat`, which builds every mesh of the scene in one run (the render parameters are the Cornell golden's: the section
    does not depend on them); the group's scene is left at workdir/<group>.yscn"""
    cases = group_cases(group)
    path, out = os.path.join(workdir, f"{group}.yscn"), os.path.join(workdir, f"{group}.bvh.json")
    scene_of(cases).save(path)
    r = subprocess.run([ref_bin, "kat", path, KAT_PARAMS, out], capture_output=True, text=True)
    assert r.returncode == 0, f"yart_ref kat {group}: exit status {r.returncode}: {r.stderr[-2000:]}"
    with open(out) as f:
        v = json.load(f)["bvh"]
    assert len(v) == 3 * len(cases)
    return {name: v[3 * k:3 * k + 3] for k, (name, _, _) in enumerate(cases)}


def reference_tree(ref_bin, scene_path, mesh, workdir):
    """the reference's own arrays of one mesh of a scene (`yart_ref bvh`) -> (nodes (n, 8) u32, idx)"""
    out = os.path.join(workdir, "tree.bin")
    r = subprocess.run([ref_bin, "bvh", scene_path, str(mesh), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(out, np.uint32)
    n, nt = int(raw[0]), int(raw[1])
    return raw[2:2 + 8 * n].reshape(n, 8).copy(), raw[2 + 8 * n:2 + 8 * n + nt].copy()


def first_difference(nodes_a, idx_a, nodes_b, idx_b):
    """a sentence on where two trees first differ"""
    words = []
    n = min(len(nodes_a), len(nodes_b))
    bad = np.nonzero((np.asarray(nodes_a)[:n] != np.asarray(nodes_b)[:n]).any(axis=1))[0]
    if len(nodes_a) != len(nodes_b):
        words.append(f"{len(nodes_a)} nodes against {len(nodes_b)}")
    if len(bad):
        k = int(bad[0])
        words.append(f"first differing node {k}: {list(map(int, nodes_a[k]))} against {list(map(int, nodes_b[k]))}")
    bad = np.nonzero(np.asarray(idx_a) != np.asarray(idx_b))[0] if len(idx_a) == len(idx_b) else []
    if len(bad):
        k = int(bad[0])
        words.append(f"first differing index position {k}: {int(idx_a[k])} against {int(idx_b[k])} ({len(bad)} positions differ)")
    return "; ".join(words) or "no difference"


# ---------------------------------------------------------------------------------------------------------------- events
EVENTS = tuple(f"child_span_{t}" for t in THRESHOLDS) + ("big_leaf", "cost_leaf_20", "m_1", "m_span_minus_1", "m_multiple_of_64", "non_finite_costs")
DEPTHS = ("depth_above_256", "depth_below_subtree_root")


def tree_shape(nodes):
    """per node: (first, triangles, depth) from leaf first / span and sums over the children (children stand behind their parent)"""
    nodes = np.asarray(nodes)
    n = len(nodes)
    first, total, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in range(n - 1, -1, -1):
        if nodes[k, 7]:
            first[k], total[k] = nodes[k, 6], nodes[k, 7]
        else:
            l = int(nodes[k, 6])
            first[k], total[k] = first[l], total[l] + total[l + 1]
    for k in range(n):
        if not nodes[k, 7]:
            depth[nodes[k, 6]] = depth[nodes[k, 6] + 1] = depth[k] + 1
    return first, total, depth


def _a_bin_split_does_it(cent, m):
    """Is `first m left, the rest right` what one of the 3 x 19 split positions of the node's own bins gives? Then a split that also
    separates the signs of x proves nothing about the costs."""
    with np.errstate(all="ignore"):
        for axis in range(3):
            c = cent[:, axis]
            bmin = c.min()
            bsize = c.max() - bmin
            for i in range(19):
                left = c < bmin + bsize * (F(i + 1) / F(20))
                if left[:m].all() and not left[m:].any():
                    return True
    return False


def tree_events(nodes, idx, pos, faces):
    """-> (set of EVENTS this tree meets, {depth name: value})"""
    nodes = np.asarray(nodes)
    first, total, depth = tree_shape(nodes)
    inner = np.nonzero(nodes[:, 7] == 0)[0]
    met = set()
    spans = set(int(v) for v in total[1:])
    for t in THRESHOLDS:
        if t in spans:
            met.add(f"child_span_{t}")
    if (nodes[:, 7] > MAX_LEAF).any():
        met.add("big_leaf")
    cent_all = centroids(pos, faces)[np.asarray(idx).astype(np.int64)]
    for k in np.nonzero(nodes[:, 7] == MAX_LEAF)[0]:             # a leaf of exactly 20 triangles that a split could have divided
        if len(np.unique(cent_all[int(nodes[k, 6]):int(nodes[k, 6]) + MAX_LEAF], axis=0)) > 1:
            met.add("cost_leaf_20")
            break
    m = total[nodes[inner, 6].astype(np.int64)] if len(inner) else np.zeros(0, np.int64)
    if (m == 1).any():
        met.add("m_1")
    if (m == total[inner] - 1).any():
        met.add("m_span_minus_1")
    if (m % 64 == 0).any():
        met.add("m_multiple_of_64")
    # a node whose costs were all non-finite: its split is `c < 0` on axis 0 (recognised by the children's ranges), or it stayed a
    # leaf of more than 20 triangles
    if "big_leaf" in met:
        met.add("non_finite_costs")
    else:
        cent = cent_all
        neg = np.concatenate([[0], np.cumsum(cent[:, 0] < 0)])
        for k, mm in zip(inner, m):
            a, mm, b = int(first[k]), int(mm), int(first[k] + total[k])
            if neg[a + mm] - neg[a] == mm and neg[b] - neg[a + mm] == 0 and not _a_bin_split_does_it(cent[a:b], mm):
                met.add("non_finite_costs")
                break
    # the part of the tree the level kernels build, and the subtrees one wave finishes (k_subtree)
    above = total > LOCAL_SPAN
    depths = {"depth_above_256": int(depth[above].max()) + 1 if above.any() else 0}
    below = np.zeros(len(nodes), np.int64)                       # height below each node
    for k in range(len(nodes) - 1, -1, -1):
        if not nodes[k, 7]:
            l = int(nodes[k, 6])
            below[k] = 1 + max(below[l], below[l + 1])
    depths["depth_below_subtree_root"] = int(below[~above].max()) if (~above).any() else 0
    return met, depths


def count_events(trees):
    """trees: {group: [(nodes, idx, pos, faces), ...]} -> {group: {event: cases that meet it, depth: maximum}}"""
    out = {}
    for group, items in trees.items():
        c = {e: 0 for e in EVENTS}
        d = {e: 0 for e in DEPTHS}
        for nodes, idx, pos, faces in items:
            met, depths = tree_events(nodes, idx, pos, faces)
            for e in met:
                c[e] += 1
            for e, v in depths.items():
                d[e] = max(d[e], v)
        out[group] = {**c, **d}
    return out
