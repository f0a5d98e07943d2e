"""Aimed inputs for the two builders of the top-level hierarchy (host_scene.hpp::buildTopLevel; csrc/tlas_build.hpp and
csrc/tlas_build_kernels.inc), shared by tests/test_tlas_build_host.py and tests/test_tlas_build.py. Plain NumPy.

A case is (kind, leaves, mesh (n,) int32, node_world (n, 8) float32: lo.xyz, lo.w, hi.xyz, hi.w). Mesh-less nodes are interleaved
with the mesh nodes in every case (the leaf ids are never one contiguous range), carry boxes of 1e30 that nothing may read, and pad
the cases of fewer than 64 leaves to 64 nodes and more. The .w words hold a pattern the builders ignore.

LEAF COUNTS: the smallest trees, the counts around 64, and around cap = kTlasLocalLeaves the counts at which the top levels hand over
to the subtrees and sibling ranges differ by one leaf.

KINDS (every kind at every leaf count, so each is met by 16 cases; `counts()` checks at least 8):
  random      random boxes
  equal       every centre equal (boxes of power-of-two half extents around one point): the node index decides every split
  lattice     centres on a lattice of 4 values per axis: many ties inside a range
  axis_tie    centres (x, -x, z / 4): the two widest axes have the same extent in every range, the lower axis wins — and sorting by
              y instead would reverse the halves
  inf_extent  centres up to +-3.2e38 on x and y: cmax - cmin overflows to +inf on both
  nonfinite   a quarter of the boxes each with lo = -inf, hi = +inf (NaN centre), lo = hi = +inf, lo + hi overflowing — all count as
              0 —, among finite boxes around 0
  zeros       a group of boxes that are -0 on every bound (centre -0) next to boxes with lo = -1, hi = 1 (centre +0), among others

No bound (lo or hi of an axis) carries +0 on one leaf and -0 on another in any case: there buildTopLevel's boxes depend on the inner
order of std::nth_element. `check_signed_zero_rule` asserts that of every case made here."""
import struct

import numpy as np

KINDS = ["random", "equal", "lattice", "axis_tie", "inf_extent", "nonfinite", "zeros"]
MAGIC = 0x31534C54          # 'TLS1'


def leaf_counts(cap):
    return [1, 2, 3, 4, 5, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap, 2 * cap + 1, 4 * cap + 3, 8 * cap + 5]


def _boxes(kind, n, rng):
    """-> (lo, hi) of n leaves, (n, 3) float32 each"""
    f = np.float32
    if kind == "random":
        lo = rng.uniform(-10, 10, (n, 3)).astype(f)
        return lo, (lo + rng.uniform(0.01, 2, (n, 3)).astype(f)).astype(f)
    if kind == "equal":
        c = np.array([1.0, 2.0, 3.0], f)
        e = np.exp2(-rng.integers(1, 6, (n, 3))).astype(f)          # c -+ e and their sum are exact
        return (c - e).astype(f), (c + e).astype(f)
    if kind == "lattice":
        c = (rng.integers(0, 4, (n, 3)) - 1.5).astype(f)
        return (c - f(0.25)).astype(f), (c + f(0.25)).astype(f)
    if kind == "axis_tie":
        x = rng.integers(1, 4096, n).astype(f) / f(8)               # exact in binary32, as are -x, x / 4 and the half sums
        c = np.stack([x, -x, x / f(4)], 1).astype(f)
        return c.copy(), c.copy()
    if kind == "inf_extent":
        c = rng.uniform(-3.2e38, 3.2e38, (n, 3)).astype(f)
        c[:, 2] = rng.uniform(1, 9, n).astype(f)
        if n > 1:
            c[0, :2], c[1, :2] = f(3.2e38), f(-3.2e38)
        return c.copy(), c.copy()
    if kind == "nonfinite":
        lo = rng.uniform(-5, 5, (n, 3)).astype(f)
        lo[lo == 0] = f(0.5)
        hi = (lo + f(0.25)).astype(f)
        hi[hi == 0] = f(0.125)
        which = rng.integers(0, 4, n)
        axis = rng.integers(0, 3, n)
        for i in range(n):
            if which[i] == 1:
                lo[i, axis[i]], hi[i, axis[i]] = -np.inf, np.inf
            elif which[i] == 2:
                lo[i, axis[i]] = hi[i, axis[i]] = np.inf
            elif which[i] == 3:
                lo[i, axis[i]] = hi[i, axis[i]] = f(3e38)
        return lo, hi
    if kind == "zeros":
        lo = rng.uniform(-3, 3, (n, 3)).astype(f)
        lo[lo == 0] = f(0.5)
        hi = (lo + f(0.5)).astype(f)
        hi[hi == 0] = f(0.125)
        which = rng.integers(0, 3, n)
        lo[which == 1], hi[which == 1] = f(-0.0), f(-0.0)
        lo[which == 2], hi[which == 2] = f(-1.0), f(1.0)
        return lo, hi
    raise KeyError(kind)


def make_case(kind, leaves, seed):
    rng = np.random.default_rng(seed)
    n = max(64, leaves + leaves // 4 + 2)
    ids = np.sort(rng.choice(np.arange(1, n), leaves, replace=False))     # node 0 is never a mesh node
    if leaves > 1 and ids[-1] - ids[0] == leaves - 1:                       # contiguous by chance: open a gap
        if ids[-1] != n - 1:
            ids[-1] = n - 1
        else:
            ids[0] -= 1                                                     # (n - leaves >= 2: still a node above 0)
    mesh = np.full(n, -1, np.int32)
    mesh[ids] = rng.integers(0, 5, leaves)
    world = np.full((n, 8), 1e30, np.float32)
    world[:, 3] = np.arange(n, dtype=np.float32)
    world[:, 7] = -7.0
    lo, hi = _boxes(kind, leaves, rng)
    world[ids, 0:3], world[ids, 4:7] = lo, hi
    return kind, leaves, mesh, world


def suite(cap, max_leaves=None):
    cases = []
    for ki, kind in enumerate(KINDS):
        for li, leaves in enumerate(leaf_counts(cap)):
            if max_leaves is None or leaves <= max_leaves:
                cases.append(make_case(kind, leaves, 1000 * ki + li))
    return cases


def counts(cases):
    out = {k: 0 for k in KINDS}
    for kind, _, _, _ in cases:
        out[kind] += 1
    return out


def check_signed_zero_rule(cases):
    for kind, leaves, mesh, world in cases:
        ids = np.flatnonzero(mesh >= 0)
        assert len(ids) == leaves and (leaves == 1 or ids[-1] - ids[0] > leaves - 1), (kind, leaves)
        bits = world[ids].view(np.uint32)
        for col in (0, 1, 2, 4, 5, 6):
            assert not ((bits[:, col] == 0).any() and (bits[:, col] == 0x80000000).any()), (kind, leaves, col)


def save(cases, path):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC, len(cases)))
        for kind, leaves, mesh, world in cases:
            f.write(struct.pack("<III", KINDS.index(kind), leaves, len(mesh)))
            f.write(np.ascontiguousarray(mesh, np.int32).tobytes())
            f.write(np.ascontiguousarray(world, np.float32).tobytes())
