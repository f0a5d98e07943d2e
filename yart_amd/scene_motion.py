"""Per-pixel motion of a scene between two frames (``yart_hip_scene_pixel_motion_*``) stated in NumPy.

:func:`scene_motion_reference` is written from the definition in the header comment of ``include/yart_hip.h``: the nodes' composed
transforms in float64 with explicit element-wise sums (no ``@``, which may fuse), then every pixel in float32, every operation in
the order the definition gives. It is what the tests hold the device kernels (and ``csrc/scene_motion.hpp`` compiled for the host)
to, bit for bit. Only + - * /, sqrt (correctly rounded) and comparisons.

The records it returns — (H, W, 8) float32: ``{P'.xyz, kind}``, ``{n'.xyz, 0}``, kind a uint32 stored as bits — are what
``TemporalAccumulator.accumulate(..., pixel_motion=)`` and ``temporal_reference(..., pixel_motion=)`` take.
"""
from __future__ import annotations

import numpy as np

from .temporal import _cross, _dot

RECORD_WORDS = 8
KIND_WORD = 3
KIND_STATIC, KIND_MOVED = 0, 1

_F = np.float32


def _node_field(node, name, index):
    """a field of a node: an attribute, a key (a dict, or a record of api.NODE_DTYPE), or position ``index`` of a tuple"""
    if isinstance(node, dict) or (isinstance(node, np.void) and node.dtype.names):
        return node[name]
    return getattr(node, name) if hasattr(node, name) else node[index]


def _rows(node, name, index):
    """the top three rows of a node's 4 x 4 ``fwd`` / ``inv`` as float32 (3, 4)"""
    return np.asarray(_node_field(node, name, index), _F).reshape(4, 4)[:3].copy()


def _mul(a, b):
    """a · b for 3 x 4 float64 matrices with the implied last row (0, 0, 0, 1): each element (a0 * b0 + a1 * b1) + a2 * b2, and
    + a3 (the word times 1) in the last column"""
    out = np.empty((3, 4), np.float64)
    for i in range(3):
        for j in range(4):
            s = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
            if j == 3:
                s = s + a[i, 3]
            out[i, j] = s
    return out


def node_chains(nodes_prev, nodes_cur):
    """Per node (Wc, Ac, Wp, Ap) as float32 (n, 4, 3, 4), ``changed`` (n,) bool and ``mesh`` (n,) int: the composed transforms of
    the current and the previous node list — W = fwd_root · … · fwd_node, A = inv_node · … · inv_root, in float64 by a walk from the
    node to the root, rounded at the end — and whether a fwd / inv word on the node's chain differs between the lists.
    A node is anything with ``parent``, ``mesh``, ``fwd`` and ``inv`` (attributes or keys)."""
    n = len(nodes_cur)
    assert len(nodes_prev) == n, "the two frames' scenes do not have the same nodes"
    mats = np.zeros((n, 4, 3, 4), _F)
    changed = np.zeros(n, bool)
    mesh = np.zeros(n, np.int64)
    for i in range(n):
        mesh[i] = int(_node_field(nodes_cur[i], "mesh", 1))
        for f, nodes in enumerate((nodes_cur, nodes_prev)):
            k = i
            w = _rows(nodes[k], "fwd", 2).astype(np.float64)
            a = _rows(nodes[k], "inv", 3).astype(np.float64)
            k = int(_node_field(nodes[k], "parent", 0))
            while k >= 0:
                w = _mul(_rows(nodes[k], "fwd", 2).astype(np.float64), w)
                a = _mul(a, _rows(nodes[k], "inv", 3).astype(np.float64))
                k = int(_node_field(nodes[k], "parent", 0))
            mats[i, 2 * f], mats[i, 2 * f + 1] = w.astype(_F), a.astype(_F)
        k = i
        while k >= 0:
            for name, idx in (("fwd", 2), ("inv", 3)):
                c = np.asarray(_node_field(nodes_cur[k], name, idx), _F).reshape(16).view(np.uint32)
                p = np.asarray(_node_field(nodes_prev[k], name, idx), _F).reshape(16).view(np.uint32)
                changed[i] |= bool((c != p).any())
            assert int(_node_field(nodes_cur[k], "parent", 0)) == int(_node_field(nodes_prev[k], "parent", 0))
            k = int(_node_field(nodes_cur[k], "parent", 0))
    return mats, changed, mesh


def _point(m, p):
    return np.stack([_dot(m[..., i, :3], p) + m[..., i, 3] for i in range(3)], -1).astype(_F)


def _lin_t(m, v):
    return np.stack([_dot(m[..., :3, j], v) for j in range(3)], -1).astype(_F)


def scene_motion_reference(nodes_prev, nodes_cur, meshes, positions_prev, positions_cur, position, normal, coverage, ids):
    """``nodes_prev`` / ``nodes_cur``: the node lists of the previous and the current frame (``yscn.Scene.nodes``, or records with
    parent / mesh / fwd / inv); ``meshes``: per mesh its faces, (n_tris, >= 3) vertex ids (a ``yscn.Mesh`` will do);
    ``positions_prev`` / ``positions_cur``: per mesh its (n_verts, >= 3) float32 vertex positions in the two frames; ``position`` /
    ``normal`` (H, W, 3), ``coverage`` (H, W), ``ids`` (H, W, 4) int32: the feature buffers of the current frame.
    Returns the records, (H, W, 8) float32."""
    P = np.asarray(position, _F)
    h, w = P.shape[:2]
    n = np.asarray(normal, _F).reshape(h, w, 3)
    coverage = np.asarray(coverage, _F).reshape(h, w)
    ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(h, w, 4)).view(np.uint32)
    node, tri = ids[..., 0], ids[..., 3]
    mats, changed, node_mesh = node_chains(nodes_prev, nodes_cur)
    faces = [np.asarray(getattr(m, "faces", m)).reshape(len(getattr(m, "faces", m)), -1)[:, :3].astype(np.int64) for m in meshes]
    n_tris = np.array([len(f) for f in faces] + [0], np.int64)
    cur = [np.asarray(v, _F)[:, :3] for v in positions_cur]
    prev = [np.asarray(v, _F)[:, :3] for v in positions_prev]
    with np.errstate(all="ignore"):
        ok = (coverage == _F(1.0)) & np.isfinite(P).all(-1) & np.isfinite(n).all(-1) & (node < np.uint32(len(nodes_cur)))
        nd = np.where(ok, node, 0).astype(np.int64)
        mesh = node_mesh[nd]
        ok &= mesh >= 0
        ok &= tri < n_tris[np.where(ok, mesh, -1)].astype(np.uint32)
        # the triangle's vertices in both frames, gathered per pixel
        tc, tp = np.zeros((h, w, 3, 3), _F), np.zeros((h, w, 3, 3), _F)
        for m in np.unique(mesh[ok]):
            sel = ok & (mesh == m)
            v = faces[m][tri[sel].astype(np.int64)]
            tc[sel], tp[sel] = cur[m][v], prev[m][v]
        same = (tc.view(np.uint32) == tp.view(np.uint32)).all((-1, -2))
        moved = ok & ~(~changed[nd] & same)
        M = mats[nd]
        a, b, c = tc[..., 0, :], tc[..., 1, :], tc[..., 2, :]
        a_, b_, c_ = tp[..., 0, :], tp[..., 1, :], tp[..., 2, :]
        po = _point(M[..., 1, :, :], P)
        e1, e2, r = (b - a).astype(_F), (c - a).astype(_F), (po - a).astype(_F)
        d11, d12, d22, r1, r2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(r, e1), _dot(r, e2)
        det = d11 * d22 - d12 * d12
        u = (d22 * r1 - d12 * r2) / det
        v = (d11 * r2 - d12 * r1) / det
        f1, f2 = (b_ - a_).astype(_F), (c_ - a_).astype(_F)
        p_ = ((a_ + u[..., None] * f1) + v[..., None] * f2).astype(_F)
        Pq = _point(M[..., 2, :, :], p_)
        no = _lin_t(M[..., 0, :, :], n)
        g11, g12, g22 = _dot(f1, f1), _dot(f1, f2), _dot(f2, f2)
        gdet = g11 * g22 - g12 * g12
        D1 = ((g22[..., None] * f1 - g12[..., None] * f2) / gdet[..., None]).astype(_F)
        D2 = ((g11[..., None] * f2 - g12[..., None] * f1) / gdet[..., None]).astype(_F)
        N, N_ = _cross(e1, e2), _cross(f1, f2)
        gamma = _dot(no, N) / np.sqrt(_dot(N, N) * _dot(N_, N_))
        no_ = ((_dot(no, e1)[..., None] * D1 + _dot(no, e2)[..., None] * D2) + gamma[..., None] * N_).astype(_F)
        nq = _lin_t(M[..., 3, :, :], no_)
    rec = np.zeros((h, w, RECORD_WORDS), _F)
    rec[..., 0:3] = np.where(moved[..., None], Pq, _F(0))
    rec[..., 4:7] = np.where(moved[..., None], nq, _F(0))
    rec.view(np.uint32)[..., KIND_WORD] = np.where(moved, KIND_MOVED, KIND_STATIC)
    return rec
