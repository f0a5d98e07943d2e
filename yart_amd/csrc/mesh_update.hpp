// mesh_update.hpp — the per-record arithmetic of yart_hip_scene_update_meshes: what host_scene.hpp::buildHostImage derives from one
// mesh's BVH (node array + index permutation, as either builder returns them) and its vertices, stated per record so that the
// kernels (mesh_update_kernels.inc) and the host (a mesh the device build refuses, tests/meshupdatesim) run the same operations.
// buildHostImage itself is not written on top of this header: scene creation keeps its code, and the tests compare the two byte
// for byte.
//
//   muLeafRecord      the LeafTri of leaf position k: p0, e1 = p1 - p0, e2 = p2 - p0 of triangle indices[k], its ShadeTri index,
//                     material, and the material's MAT_HAS_ALPHA | MAT_TRANSPARENT
//   muLinkWord        a node's link word: the reference's index | alpha bit | saturated span. buildHostImage finds the alpha bit
//                     bottom-up; a node's triangles are one range [first, first + span) of the leaf order, so the bit is "the range
//                     holds a record with MAT_HAS_ALPHA": a difference of two entries of a prefix sum over the leaf records
//   muLongSpanWord    what a leaf's first record carries besides its material flags: the true span (traverse.hpp::leafSpan)
//   muDeriveHost      all of it for one mesh on the host, with the ranges of the inner nodes and the stack need found by sweeps
//                     over the node array (children are allocated after their parent)
//   muVertexBox       the box of a mesh's vertices with create's Bounds3::expand (exact in the sign of zeros)
#pragma once
#include <stdexcept>
#include <vector>

#include "bvh_build.hpp"
#include "scene_types.hpp"
#include "scene_update.hpp"

namespace yart_hip {

YART_HD void muLeafRecord(LeafTri& lt, const float* p0, const float* p1, const float* p2, uint32_t shadeTri, uint32_t material, uint32_t materialFlags) {
  for (int c = 0; c < 3; c++) { lt.p0[c] = p0[c]; lt.e1[c] = p1[c] - p0[c]; lt.e2[c] = p2[c] - p0[c]; }
  lt.triIdx = shadeTri;
  lt.material = material;
  lt.matFlags = materialFlags & (MAT_HAS_ALPHA | MAT_TRANSPARENT);
}

// index: the builder's leftFirst (left child / first leaf position); span: the builder's (0 for an inner node)
YART_HD uint32_t muLinkWord(uint32_t index, uint32_t span, bool alphaInRange) {
  return index | (alphaInRange ? kLinkAlphaBit : 0u) | ((span < kSpanBig ? span : kSpanBig) << kSpanShift);
}
YART_HD uint32_t muLongSpanWord(uint32_t span) { return span << kLeafSpanShift; }
YART_HD bool muLeafSpanFits(uint32_t span) { return span < (1u << (32 - kLeafSpanShift)); }

// One mesh on the host. nodes / indices: a builder's output (plain leftFirst); positions: 3 floats per vertex; triVerts: the mesh's
// faces (x, y, z vertices, w material); materialFlags: MaterialDev::flags per material. Writes nNodes link-word nodes into nodesOut
// (bounds and span copied), nTris records into leafOut; returns the root's alpha flag and the stack need.
struct MuDerived { uint32_t hasAlpha, stackNeed; };
inline MuDerived muDeriveHost(const BvhNode* nodes, uint32_t nNodes, const uint32_t* indices, uint32_t nTris, const float* positions,
                              const u4* triVerts, uint32_t triOffset, const uint32_t* materialFlags, BvhNode* nodesOut, LeafTri* leafOut) {
  std::vector<uint32_t> prefix(size_t(nTris) + 1u, 0u);
  for (uint32_t k = 0; k < nTris; k++) {
    const uint32_t t = indices[k];
    const u4 tv = triVerts[t];
    muLeafRecord(leafOut[k], positions + size_t(tv.x) * 3, positions + size_t(tv.y) * 3, positions + size_t(tv.z) * 3, triOffset + t, tv.w,
                 materialFlags[tv.w]);
    prefix[k + 1u] = prefix[k] + ((leafOut[k].matFlags & MAT_HAS_ALPHA) ? 1u : 0u);
  }
  // ranges bottom-up, depths top-down: a child's index is larger than its parent's
  std::vector<uint32_t> first(nNodes), count(nNodes), depth(nNodes, 0u);
  for (uint32_t n = nNodes; n-- > 0u;) {
    if (nodes[n].span > 0u) { first[n] = nodes[n].leftFirst; count[n] = nodes[n].span; }
    else {
      const uint32_t l = nodes[n].leftFirst;
      if (l <= n || l + 1u >= nNodes) throw std::invalid_argument("bvh: child link does not point behind its node");
      first[n] = first[l]; count[n] = count[l] + count[l + 1u];
    }
  }
  MuDerived d{0u, 0u};
  for (uint32_t n = 0; n < nNodes; n++) {
    const BvhNode& bn = nodes[n];
    const bool alpha = prefix[first[n] + count[n]] != prefix[first[n]];
    nodesOut[n] = bn;
    nodesOut[n].leftFirst = muLinkWord(bn.leftFirst, bn.span, alpha);
    if (bn.span > 0u) {
      if (!muLeafSpanFits(bn.span)) throw std::invalid_argument("mesh: a BVH leaf of 2^24 or more triangles is not supported");
      leafOut[bn.leftFirst].matFlags |= muLongSpanWord(bn.span);
      d.stackNeed = depth[n] > d.stackNeed ? depth[n] : d.stackNeed;     // need(root) = the most inner nodes above a leaf
    } else {
      depth[bn.leftFirst] = depth[bn.leftFirst + 1u] = depth[n] + 1u;
    }
    if (n == 0u) d.hasAlpha = alpha ? 1u : 0u;
  }
  return d;
}

// create's vertex box (Node(Mesh*), scene.hpp:17-22): Bounds3::expand over the vertices in order
inline SuBox muVertexBox(const float* positions, uint32_t nVerts) {
  Bounds3 vb;
  for (uint32_t v = 0; v < nVerts; v++) vb.expand(positions + size_t(v) * 3);
  SuBox sb;
  for (int c = 0; c < 3; c++) { sb.mn[c] = vb.mn[c]; sb.mx[c] = vb.mx[c]; }
  return sb;
}

}  // namespace yart_hip
