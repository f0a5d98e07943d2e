// tlas_build.hpp — host_scene.hpp::buildTopLevel restated level by level, so that kernels (tlas_build_kernels.inc) can build the
// top-level hierarchy with the recursive builder's bytes. What the restatement rests on:
//
//   the shape   With L mesh nodes the tree has 2L - 1 records. A range [lo, hi) of leaf positions splits at mid = lo + (hi - lo) / 2,
//               the children pair of the k-th inner node in pre-order lies at 1 + 2k: ranges, levels, the inner nodes' `a`, every
//               `b` and the height depend on L alone (TlasShape, O(L) on the host, once per leaf count).
//   a split     is a selection under a strict total order — (centre on the axis, node index) —, so its result does not depend on
//               what std::nth_element does inside: the lower half of a range holds its mid - lo smallest ids. The centre is
//               0.5f * (lo + hi) in binary32, 0.0f where that is not finite; -0 and +0 compare equal; equal centres are ordered by
//               node index. tlasOrdKey maps a centre to an integer of the same order with both zeros alike.
//   the axis    has the largest cmax - cmin of those centres over the range; the comparison is strict, the lowest axis wins a tie.
//               The extent can be +inf, never a NaN.
//   one key     (segment number : 12 bits, tlasOrdKey(centre) : 32 bits, node index : 20 bits) does a whole level: segments are
//               contiguous and numbered in position order, so sorting a whole array of such keys leaves every element inside its
//               segment. Sorting a segment completely is more than the selection asks for and gives the same two halves.
//   the boxes   are the min / max fold of the leaves' nodeWorld boxes, order-free (but for a bound that carries +0 on one leaf and
//               -0 on another: there the recursive builder's result depends on nth_element's inner order; padded world boxes of
//               scenes do not do that). A bound that is a NaN is outside the contract as well.
//
// The build runs in two phases. Levels on which a range holds more than kTlasLocalLeaves leaves ("top levels") sort the whole leaf
// array once per level; then every range of at most kTlasLocalLeaves leaves whose parent is larger (a "subtree root") is finished on
// its own, all of its remaining levels — on the device by one workgroup in LDS. tlasBuildLevelwise is the host statement of exactly
// that; tests/tlassim compares it with buildTopLevel.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "scene_types.hpp"

namespace yart_hip {

constexpr uint32_t kTlasMinNodes = 64;                 // scenes of fewer nodes have no top-level hierarchy
constexpr uint32_t kTlasMaxNodes = 1u << 20;           // the key's node field
constexpr uint32_t kTlasLocalLeaves = 2048;            // 2048 keys of 8 bytes: 16 KB of LDS
constexpr uint32_t kTlasLeafMark = 0x80000000u;        // TlasShape::recA of a leaf record: the mark, and the leaf's position

YART_HD uint32_t tlasOrdKey(float v) {                 // order-preserving map float -> uint32, both zeros alike
  uint32_t b = __builtin_bit_cast(uint32_t, v == 0.0f ? 0.0f : v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
YART_HD float tlasOrdVal(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __builtin_bit_cast(float, b);
}
// the centre of node n's world box on axis c, as buildTopLevel takes it
YART_HD float tlasCentre(const f4* nodeWorld, uint32_t n, int c) {
  const f4 lo = nodeWorld[size_t(n) * 2u], hi = nodeWorld[size_t(n) * 2u + 1u];
  const float v = 0.5f * (c == 0 ? lo.x + hi.x : c == 1 ? lo.y + hi.y : lo.z + hi.z);
  return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u ? v : 0.0f;
}
// the split axis of a range from the smallest and largest key of its centres per axis
YART_HD int tlasAxis(const uint32_t* kmin, const uint32_t* kmax) {
  int axis = 0;
  float best = tlasOrdVal(kmax[0]) - tlasOrdVal(kmin[0]);
  for (int c = 1; c < 3; c++) {
    const float e = tlasOrdVal(kmax[c]) - tlasOrdVal(kmin[c]);
    if (e > best) { best = e; axis = c; }
  }
  return axis;
}
YART_HD unsigned long long tlasKey(uint32_t segment, uint32_t centreKey, uint32_t node) {
  return ((unsigned long long) segment << 52) | ((unsigned long long) centreKey << 20) | (unsigned long long) node;
}
constexpr uint32_t kTlasKeyNodeMask = 0xfffffu;

// The range position p lies in, `depth` levels below the range [lo, hi), and that range's number among the ranges of its level in
// position order (a range of one leaf stays as it is)
struct TlasSegment { uint32_t lo, hi, ord; };
YART_HD TlasSegment tlasSegmentOf(uint32_t lo, uint32_t hi, uint32_t depth, uint32_t p) {
  TlasSegment s{lo, hi, 0u};
  for (uint32_t d = 0; d < depth; d++) {
    s.ord <<= 1;
    if (s.hi - s.lo > 1u) {
      const uint32_t mid = s.lo + (s.hi - s.lo) / 2u;
      if (p < mid) s.hi = mid; else { s.lo = mid; s.ord |= 1u; }
    }
  }
  return s;
}
// the largest range `depth` levels below a range of n leaves (the upper halves take the odd leaf)
YART_HD uint32_t tlasLargestRange(uint32_t n, uint32_t depth) {
  for (uint32_t d = 0; d < depth && n > 1u; d++) n -= n / 2u;
  return n;
}

// What depends on the leaf count alone
struct TlasShape {
  uint32_t leaves = 0, height = 0;
  uint32_t topLevels = 0;                       // levels 0 .. topLevels - 1 hold a range of more than kTlasLocalLeaves leaves
  std::vector<uint32_t> recA;                   // per record: an inner node's `a`, or kTlasLeafMark | the leaf's position
  std::vector<uint32_t> order, first;           // the records by level; first[l] .. first[l + 1]: level l (height + 2 entries)
  std::vector<uint32_t> rootLo, rootHi;         // the subtree roots' ranges
  uint32_t records() const { return uint32_t(recA.size()); }
};
inline TlasShape tlasShape(uint32_t leaves) {
  TlasShape s;
  s.leaves = leaves;
  if (!leaves) return s;
  s.recA.assign(size_t(leaves) * 2u - 1u, 0u);
  std::vector<uint32_t> level(s.recA.size(), 0u);
  struct Item { uint32_t at, lo, hi, level, parentSize; };
  std::vector<Item> stack{{0u, 0u, leaves, 0u, 0xffffffffu}};
  uint32_t used = 1;
  while (!stack.empty()) {                      // pre-order, as the recursion allocates the children pairs
    const Item it = stack.back();
    stack.pop_back();
    const uint32_t n = it.hi - it.lo;
    s.height = std::max(s.height, it.level);
    level[it.at] = it.level;
    if (n > kTlasLocalLeaves) s.topLevels = std::max(s.topLevels, it.level + 1u);
    else if (it.parentSize > kTlasLocalLeaves) { s.rootLo.push_back(it.lo); s.rootHi.push_back(it.hi); }
    if (n == 1u) { s.recA[it.at] = kTlasLeafMark | it.lo; continue; }
    const uint32_t mid = it.lo + n / 2u;
    s.recA[it.at] = used;
    stack.push_back({used + 1u, mid, it.hi, it.level + 1u, n});
    stack.push_back({used, it.lo, mid, it.level + 1u, n});
    used += 2u;
  }
  s.first.assign(size_t(s.height) + 2u, 0u);
  for (uint32_t l : level) s.first[l + 1u]++;
  for (size_t l = 0; l + 1u < s.first.size(); l++) s.first[l + 1u] += s.first[l];
  s.order.resize(s.recA.size());
  std::vector<uint32_t> at(s.first.begin(), s.first.end() - 1);
  for (uint32_t k = 0; k < s.records(); k++) s.order[at[level[k]]++] = k;
  return s;
}

// The leaf positions' first order: the mesh nodes, ascending
inline std::vector<uint32_t> tlasLeafIds(const int32_t* mesh, uint32_t nNodes) {
  std::vector<uint32_t> ids;
  if (nNodes >= kTlasMinNodes)
    for (uint32_t i = 0; i < nNodes; i++) if (mesh[i] >= 0) ids.push_back(i);
  return ids;
}

// One level of the range [lo, hi) of `ids`, `depth` levels below it: per range of that level the centres' extents, the axis, the
// keys; one sort of the whole range.
inline void tlasSortLevel(const f4* nodeWorld, uint32_t* ids, uint32_t lo, uint32_t hi, uint32_t depth) {
  const uint32_t n = hi - lo;
  std::vector<uint32_t> kmin(size_t(3) << depth, 0xffffffffu), kmax(size_t(3) << depth, 0u);
  for (uint32_t p = 0; p < n; p++) {
    const TlasSegment sg = tlasSegmentOf(0u, n, depth, p);
    for (int c = 0; c < 3; c++) {
      const uint32_t k = tlasOrdKey(tlasCentre(nodeWorld, ids[lo + p], c));
      kmin[sg.ord * 3u + c] = std::min(kmin[sg.ord * 3u + c], k); kmax[sg.ord * 3u + c] = std::max(kmax[sg.ord * 3u + c], k);
    }
  }
  std::vector<unsigned long long> keys(n);
  for (uint32_t p = 0; p < n; p++) {
    const TlasSegment sg = tlasSegmentOf(0u, n, depth, p);
    const uint32_t node = ids[lo + p];
    const int axis = tlasAxis(&kmin[sg.ord * 3u], &kmax[sg.ord * 3u]);
    keys[p] = tlasKey(sg.ord, sg.hi - sg.lo > 1u ? tlasOrdKey(tlasCentre(nodeWorld, node, axis)) : 0u, node);
  }
  std::sort(keys.begin(), keys.end());
  for (uint32_t p = 0; p < n; p++) ids[lo + p] = uint32_t(keys[p]) & kTlasKeyNodeMask;
}

// The records from the sorted leaves: links from the shape, boxes level by level from the deepest (a leaf takes its node's world
// box, an inner node the min / max of its two children: scene_update_kernels.inc's refit)
inline void tlasEmit(const TlasShape& s, const f4* nodeWorld, const uint32_t* ids, TlasNode* tlas) {
  for (uint32_t l = s.height + 1u; l-- > 0u;)
    for (uint32_t k = s.first[l]; k < s.first[l + 1u]; k++) {
      TlasNode& t = tlas[s.order[k]];
      const uint32_t a = s.recA[s.order[k]];
      if (a & kTlasLeafMark) {
        t.a = ids[a & ~kTlasLeafMark]; t.b = 1u;
        const f4 lo = nodeWorld[size_t(t.a) * 2u], hi = nodeWorld[size_t(t.a) * 2u + 1u];
        t.lo[0] = lo.x; t.lo[1] = lo.y; t.lo[2] = lo.z; t.hi[0] = hi.x; t.hi[1] = hi.y; t.hi[2] = hi.z;
      } else {
        t.a = a; t.b = 0u;
        const TlasNode& x = tlas[a]; const TlasNode& y = tlas[a + 1u];
        for (int c = 0; c < 3; c++) { t.lo[c] = stdmin(x.lo[c], y.lo[c]); t.hi[c] = stdmax(x.hi[c], y.hi[c]); }
      }
    }
}

// buildTopLevel, level by level; returns the height. mesh: per node, < 0 = not a mesh node.
inline uint32_t tlasBuildLevelwise(const int32_t* mesh, uint32_t nNodes, const f4* nodeWorld, std::vector<TlasNode>& tlas) {
  std::vector<uint32_t> ids = tlasLeafIds(mesh, nNodes);
  tlas.clear();
  if (ids.empty()) return 0u;
  const TlasShape s = tlasShape(uint32_t(ids.size()));
  for (uint32_t d = 0; d < s.topLevels; d++) tlasSortLevel(nodeWorld, ids.data(), 0u, s.leaves, d);
  for (size_t r = 0; r < s.rootLo.size(); r++)
    for (uint32_t d = 0; tlasLargestRange(s.rootHi[r] - s.rootLo[r], d) > 1u; d++) tlasSortLevel(nodeWorld, ids.data(), s.rootLo[r], s.rootHi[r], d);
  tlas.assign(s.records(), TlasNode{});
  tlasEmit(s, nodeWorld, ids.data(), tlas.data());
  return s.height;
}

}  // namespace yart_hip
