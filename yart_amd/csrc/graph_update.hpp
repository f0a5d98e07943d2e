// graph_update.hpp — the topology pass of yart_hip_scene_update_graph: what host_scene.hpp::buildHostImage derives from the node
// list's parent and mesh words alone, in one integer pass over the new list, so that the library (graph_update_kernels.inc) and the
// host simulator (tests/graphupdatesim) run the same statements. buildHostImage itself is not written on top of this header: scene
// creation keeps its code, and the tests compare the two byte for byte. Everything that depends on the transforms and the meshes'
// boxes stays scene_update.hpp's (k_su_scatter / k_su_fold / k_su_world on the device, suRederiveHost on the host).
//
//   GuTopo            the 16 bytes of topology per node the device is handed: parent, mesh, skip link, depth
//   guWorldWords      the two .w words of a node's nodeWorld pair: the bits of the pre-order subtree [i, skip) as a 64-bit mask below
//                     64 nodes; lo.w = skip, hi.w = 0 from 64 nodes on
//   guDerive          the pass: GuTopo per node, the deepest level, suIdentityFlags, the level tables of SceneUpdateTables by
//                     scene_update_kernels.inc::suBuildTables' rule (only for graphs of at most kSceneUpdateMaxLevels levels: deeper
//                     ones take suRederiveHost), the leaf list and the shape of the top-level hierarchy
//   guApplyNode       the topology fields of one NodeDev and the .w words of its pair: what k_gu_topology writes per lane, and
//                     guApplyHost over the arrays of a host image
//   guCapacity        the growth rule of every buffer a graph update may have to enlarge
#pragma once
#include <cstring>
#include <vector>

#include "scene_update.hpp"
#include "tlas_build.hpp"

namespace yart_hip {

constexpr uint32_t kGuMaxNodes = 1u << 20;             // wavefront.hpp::wfHitWord: node indices have 20 bits

struct GuTopo { int32_t parent, mesh; uint32_t skip, depth; };
static_assert(sizeof(GuTopo) == 16, "staged as four words per node");

YART_HD void guWorldWords(uint32_t i, uint32_t skip, uint32_t nNodes, uint32_t& loW, uint32_t& hiW) {
  if (nNodes < 64u) {                                  // (skip - i <= 63: the shifts are defined)
    const unsigned long long sub = ((1ull << (skip - i)) - 1ull) << i;
    loW = uint32_t(sub); hiW = uint32_t(sub >> 32);
  } else {
    loW = skip; hiW = 0u;
  }
}

struct GuDerived {
  std::vector<GuTopo> topo;
  std::vector<uint32_t> flags;                         // suIdentityFlags' words (NodeDev::pad[0])
  bool allIdentity = true;
  uint32_t maxNodeDepth = 0, levels = 0;
  // SceneUpdateTables: the children as a CSR list, the nodes with children by level (those of fanOut children and more first)
  std::vector<uint32_t> childOff, childIdx, parents, levelFirst, levelBig, levelSmall;
  std::vector<uint32_t> leafIds;                       // tlasLeafIds: the mesh nodes of a list of 64 nodes and more
  uint32_t tlasRecords = 0, tlasHeight = 0;            // 2 * leaves - 1 records (0 without leaves); the height of a median-split tree
};

// A buffer that has to hold `count` elements and does not is re-allocated for count + count / 2 + 64: a node list that grows by one
// node per frame re-allocates every log1.5 steps, not every frame. Buffers never shrink.
inline size_t guCapacity(size_t count) { return count + count / 2u + 64u; }

// The height of the top-level hierarchy over `leaves` leaves (TlasShape::height without building the shape)
inline uint32_t guTlasHeight(uint32_t leaves) {
  uint32_t h = 0;
  while (tlasLargestRange(leaves, h) > 1u) h++;
  return h;
}

// desc: nn >= 1 records in pre-order (node 0 the root, every other parent below its node's index): the caller has checked that.
// fanOut: scene_update_kernels.inc's kSuFanOut.
inline void guDerive(const YartNodeDesc* desc, uint32_t nn, uint32_t fanOut, GuDerived& g) {
  g.topo.assign(nn, GuTopo{});
  g.maxNodeDepth = 0;
  for (uint32_t i = 0; i < nn; i++) {
    g.topo[i].parent = desc[i].parent; g.topo[i].mesh = desc[i].mesh;
    g.topo[i].depth = i == 0 ? 0u : g.topo[desc[i].parent].depth + 1u;
    if (g.topo[i].depth > g.maxNodeDepth) g.maxNodeDepth = g.topo[i].depth;
  }
  // skip link: the first later node that is not in the subtree, with a stack of the open subtrees (host_scene.hpp)
  {
    std::vector<uint32_t> open;
    for (uint32_t i = 0; i < nn; i++) {
      while (!open.empty() && g.topo[open.back()].depth >= g.topo[i].depth) { g.topo[open.back()].skip = i; open.pop_back(); }
      open.push_back(i);
    }
    for (uint32_t k : open) g.topo[k].skip = nn;
  }
  g.flags.assign(nn, 0u);
  g.allIdentity = suIdentityFlags(desc, nn, g.flags.data());
  g.levels = g.maxNodeDepth + 1u;
  g.childOff.clear(); g.childIdx.clear(); g.parents.clear(); g.levelFirst.clear(); g.levelBig.clear(); g.levelSmall.clear();
  if (g.levels <= kSceneUpdateMaxLevels) {
    g.childOff.assign(size_t(nn) + 1u, 0u); g.childIdx.assign(nn - 1u, 0u);
    for (uint32_t i = 1; i < nn; i++) g.childOff[size_t(desc[i].parent) + 1u]++;
    for (uint32_t i = 0; i < nn; i++) g.childOff[i + 1u] += g.childOff[i];
    {
      std::vector<uint32_t> at(g.childOff.begin(), g.childOff.end() - 1);
      for (uint32_t i = 1; i < nn; i++) g.childIdx[at[desc[i].parent]++] = i;            // ascending within a parent
    }
    // parents by level, the big ones of a level first, ascending within each: two counting passes
    g.levelBig.assign(g.levels, 0u); g.levelSmall.assign(g.levels, 0u); g.levelFirst.assign(g.levels, 0u);
    for (uint32_t i = 0; i < nn; i++) {
      const uint32_t nc = g.childOff[i + 1u] - g.childOff[i];
      if (nc) (nc >= fanOut ? g.levelBig : g.levelSmall)[g.topo[i].depth]++;
    }
    uint32_t total = 0;
    for (uint32_t l = 0; l < g.levels; l++) { g.levelFirst[l] = total; total += g.levelBig[l] + g.levelSmall[l]; }
    g.parents.assign(total, 0u);
    std::vector<uint32_t> atBig(g.levelFirst), atSmall(g.levels);
    for (uint32_t l = 0; l < g.levels; l++) atSmall[l] = g.levelFirst[l] + g.levelBig[l];
    for (uint32_t i = 0; i < nn; i++) {
      const uint32_t nc = g.childOff[i + 1u] - g.childOff[i];
      if (nc) g.parents[(nc >= fanOut ? atBig : atSmall)[g.topo[i].depth]++] = i;
    }
    if (g.childIdx.empty()) g.childIdx.push_back(0u);                  // (never an empty upload)
    if (g.parents.empty()) g.parents.push_back(0u);
  }
  g.leafIds.clear();
  if (nn >= kTlasMinNodes)
    for (uint32_t i = 0; i < nn; i++) if (desc[i].mesh >= 0) g.leafIds.push_back(i);    // tlasLeafIds over the descriptors
  const uint32_t leaves = uint32_t(g.leafIds.size());
  g.tlasRecords = leaves ? 2u * leaves - 1u : 0u;
  g.tlasHeight = guTlasHeight(leaves);
}

// nodes / nodeWorld: nn records / pairs. The transforms, identity flags, boxes and the x, y, z of the pairs are scene_update.hpp's.
YART_HD void guApplyNode(const GuTopo& t, uint32_t i, uint32_t nNodes, NodeDev& nd, f4& worldLo, f4& worldHi) {
  nd.mesh = t.mesh; nd.parent = t.parent; nd.skip = t.skip; nd.depth = t.depth;
  nd.pad[1] = 0u;
  uint32_t loW, hiW;
  guWorldWords(i, t.skip, nNodes, loW, hiW);
  worldLo.w = __builtin_bit_cast(float, loW); worldHi.w = __builtin_bit_cast(float, hiW);
}
inline void guApplyHost(const GuDerived& g, NodeDev* nodes, f4* nodeWorld) {
  const uint32_t nn = uint32_t(g.topo.size());
  for (uint32_t i = 0; i < nn; i++) guApplyNode(g.topo[i], i, nn, nodes[i], nodeWorld[2u * i], nodeWorld[2u * i + 1u]);
}

}  // namespace yart_hip
