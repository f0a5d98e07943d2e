// texture_update.hpp — the arithmetic of yart_hip_scene_update_textures: what host_scene.hpp::buildHostImage derives from the texels
// of an 8-bit material texture besides the texels themselves, stated per record so that the kernels (texture_update_kernels.inc) and
// the host (tests/texturesim) run the same operations. buildHostImage itself is not written on top of this header: scene creation
// keeps its code, and the tests compare the two byte for byte.
//
//   tuIsClone         the TexDev entries creation appends for the members of a base-colour / normal / metal-rough bundle (one per
//                     material and member) copy the texture's record and point into the bundle's 64-byte records
//   tuPlaces          the TexDev entries through which a texture's footprint records are rewritten: one per distinct quadOffset —
//                     the texture's own array if it has one, and one clone per bundle that holds it
//   tuWordHasAlpha    one RGBA word (channel c in byte c): its alpha byte is below 255 (parametric.cpp:61-63)
//   tuLeafFlags       a leaf record's matFlags word with the alpha bit of its material: MAT_TRANSPARENT and, in a leaf's first
//                     record, the long-span word (kLeafSpanShift) stay
//   tuNodeRange       the range [first, end) of the leaf order below a node of the FINAL node array (link words): the first position
//                     of its left-most leaf up to the end of its right-most one, the true span from traverse.hpp::leafSpan
//   tuLinkWord        a link word with the alpha bit set or cleared; index and span bits stay
#pragma once
#include <cstring>
#include <vector>

#include "host_scene.hpp"
#include "traverse.hpp"

namespace yart_hip {

YART_HD bool tuIsClone(const TexDev& t) { return t.quadStride != 0u; }
YART_HD bool tuWordHasAlpha(uint32_t rgba) { return (rgba >> 24) < 255u; }
YART_HD uint32_t tuLeafFlags(uint32_t matFlags, uint32_t materialFlags) {
  return (matFlags & ~uint32_t(MAT_HAS_ALPHA)) | (materialFlags & uint32_t(MAT_HAS_ALPHA));
}
YART_HD uint32_t tuLinkWord(uint32_t link, bool alphaInRange) {
  return (link & ~kLinkAlphaBit) | (alphaInRange ? kLinkAlphaBit : 0u);
}
// nodes / leaves: the mesh's (nodes[0] its root, leaves[0] the first record of its leaf order). A tree is at most kMaxStackBound
// levels deep; a walk that leaves the arrays or does not end gives false (the arrays are then not a tree of this library).
YART_HD bool tuNodeRange(const BvhNode* nodes, uint32_t nNodes, const LeafTri* leaves, uint32_t nTris, uint32_t node, uint32_t& first, uint32_t& end) {
  uint32_t at = node, steps = 0;
  while (nodes[at].span == 0u) {                              // left-most leaf
    at = nodes[at].leftFirst & kLinkIndexMask;
    if (at >= nNodes || ++steps > 4096u) return false;
  }
  first = nodes[at].leftFirst & kLinkIndexMask;
  at = node; steps = 0;
  while (nodes[at].span == 0u) {                              // right-most leaf
    at = (nodes[at].leftFirst & kLinkIndexMask) + 1u;
    if (at >= nNodes || ++steps > 4096u) return false;
  }
  const uint32_t last = nodes[at].leftFirst & kLinkIndexMask;
  if (first >= nTris || last >= nTris) return false;
  end = last + leafSpan(leaves, last, nodes[at].leftFirst >> kSpanShift);
  return end > first && end <= nTris;
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
inline std::vector<uint32_t> tuPlaces(const std::vector<TexDev>& textures, uint32_t texture) {
  std::vector<uint32_t> places;
  const TexDev& t = textures[texture];
  if (t.quadOffset != kNoTexQuads) places.push_back(texture);
  for (uint32_t i = 0; i < textures.size(); i++) {
    const TexDev& c = textures[i];
    if (!tuIsClone(c) || c.isFloat || c.offset != t.offset) continue;      // (8-bit textures never share an offset: each has texels)
    bool seen = false;
    for (uint32_t p : places) seen |= textures[p].quadOffset == c.quadOffset && tuIsClone(textures[p]);
    if (!seen) places.push_back(i);
  }
  return places;
}
// "any alpha byte below 255" over nTexels RGBA texels, word by word as the reduction kernel takes them
inline bool tuAnyAlpha(const uint8_t* rgba, size_t nTexels) {
  bool any = false;
  for (size_t i = 0; i < nTexels; i++) {
    uint32_t w;
    std::memcpy(&w, rgba + 4u * i, 4);
    any |= tuWordHasAlpha(w);
  }
  return any;
}

}  // namespace yart_hip
