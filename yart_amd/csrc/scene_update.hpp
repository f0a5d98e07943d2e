// scene_update.hpp — the per-node arithmetic of yart_hip_scene_update: what host_scene.hpp::buildHostImage derives from the
// nodes' transforms, stated per node so that a kernel (scene_update_kernels.inc) and the host (scenes deeper than
// kSceneUpdateMaxLevels, tests/sceneupdatesim) run the same operations. buildHostImage itself is not written on top of this
// header: scene creation keeps its code, and the tests compare the two byte for byte.
//
//   suChildContribution   what a child adds to its parent's box: bounds::fromPoints of the 8 corners of the child's final box
//                         through mulPoint(child.fwd, .) — host_scene.hpp's appendChild loop
//   SuFold / suFoldJoin   the fold of a node's own mesh box and its children's contributions as a reduction over (value, index):
//                         buildHostImage joins the children in descending index order with Bounds3::join, whose
//                         ymin(m, n) = m < n ? m : n lets the LATER operand win a tie. So per bound the result is the
//                         numerical min / max, among equal candidates (+0 and -0 are equal) the lowest-index child, and the node's
//                         own box only if no child ties it. That rule is a total order on (value, index) — the own box carries the
//                         largest index — hence associative and commutative: any split of the children reproduces the host's bytes.
//                         (No candidate is a NaN: fromPoints' strict comparisons never take one, and a mesh whose vertex box is
//                         not finite is refused by the update.)
//   suWorldBox            the padded world-space box of a node in binary64 (nodeWorld), host_scene.hpp's loop
#pragma once
#include "../../include/yart_hip.h"
#include "scene_types.hpp"

namespace yart_hip {

// A scene whose graph has more levels than this is re-derived on the host (one launch per level would be that many launches).
constexpr uint32_t kSceneUpdateMaxLevels = 64;
constexpr uint32_t kSuOwnBox = 0xffffffffu;          // the index the node's own mesh box carries in the fold

static_assert(sizeof(NodeDev) == 176 && sizeof(YartNodeDesc) == 136, "the update's kernels copy these records word by word");

struct SuBox { float mn[3], mx[3]; };
struct SuFold { float mn[3], mx[3]; uint32_t imn[3], imx[3]; };

YART_HD SuBox suEmptyBox() {
  SuBox b;
  for (int c = 0; c < 3; c++) { b.mn[c] = kInf; b.mx[c] = -kInf; }
  return b;
}

YART_HD SuBox suChildContribution(const float* fwd, const float* bmin, const float* bmax) {
  SuBox b = suEmptyBox();
  for (int xi = 0; xi < 2; xi++) for (int yi = 0; yi < 2; yi++) for (int zi = 0; zi < 2; zi++) {     // transform.hpp:75-90 corner order
    const f3 p = mulPoint(fwd, mk3(xi ? bmax[0] : bmin[0], yi ? bmax[1] : bmin[1], zi ? bmax[2] : bmin[2]));
    const float v[3] = {p.x, p.y, p.z};
    for (int c = 0; c < 3; c++) {                                                                      // bounds.hpp:89-104
      if (v[c] < b.mn[c]) b.mn[c] = v[c];
      if (v[c] > b.mx[c]) b.mx[c] = v[c];
    }
  }
  for (int c = 0; c < 3; c++) { b.mn[c] -= 0.001f; b.mx[c] += 0.001f; }
  return b;
}

YART_HD SuFold suFoldOf(const SuBox& b, uint32_t index) {
  SuFold f;
  for (int c = 0; c < 3; c++) { f.mn[c] = b.mn[c]; f.mx[c] = b.mx[c]; f.imn[c] = index; f.imx[c] = index; }
  return f;
}
// the identity of suFoldJoin: loses against every candidate, the own box of a node without a mesh (+inf / -inf) included
YART_HD SuFold suFoldIdentity() { return suFoldOf(suEmptyBox(), kSuOwnBox); }

YART_HD void suFoldJoin(SuFold& a, const SuFold& b) {
  for (int c = 0; c < 3; c++) {
    if (b.mn[c] < a.mn[c] || (b.mn[c] == a.mn[c] && b.imn[c] < a.imn[c])) { a.mn[c] = b.mn[c]; a.imn[c] = b.imn[c]; }
    if (b.mx[c] > a.mx[c] || (b.mx[c] == a.mx[c] && b.imx[c] < a.imx[c])) { a.mx[c] = b.mx[c]; a.imx[c] = b.imx[c]; }
  }
}

YART_HD bool suFinite(double v) { return v - v == 0.0; }          // false for +-inf and NaN

// lo / hi: the x, y, z of the node's nodeWorld pair (the .w words depend on the topology only and are not touched)
YART_HD void suWorldBox(const NodeDev* nodes, uint32_t i, float lo[3], float hi[3]) {
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  const NodeDev& nd = nodes[i];
  bool finite = nd.depth < kMaxNodeDepth;
  for (int corner = 0; corner < 8 && finite; corner++) {
    double p[3] = {(corner & 4) ? nd.bmax[0] : nd.bmin[0], (corner & 2) ? nd.bmax[1] : nd.bmin[1],
                   (corner & 1) ? nd.bmax[2] : nd.bmin[2]};
    for (int32_t a = int32_t(i); a >= 0; a = nodes[a].parent) {
      const float* m = nodes[a].xf.fwd;
      double q[3];
      for (int r = 0; r < 3; r++) q[r] = double(m[4 * r]) * p[0] + double(m[4 * r + 1]) * p[1] + double(m[4 * r + 2]) * p[2] + double(m[4 * r + 3]);
      p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    for (int c = 0; c < 3; c++) {
      if (!suFinite(p[c])) finite = false;
      mn[c] = p[c] < mn[c] ? p[c] : mn[c];              // std::min(mn, p)
      mx[c] = mx[c] < p[c] ? p[c] : mx[c];              // std::max(mx, p)
    }
  }
  for (int c = 0; c < 3; c++) {
    const double an = __builtin_fabs(mn[c]), ax = __builtin_fabs(mx[c]);
    const double pad = 2e-3 + 1e-4 * (an < ax ? ax : an);
    lo[c] = finite ? float(mn[c] - pad) : -kInf;
    hi[c] = finite ? float(mx[c] + pad) : kInf;
  }
}

// NodeDev::pad[0] of every node from the new transforms (bit 0: the node's chain is exactly the identity, bit 1: its parent's is);
// returns HostImage::allIdentity. `parent` as at create (pre-order: a parent precedes its children).
inline bool suIdentityFlags(const YartNodeDesc* desc, uint32_t nn, uint32_t* flags) {
  static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  bool all = true;
  for (uint32_t i = 0; i < nn; i++) {
    bool ident = std::memcmp(desc[i].fwd, I, 64) == 0 && std::memcmp(desc[i].inv, I, 64) == 0;
    const bool parentIdent = i == 0 || (flags[desc[i].parent] & 1u);
    if (i > 0) ident = ident && parentIdent;
    flags[i] = (ident ? 1u : 0u) | (parentIdent ? 2u : 0u);
    if (!ident) all = false;
  }
  return all;
}

// Steps 1-3 of the update on the host, over the arrays of a scene image: transforms and flags, boxes (children folded with the
// (value, index) rule), world boxes. meshBox: one per mesh. Scenes deeper than kSceneUpdateMaxLevels take this path.
inline void suRederiveHost(NodeDev* nodes, f4* nodeWorld, uint32_t nn, const YartNodeDesc* desc, const uint32_t* flags, const SuBox* meshBox,
                           SuFold* scratch /* nn */) {
  for (uint32_t i = 0; i < nn; i++) {
    std::memcpy(nodes[i].xf.fwd, desc[i].fwd, 64); std::memcpy(nodes[i].xf.inv, desc[i].inv, 64);
    nodes[i].pad[0] = flags[i];
    scratch[i] = suFoldOf(nodes[i].mesh >= 0 ? meshBox[nodes[i].mesh] : suEmptyBox(), kSuOwnBox);
  }
  for (uint32_t i = nn; i-- > 0;) {                    // a node's children all follow it: its fold is complete when it is reached
    for (int c = 0; c < 3; c++) { nodes[i].bmin[c] = scratch[i].mn[c]; nodes[i].bmax[c] = scratch[i].mx[c]; }
    if (i > 0) suFoldJoin(scratch[nodes[i].parent], suFoldOf(suChildContribution(nodes[i].xf.fwd, nodes[i].bmin, nodes[i].bmax), i));
  }
  for (uint32_t i = 0; i < nn; i++) suWorldBox(nodes, i, &nodeWorld[2 * i].x, &nodeWorld[2 * i + 1].x);
}

}  // namespace yart_hip
