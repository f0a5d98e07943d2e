// scene_motion.hpp — per-pixel motion of a device scene between the frame kept by yart_hip_scene_keep_previous and the current one
// (yart_hip_scene_pixel_motion_*): where each pixel's surface point was in the previous frame, and what its normal was, for rigid
// nodes and deforming meshes alike. The arithmetic of one node and of one pixel, as inline functions for the device kernels
// (scene_motion_kernels.inc) and for the host (tests/scenemotionsim).
//
// The definition is the comment above yart_hip_scene_pixel_motion_device in include/yart_hip.h; yart_amd/scene_motion.py
// scene_motion_reference is the NumPy statement. smNodeChain works in binary64 and smPixel in binary32, every operation individually
// rounded in the order written (the build has no FMA contraction); only + - * /, sqrtf (correctly rounded) and comparisons: no libm.
#pragma once
#include "denoise.hpp"
#include "scene_types.hpp"

namespace yart_hip {

// Per scene node, thirteen 16-byte words:
//   words 0 .. 2    Wc   object to world, current:   fwd_root · … · fwd_node, rows of a 3 x 4 matrix
//   words 3 .. 5    Ac   world to object, current:   inv_node · … · inv_root
//   words 6 .. 8    Wp   object to world, previous
//   words 9 .. 11   Ap   world to object, previous
//   word  12        {changed (u32 bits), mesh (i32 bits), 0, 0}   changed: a fwd / inv word on the node's chain differs between the frames
constexpr uint32_t kSmChainWords = 13;
constexpr uint32_t kSmRecordWords = 2;           // 16-byte words per pixel record: {P'.xyz, kind}, {n'.xyz, 0}
constexpr uint32_t kSmStatic = 0u, kSmMoved = 1u;

// m (3 x 4, binary64) = a · m or m · a for the top three rows of the row-major 4 x 4 binary32 matrix a, both with the implied last row
// (0, 0, 0, 1): each element a sum in ascending k of individually rounded products (k = 3 of the last column: the word times 1)
YART_HD void smMulLeft(const float* a, double m[12]) {
  double r[12];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double s = (double(a[4 * i]) * m[j] + double(a[4 * i + 1]) * m[4 + j]) + double(a[4 * i + 2]) * m[8 + j];
      if (j == 3) s = s + double(a[4 * i + 3]);
      r[4 * i + j] = s;
    }
  for (int k = 0; k < 12; k++) m[k] = r[k];
}
YART_HD void smMulRight(double m[12], const float* a) {
  double r[12];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double s = (m[4 * i] * double(a[j]) + m[4 * i + 1] * double(a[4 + j])) + m[4 * i + 2] * double(a[8 + j]);
      if (j == 3) s = s + m[4 * i + 3];
      r[4 * i + j] = s;
    }
  for (int k = 0; k < 12; k++) m[k] = r[k];
}

YART_HD bool smSameWords(const float* a, const float* b, int n) {
  bool same = true;
  for (int k = 0; k < n; k++) same = same && dnBits(a[k]) == dnBits(b[k]);
  return same;
}

// One node: its thirteen words from the previous and the current node array (same topology), by a leaf-to-root walk over `parent`
YART_HD void smNodeChain(const NodeDev* prev, const NodeDev* cur, uint32_t i, f4 out[kSmChainWords]) {
  double w[2][12], a[2][12];
  bool changed = false;
  for (int32_t k = int32_t(i); k >= 0; k = cur[k].parent) {
    const NodeDev* nd[2] = {cur + k, prev + k};
    for (int f = 0; f < 2; f++) {
      if (k == int32_t(i)) {
        for (int e = 0; e < 12; e++) { w[f][e] = double(nd[f]->xf.fwd[e]); a[f][e] = double(nd[f]->xf.inv[e]); }
      } else {
        smMulLeft(nd[f]->xf.fwd, w[f]);
        smMulRight(a[f], nd[f]->xf.inv);
      }
    }
    changed = changed || !smSameWords(cur[k].xf.fwd, prev[k].xf.fwd, 16) || !smSameWords(cur[k].xf.inv, prev[k].xf.inv, 16);
  }
  for (int f = 0; f < 2; f++)
    for (int r = 0; r < 3; r++) {
      out[6 * f + r] = dnF4(float(w[f][4 * r]), float(w[f][4 * r + 1]), float(w[f][4 * r + 2]), float(w[f][4 * r + 3]));
      out[6 * f + 3 + r] = dnF4(float(a[f][4 * r]), float(a[f][4 * r + 1]), float(a[f][4 * r + 2]), float(a[f][4 * r + 3]));
    }
  out[12] = dnF4(__builtin_bit_cast(float, changed ? 1u : 0u), __builtin_bit_cast(float, cur[i].mesh), 0.0f, 0.0f);
}

YART_HD f3 smXyz(f4 v) { return mk3(v.x, v.y, v.z); }
YART_HD bool smSame3(f4 a, f4 b) { return dnBits(a.x) == dnBits(b.x) && dnBits(a.y) == dnBits(b.y) && dnBits(a.z) == dnBits(b.z); }
// rows r0 .. r2 of a 3 x 4 matrix times the point p, and the transpose of its linear part times the vector v
YART_HD f3 smPoint(f4 r0, f4 r1, f4 r2, f3 p) { return mk3(dot(smXyz(r0), p) + r0.w, dot(smXyz(r1), p) + r1.w, dot(smXyz(r2), p) + r2.w); }
YART_HD f3 smLinT(f4 r0, f4 r1, f4 r2, f3 v) {
  return mk3(dot(mk3(r0.x, r1.x, r2.x), v), dot(mk3(r0.y, r1.y, r2.y), v), dot(mk3(r0.z, r1.z, r2.z), v));
}

// One pixel. Scene decides how a 16-byte word is fetched: sc.nodes(); sc.chain(node, i); sc.mesh(m, i), i = 0: {nodeOffset,
// leafOffset, triOffset, vertOffset}, 1: {nTris, ...} of MeshDev; sc.tri(t): triVerts; sc.cur(v) / sc.prev(v): the current and the
// previous vPos. ids: the pixel's four ids words. w0, w1: the pixel's record.
template <class Scene>
YART_HD void smPixel(const Scene& sc, f3 P, f3 n, float coverage, uint32_t node, uint32_t tri, f4& w0, f4& w1) {
  w0 = w1 = dnF4(0.0f, 0.0f, 0.0f, 0.0f);
  const bool finite = dnFinite(P.x) && dnFinite(P.y) && dnFinite(P.z) && dnFinite(n.x) && dnFinite(n.y) && dnFinite(n.z);
  if (!(coverage == 1.0f) || !finite || node >= sc.nodes()) return;
  const f4 head = sc.chain(node, 12u);
  const int32_t mesh = int32_t(dnBits(head.y));
  if (mesh < 0) return;
  const u4 m0 = sc.mesh(uint32_t(mesh), 0u), m1 = sc.mesh(uint32_t(mesh), 1u);
  if (tri >= m1.x) return;
  const u4 tv = sc.tri(size_t(m0.z) + tri);
  const size_t vo = m0.w;
  const f4 ca = sc.cur(vo + tv.x), cb = sc.cur(vo + tv.y), cc = sc.cur(vo + tv.z);
  const f4 pa = sc.prev(vo + tv.x), pb = sc.prev(vo + tv.y), pc = sc.prev(vo + tv.z);
  if (dnBits(head.x) == 0u && smSame3(ca, pa) && smSame3(cb, pb) && smSame3(cc, pc)) return;
  const f3 a = smXyz(ca), a_ = smXyz(pa);
  // the point: barycentric coordinates in the current triangle's plane, carried to the previous triangle
  const f3 po = smPoint(sc.chain(node, 3u), sc.chain(node, 4u), sc.chain(node, 5u), P);
  const f3 e1 = smXyz(cb) - a, e2 = smXyz(cc) - a, r = po - a;
  const float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), r1 = dot(r, e1), r2 = dot(r, e2);
  const float det = d11 * d22 - d12 * d12;
  const float u = (d22 * r1 - d12 * r2) / det, v = (d11 * r2 - d12 * r1) / det;
  const f3 f1 = smXyz(pb) - a_, f2 = smXyz(pc) - a_;
  const f3 p_ = (a_ + u * f1) + v * f2;
  const f3 Pq = smPoint(sc.chain(node, 6u), sc.chain(node, 7u), sc.chain(node, 8u), p_);
  // the normal: the inverse transpose of the same map
  const f3 no = smLinT(sc.chain(node, 0u), sc.chain(node, 1u), sc.chain(node, 2u), n);
  const float g11 = dot(f1, f1), g12 = dot(f1, f2), g22 = dot(f2, f2);
  const float gdet = g11 * g22 - g12 * g12;
  const f3 D1 = (g22 * f1 - g12 * f2) / gdet, D2 = (g11 * f2 - g12 * f1) / gdet;
  const f3 N = cross(e1, e2), N_ = cross(f1, f2);
  const float gamma = dot(no, N) / sqrtf(dot(N, N) * dot(N_, N_));
  const f3 no_ = (dot(no, e1) * D1 + dot(no, e2) * D2) + gamma * N_;
  const f3 nq = smLinT(sc.chain(node, 9u), sc.chain(node, 10u), sc.chain(node, 11u), no_);
  w0 = dnF4(Pq.x, Pq.y, Pq.z, __builtin_bit_cast(float, kSmMoved));
  w1 = dnF4(nq.x, nq.y, nq.z, 0.0f);
}

}  // namespace yart_hip
