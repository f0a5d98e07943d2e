// aov.hpp — first-hit feature buffers (YART_AOV_*): what bounce 0 of a path knows about the surface it sees.
//
// The definition is the reference's Hit after testNode / testMesh (cpu/hit.hpp, cpu/ray-integrator.cpp:20-82) for the camera
// ray of a (pixel, sample): t, p and n (after BSDF::normal, world space) as finalizeHit leaves them, the base colour
// ParametricBSDF::fImpl starts from (parametric.cpp:75-78, 90-91: matBase) and the indices of the node, mesh, material and
// triangle. Every pipeline captures one AovRecord per path at the same point — after bounce 0's closest hit is final, before
// the shade stage — from the same function, so the buffers do not depend on the pipeline.
#pragma once
#include "bsdf.hpp"
#include "traverse.hpp"

namespace yart_hip {

// Per-path feature record: three 16-byte words, 48 bytes per path. A miss is {0, 0, 0, -1}, {0, 0, 0, 0}, {0, 0, 0, 0}.
//   r0 = {albedo.xyz, t (-1: miss)}   r1 = {n.xyz, hit (u32 0 / 1)}   r2 = {p.xyz, hit (u32 0 / 1)}
struct AovRecord { f4 r0, r1, r2; };
struct AovIds { int32_t node, mesh, material, tri; };   // all -1: miss

YART_HD f4 aovF4(float x, float y, float z, float w) { f4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

// the record of a closest hit `hr` (didHit: the walk's result) of the ray (o, d)
YART_HD AovRecord aovCapture(const SceneDev& sc, const HitRec& hr, bool didHit, f3 o, f3 d, AovIds& ids) {
  AovRecord r;
  if (!didHit) {
    r.r0 = aovF4(0.0f, 0.0f, 0.0f, -1.0f); r.r1 = aovF4(0.0f, 0.0f, 0.0f, 0.0f); r.r2 = r.r1;
    ids.node = ids.mesh = ids.material = ids.tri = -1;
    return r;
  }
  const Hit h = finalizeHit(sc, hr, o, d);
  const f3 base = matBase(sc, sc.materials[h.material], h.uv);
  const float one = __builtin_bit_cast(float, 1u);
  r.r0 = aovF4(base.x, base.y, base.z, h.t);
  r.r1 = aovF4(h.n.x, h.n.y, h.n.z, one);
  r.r2 = aovF4(h.p.x, h.p.y, h.p.z, one);
  ids.node = int32_t(hr.node); ids.mesh = int32_t(sc.nodes[hr.node].mesh); ids.material = int32_t(h.material);
  ids.tri = int32_t(localTri(sc, hr));
  return r;
}

}  // namespace yart_hip
