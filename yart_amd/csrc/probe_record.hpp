// probe_record.hpp — the result record of yart_hip_probe_rays (include/yart_hip.h) for one ray record: one traverseScene in
// the instantiation MODE, as closest-hit or occlusion walk by the ray's kind word, then finalizeHit. Shared by k_probe_rays
// (probes.inc) and the `hits` mode of tests/hostsim, which compiles it for the host: the CPU tests run the very function
// the kernel runs. q: 12 words, w: 20 words (the layout is spelled out in oracle/rayrec.hpp).
#pragma once
#include "traverse.hpp"

namespace yart_hip {

template <bool NEE, int MODE>
YART_HD void probeRayRecordOf(const SceneDev& sc, const SamplerConfig& cfg, const TravStack& stk, const uint32_t* q, uint32_t* w) {
  float f[7];
  for (int i = 0; i < 7; i++) f[i] = __builtin_bit_cast(float, q[i]);
  const f3 o = mk3(f[0], f[1], f[2]), d = mk3(f[3], f[4], f[5]);
  Sampler smp;
  startPixelSample(smp, cfg, q[8], q[9], q[10]);
  HitRec hr; hr.t = f[6]; hr.u = hr.v = 0; hr.tri = 0; hr.node = 0; hr.backSide = 0;
  f3 att = mk3(1.0f);
  AlphaCtx ac; ac.sampler = &smp; ac.cfg = cfg;
  const bool hit = traverseScene<NEE, MODE>(sc, o, d, 0.001f, hr, att, stk, ac);
  for (int i = 0; i < 20; i++) w[i] = 0u;
  if ((MODE & TRAV_FAST) && ac.deferred) { w[18] = 1u; return; }
  float r[14] = {0};
  r[9] = r[10] = r[11] = 1.0f;
  w[0] = hit ? 1u : 0u; w[2] = 0xffffffffu;
  // (a fast occlusion walk stops tracking the hit once the ray is occluded: the flag, the attenuation of an unoccluded ray and
  // the draw are its results)
  if (hit && !(NEE && (MODE & TRAV_FAST))) {
    w[1] = localTri(sc, hr); w[2] = uint32_t(sc.shadeTris[hr.tri].light); w[3] = hr.backSide & 1u; w[4] = __builtin_bit_cast(uint32_t, hr.t);
    if (!NEE) {
      const Hit h = finalizeHit(sc, hr, o, d);
      r[0] = h.p.x; r[1] = h.p.y; r[2] = h.p.z; r[3] = h.n.x; r[4] = h.n.y; r[5] = h.n.z; r[6] = h.tg.x; r[7] = h.tg.y; r[8] = h.tg.z;
    }
  }
  if (!(NEE && (MODE & TRAV_FAST) && hit)) { r[9] = att.x; r[10] = att.y; r[11] = att.z; }
  r[12] = get1D(smp, cfg);
  for (int i = 0; i < 13; i++) w[5 + i] = __builtin_bit_cast(uint32_t, r[i]);
}
template <int MODE>
YART_HD void probeRayRecord(const SceneDev& sc, const SamplerConfig& cfg, const TravStack& stk, const uint32_t* q, uint32_t* w) {
  if (q[7]) probeRayRecordOf<true, MODE>(sc, cfg, stk, q, w);
  else probeRayRecordOf<false, MODE>(sc, cfg, stk, q, w);
}

}  // namespace yart_hip
