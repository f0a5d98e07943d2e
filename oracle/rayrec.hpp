// rayrec.hpp — TEST INFRASTRUCTURE: the ray and result records of the `hits` mode of the three CPU checkers
// (ref_driver.cpp, oracle_main.cpp, tests/hostsim/hostsim.cpp) and of yart_hip_probe_rays (include/yart_hip.h).
// Little-endian 32-bit words; tests/raysuite.py holds the same layout as numpy dtypes.
//
// Ray, 12 words: o[3], d[3], tMax (f32; +inf for a closest-hit ray), kind (0 closest-hit, 1 occlusion: Ray::nee set,
// as MISIntegrator::unoccluded does), x, y, s (the sampler is started with startPixelSample((x, y), s) before the walk),
// one pad word. Both kinds enter testNode(root) with tMin = 0.001 and hit.t = tMax.
//
// Result, 20 words:
//   0 hit      testNode's return value (for an occlusion ray: occluded)
//   1 tri      Hit::idx, mesh-local (0 without a hit)       2 light   Hit::lightIdx (-1 without a hit)
//   3 backSide                                              4 t       Hit::t after the walk (0 without a hit)
//   5..13      p, n, tg in world space — closest-hit rays with a hit only, 0 otherwise (an occlusion walk leaves
//              Hit::n overwritten by the transparent candidates it passed, ray-integrator.cpp:213-217: no quantity
//              the renderer reads)
//   14..16     Hit::attenuation after the walk (1, 1, 1 for a closest-hit ray)
//   17 draw    one get1D() after the walk: pins the number of sampler dimensions the walk consumed
//   18 deferred  always 0 from the CPU checkers; the device's TRAV_FAST walks set it (and zero the rest) for a ray they
//              hand over to the general walk
//   19         0
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace rayrec {

struct Ray { float o[3], d[3], tMax; uint32_t kind, x, y, s, pad; };
struct Rec {
  uint32_t hit, tri; int32_t light; uint32_t backSide;
  float t, p[3], n[3], tg[3], att[3], draw;
  uint32_t deferred, pad;
};
static_assert(sizeof(Ray) == 48 && sizeof(Rec) == 80, "record layout");

inline std::vector<Ray> load(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  std::vector<Ray> v;
  Ray r;
  while (std::fread(&r, sizeof(r), 1, f) == 1) v.push_back(r);
  std::fclose(f);
  return v;
}
template <class T>
inline void save(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  std::fwrite(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
}
inline Rec miss() {
  Rec r{};
  r.light = -1;
  r.att[0] = r.att[1] = r.att[2] = 1.0f;
  return r;
}

}  // namespace rayrec
