// lighting_update.hpp — the arithmetic of yart_hip_scene_update_lighting: what host_scene.hpp::buildHostImage derives from the
// material and light descriptors and from the texels of an image light's map, stated per record, per table element and per row
// chain, so that the kernels (lighting_update_kernels.inc) and the host (tests/lightingsim) run the same operations.
// buildHostImage itself is not written on top of this header: scene creation keeps its code, and the tests compare the two byte
// for byte.
//
//   luMaterial        a MaterialDev from a new descriptor: every numeric field by create's arithmetic; the six texture slots (create
//                     remaps bundled slots to clone entries) and MAT_HAS_ALPHA (a property of the texels) stay, MAT_HAS_EMISSION is
//                     re-derived, MAT_THIN / MAT_TRANSPARENT cannot change (luTransparent: the check before the update)
//   luRederiveLights  the lights from new descriptors (emission, radius, transforms): rederiveLights for the area lights, the power
//                     CDF and the total power, create's expressions for the two infinite lights' power
//   luTexelSum        an image's Lavg numerator: three sequential binary32 sums over the texels in row-major order
//   luFunc            |((0 + r) + g) + b) / 3 * sin(theta_y)|: one entry of an image light's piecewise-constant function
//   luChainStep       one step of a CDF's running sum, cdf[k] = cdf[k-1] + f[k-1] * 1.0f / n: strictly sequential per row
//   luNormalised      an entry of a CDF divided by its integral (k / n where the integral is exactly 0)
//   luGuideEntry      G[j] of a guide table: create scans (idx carried across j); uj increases with j and the CDF is nondecreasing,
//                     so the scan equals a lower-bound search from index 1 per entry — each entry on its own
//   luMargPair / luRowPair   the interleaved records of EnvDev::pairOffset
#pragma once
#include <cstring>
#include <vector>

#include "host_scene.hpp"

namespace yart_hip {

// ---- image light tables ----------------------------------------------------------------------------------------------------------
YART_HD float luSinTheta(uint32_t y, uint32_t h) {                        // light.cpp:156-160
  const float v = (float(y) + 0.5f) / float(h);
  const float z = 1.0f - v * 2.0f;
  return sqrtf(1.0f - z * z);
}
YART_HD float luFunc(const float* texel, float sinTheta) {                // light.cpp:161-168; PiecewiseConstant1D takes |f|
  const float value = (((0.0f + texel[0]) + texel[1]) + texel[2]) / 3.0f;
  return fabsf(value * sinTheta);
}
YART_HD float luChainStep(float before, float f, uint32_t n) {            // sampling.hpp:127-129
  return before + f * (1.0f - 0.0f) / float(n);
}
YART_HD float luNormalised(float entry, uint32_t k, uint32_t n, float integral) {   // sampling.hpp:131-141
  return integral == 0.0f ? float(k) / float(n) : entry / integral;
}
// first idx in [1, n) with cdf[idx] >= j / K, else n (K a power of two: j / K is exact)
YART_HD uint32_t luGuideEntry(const float* cdf, uint32_t n, uint32_t j, uint32_t K) {
  const float uj = float(j) / float(K);
  uint32_t lo = 1u, hi = n > 1u ? n : 1u;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (cdf[mid] < uj) lo = mid + 1u; else hi = mid;
  }
  return lo;
}
// marginal record k of h + 1: {margCdf[k], rowInt[k], cdf_k[1], 0} (k = h: {margCdf[h], 0, 0, 0})
YART_HD void luMargPair(float* rec, uint32_t k, uint32_t h, float margCdfK, const float* rowInt, const float* cdf, uint32_t w) {
  rec[0] = margCdfK;
  rec[1] = k < h ? rowInt[k] : 0.0f;
  rec[2] = k < h ? cdf[size_t(k) * (w + 1u) + 1u] : 0.0f;
  rec[3] = 0.0f;
}
// row record k of w + 1: {cdf[k], func[k]} (func[w] = 0)
YART_HD void luRowPair(float* rec, uint32_t k, uint32_t w, float cdfK, const float* funcRow) {
  rec[0] = cdfK;
  rec[1] = k < w ? funcRow[k] : 0.0f;
}
// a texel word an update takes: finite and no larger than 2^64, so that no row sum, marginal sum or Lavg sum can overflow
inline bool luTexelWordOk(float v) { return std::fabs(v) <= 18446744073709551616.0f; }   // (false for NaN and +-inf)

struct LuSum { float r, g, b; };
inline LuSum luTexelSum(const float* px, size_t nTexels) {                 // light.cpp:169: Lavg += texel, row-major
  f3 s = mk3(0);
  for (size_t i = 0; i < nTexels; i++) s += mk3(px[3 * i], px[3 * i + 1], px[3 * i + 2]);
  return LuSum{s.x, s.y, s.z};
}
inline float luImagePower(const EnvDev& e, float radius, LuSum sum) {      // light.cpp:206-209
  f3 Lavg = mk3(sum.r, sum.g, sum.b);
  Lavg /= float(e.w * e.h);
  return e.surfaceArea * kPi * radius * radius * (((0.0f + Lavg.x) + Lavg.y) + Lavg.z) / 3.0f;
}

// ---- materials -------------------------------------------------------------------------------------------------------------------
inline bool luTransparent(const YartMaterialDesc& m) { return m.thin_transmission && m.transmission > 0.0f; }   // parametric.cpp:80-82
inline void luMaterial(MaterialDev& md, const YartMaterialDesc& m) {       // parametric.cpp:11-68, as buildHostImage states it
  md.base = mk3(m.base[0], m.base[1], m.base[2]);
  md.emission = mk3(m.emission[0], m.emission[1], m.emission[2]);
  md.cTrans = m.transmission; md.cMetallic = m.metallic; md.ior = m.ior; md.roughness = m.roughness;
  md.anisotropic = m.anisotropic; md.clearcoat = m.clearcoat; md.clearcoatRoughness = m.clearcoat_roughness;
  md.volumeColor = mk3(m.volume_color[0], m.volume_color[1], m.volume_color[2]);
  md.volumeDensity = m.volume_density;
  rotationZ3x3(-m.aniso_rotation, md.localRot);
  rotationZ3x3(m.aniso_rotation, md.invRot);
  uint32_t flags = md.flags & (MAT_THIN | MAT_HAS_ALPHA | MAT_TRANSPARENT);
  if (length2(md.emission) > 0.0f) flags |= MAT_HAS_EMISSION;
  md.flags = flags;
}
// the lobe-class bytes as uploadScene pads them
inline std::vector<uint8_t> luLobeClasses(const std::vector<MaterialDev>& materials) {
  std::vector<uint8_t> cls;
  for (const MaterialDev& m : materials) cls.push_back(lobeClass(m));
  while (cls.size() % 4u) cls.push_back(0);
  return cls;
}

// ---- lights ----------------------------------------------------------------------------------------------------------------------
// imageSum: per EnvDev of the image (LightDev::envOffset) the texel sum of its map as it is after the update
inline void luRederiveLights(HostImage& h, const YartLightDesc* lights, uint32_t n, const LuSum* imageSum) {
  for (uint32_t i = 0; i < n; i++) {
    LightDev& ld = h.lights[i];
    ld.emission = mk3(lights[i].emission[0], lights[i].emission[1], lights[i].emission[2]);
    ld.radius = lights[i].radius;
  }
  rederiveLights(h, lights, n);            // transforms, lightDesc, the area lights' area and power, the power CDF, the total power
  for (uint32_t i = 0; i < n; i++) {
    LightDev& ld = h.lights[i];
    const YartLightDesc& l = lights[i];
    if (ld.type == LIGHT_UNIFORM_INF) ld.power = 4.0f * kPi * kPi * l.radius * l.radius * length(ld.emission);   // light.cpp:98-103
    else if (ld.type == LIGHT_IMAGE_INF) ld.power = luImagePower(h.envs[ld.envOffset], l.radius, imageSum[ld.envOffset]);
  }
}

}  // namespace yart_hip
