// shade_record.hpp — the result record of yart_hip_probe_shading (include/yart_hip.h) for one case record: one call, or one
// small group of calls, of the shading code of bsdf.hpp / lights.hpp (the layout of both records is spelled out in
// oracle/shaderec.hpp). Shared by k_probe_shading (probes.inc) and the `shade` mode of tests/hostsim, which compiles it for the
// host: the CPU tests run the very function the kernel runs. q, w: 32 words each. The caller has checked the case's kind and
// index against the scene.
// IMPL_E: a BSDF case goes through one matEvaluate and bsdfSampleImplE / bsdfFImplE / bsdfPdfImplE in the local frame, as
// wfShade (wavefront.hpp) calls them; otherwise through bsdfSample / bsdfF / bsdfPdf (core/bsdf.cpp:5-58's wrappers).
#pragma once
#include "lights.hpp"

namespace yart_hip {

enum : uint32_t { SHADE_LUT = 0, SHADE_TEX = 1, SHADE_MAT = 2, SHADE_BSDF = 3, SHADE_LIGHT = 4, SHADE_PICK = 5, SHADE_KINDS = 6 };
enum : uint32_t { SHADE_FORM_LDS_LUT = 1u, SHADE_FORM_LDS_RECORDS = 2u, SHADE_FORM_IMPL_E = 4u, SHADE_FORM_ALL = 7u };

YART_HD void shadePut3(float* r, int k, f3 v) { r[k] = v.x; r[k + 1] = v.y; r[k + 2] = v.z; }

YART_HD void shadeCaseRecord(const SceneDev& sc, const uint32_t* q, bool implE, uint32_t* w) {
  float f[28], r[32];
  for (int i = 0; i < 28; i++) f[i] = __builtin_bit_cast(float, q[4 + i]);
  for (int i = 0; i < 32; i++) r[i] = 0.0f;
  uint32_t word0 = 0u; bool intWord0 = false;
  const uint32_t kind = q[0], index = q[1];
  if (kind == SHADE_LUT) {
    r[0] = ggxE(sc.lut, f[0], f[1]);
    r[1] = ggxEavg(sc.lut, f[1]);
    r[2] = ggxBaseE(sc.lut, f[2], f[1], f[0]);
    r[3] = ggxBaseEavg(sc.lut, f[2], f[1]);
    r[4] = ggxGlassE(sc.lut, f[3], f[1], fabsf(f[0]));
  } else if (kind == SHADE_TEX) {
    const f2 uv = mk2(f[0], f[1]);
    const uint32_t c = sc.textures[index].channels;
    if (c == 1) r[0] = texSample1(sc, int32_t(index), uv);
    else if (c == 2) { const f2 v = texSample2(sc, int32_t(index), uv); r[0] = v.x; r[1] = v.y; }
    else if (c == 3) shadePut3(r, 0, texSample3(sc, int32_t(index), uv));
    else { const f4 v = texSample4(sc, int32_t(index), uv); r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
  } else if (kind == SHADE_MAT) {
    const MaterialDev& mt = sc.materials[index];
    const f2 uv = mk2(f[0], f[1]);
    f4 t4; t4.x = f[5]; t4.y = f[6]; t4.z = f[7]; t4.w = f[8];
    r[0] = matAlpha(sc, mt, uv);
    shadePut3(r, 1, matBase(sc, mt, uv));
    shadePut3(r, 4, bsdfNormal(sc, mt, mk3(f[2], f[3], f[4]), t4, uv));
    shadePut3(r, 7, matAttenuation(mt, f[9]));
  } else if (kind == SHADE_BSDF) {
    const MaterialDev& mt = sc.materials[index];
    const f3 wo = mk3(f[0], f[1], f[2]), wi = mk3(f[3], f[4], f[5]), n = mk3(f[6], f[7], f[8]), t = mk3(f[9], f[10], f[11]);
    const f2 uv = mk2(f[12], f[13]), u = mk2(f[14], f[15]);
    const float uc = f[16], uc2 = f[17];
    const bool reg = (q[2] & 1u) != 0u;
    f3 fv; float pdf; BsdfSample s;
    if (implE) {
      const Frame fr = shadingFrame(n, t);
      const f3 woLocal = wtl(fr, wo), wiLocal = wtl(fr, wi);
      const MatEval me = matEvaluate(sc, mt, uv);
      fv = bsdfFImplE(sc, mt, me, woLocal, wiLocal);
      pdf = bsdfPdfImplE(sc, mt, me, woLocal, wiLocal);
      s = bsdfSampleImplE(sc, mt, me, woLocal, uv, u, uc, uc2, reg);
      s.wi = ltw(fr, s.wi);
    } else {
      fv = bsdfF(sc, mt, wo, wi, n, t, uv);
      pdf = bsdfPdf(sc, mt, wo, wi, n, t, uv);
      s = bsdfSample(sc, mt, wo, n, t, uv, u, uc, uc2, reg);
    }
    word0 = uint32_t(s.scatter); intWord0 = true;
    shadePut3(r, 1, fv); r[4] = pdf;
    shadePut3(r, 5, s.f); shadePut3(r, 8, s.Le); shadePut3(r, 11, s.wi);
    r[14] = s.pdf; r[15] = s.roughness;
  } else if (kind == SHADE_LIGHT) {
    const LightDev& l = sc.lights[index];
    const LightSample s = lightSample(sc, l, mk3(f[0], f[1], f[2]), mk2(f[3], f[4]));
    shadePut3(r, 0, s.Li); shadePut3(r, 3, s.wi); shadePut3(r, 6, s.p); shadePut3(r, 9, s.n); r[12] = s.pdf;
    const f3 wi = mk3(f[5], f[6], f[7]);
    r[13] = lightPdf(sc, l, wi);
    shadePut3(r, 14, lightLe(sc, l, octahedralUV(wi)));
    r[17] = lightSamplerP(sc, index);
  } else {      // SHADE_PICK
    float pl;
    word0 = lightSamplerSample(sc, f[0], pl); intWord0 = true;
    r[1] = pl;
  }
  for (int i = 0; i < 32; i++) w[i] = __builtin_bit_cast(uint32_t, r[i]);
  if (intWord0) w[0] = word0;
}

// What a case may name in a scene of these sizes (the checks of yart_hip_probe_shading, and of hostsim before it runs a
// file): nullptr if the case is fine, else what is wrong with it. texDims: width, height per texture.
inline const char* shadeCaseProblem(const uint32_t* q, uint32_t nMaterials, uint32_t nTextures, uint32_t nLights, const uint32_t* texDims) {
  const uint32_t kind = q[0], index = q[1];
  if (kind >= SHADE_KINDS) return "unknown kind";
  for (int i = 4; i < 32; i++) if ((q[i] & 0x7f800000u) == 0x7f800000u) return "an operand is not finite";
  if (kind == SHADE_TEX) {
    if (index >= nTextures) return "texture index out of range";
    if (texDims[2 * index] < 2u || texDims[2 * index + 1] < 2u) return "a TEX case needs a texture of at least 2 x 2";
  }
  if ((kind == SHADE_MAT || kind == SHADE_BSDF) && index >= nMaterials) return "material index out of range";
  if (kind == SHADE_LIGHT && index >= nLights) return "light index out of range";
  if (kind == SHADE_PICK && nLights == 0u) return "a PICK case needs a scene with lights";
  // (lightSamplerSample takes a sampler value: with u >= 1 and no area light it would index an empty power table)
  if (kind == SHADE_PICK) {
    const float u = __builtin_bit_cast(float, q[4]);
    if (!(u >= 0.0f && u < 1.0f)) return "the u of a PICK case must lie in [0, 1)";
  }
  return nullptr;
}

}  // namespace yart_hip
