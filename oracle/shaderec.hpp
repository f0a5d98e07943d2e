// shaderec.hpp — TEST INFRASTRUCTURE: the case and result records of the `shade` mode of the three CPU checkers
// (ref_driver.cpp, oracle_main.cpp, tests/hostsim/hostsim.cpp) and of yart_hip_probe_shading (include/yart_hip.h).
// Little-endian 32-bit words, 32 per record; tests/shadesuite.py holds the same layout as numpy dtypes. One case is one call
// (or one small group of calls) of the shading code: a texture fetch, the five GGX table lookups, a material's per-hit
// quantities, a BSDF's f / pdf / sample, a light's sample / pdf / Le, or the light sampler's choice.
//
// Case, 32 words:
//   0 kind    SHADE_LUT .. SHADE_PICK        1 index   texture (TEX), material (MAT, BSDF), light (LIGHT); 0 otherwise
//   2 flags   bit 0: `regularized` of BSDF::sample (BSDF); 0 otherwise                3 pad, 0
//   4..31     f[0..27], float operands by kind, every one finite, unused ones 0:
//     LUT     f[0] c  f[1] r  f[2] f0  f[3] ior              (kat::LutInput)
//     TEX     f[0..1] uv
//     MAT     f[0..1] uv  f[2..4] n  f[5..8] tangent with handedness  f[9] d
//     BSDF    f[0..2] wo  f[3..5] wi  f[6..8] n  f[9..11] t  f[12..13] uv  f[14..15] u  f[16] uc  f[17] uc2
//     LIGHT   f[0..2] p  f[3..4] u  f[5..7] wi
//     PICK    f[0] u
//
// Result, 32 words; words a kind does not name are 0:
//     LUT     0 ggxE(c, r)  1 ggxEavg(r)  2 ggxBaseE(f0, r, c)  3 ggxBaseEavg(f0, r)  4 ggxGlassE(ior, r, |c|)
//     TEX     0..C-1 the texture's C channels (Texture::sample)
//     MAT     0 alpha(uv)  1..3 base(uv)  4..6 normal(n, t4, uv)  7..9 attenuation(d)
//     BSDF    0 scatter of the sample (integer)  1..3 f(wo, wi)  4 pdf(wo, wi)  5..7 sample.f  8..10 sample.Le  11..13 sample.wi
//             14 sample.pdf  15 sample.roughness
//     LIGHT   0..2 Li  3..5 wi  6..8 p  9..11 n  12 pdf of sample(p, u);  13 pdf(wi)  14..16 Le(octahedralUV(wi))
//             17 the light sampler's probability of this light
//     PICK    0 index of the light chosen (integer)  1 its probability
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace shaderec {

enum : uint32_t { SHADE_LUT = 0, SHADE_TEX = 1, SHADE_MAT = 2, SHADE_BSDF = 3, SHADE_LIGHT = 4, SHADE_PICK = 5, SHADE_KINDS = 6 };

struct Case { uint32_t kind, index, flags, pad; float f[28]; };
struct Rec { uint32_t w[32]; };
static_assert(sizeof(Case) == 128 && sizeof(Rec) == 128, "record layout");

inline std::vector<Case> load(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  std::vector<Case> v;
  Case c;
  while (std::fread(&c, sizeof(c), 1, f) == 1) v.push_back(c);
  const bool whole = std::feof(f) && std::ftell(f) == long(v.size() * sizeof(Case));
  std::fclose(f);
  if (!whole) throw std::runtime_error(path + ": the size is not a multiple of a case record's 128 bytes");
  return v;
}
template <class T>
inline void save(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  std::fwrite(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
}
inline void put(Rec& r, int k, float v) { __builtin_memcpy(&r.w[k], &v, 4); }

}  // namespace shaderec
