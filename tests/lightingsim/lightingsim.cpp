// lightingsim — csrc/lighting_update.hpp on the host against host_scene.hpp::buildHostImage (tests/test_lighting_update_host.py).
//
//   lightingsim OLD.yscn NEW.yscn
//
// OLD and NEW are one scene with two sets of material values, light emission / radius / transforms and texels of the image lights'
// maps. The program builds buildHostImage(NEW) — what a freshly created scene holds — and re-derives, from buildHostImage(OLD) and
// NEW's descriptors and texels, what yart_hip_scene_update_lighting re-derives, with the functions of lighting_update.hpp driven the
// way the kernels of lighting_update_kernels.inc drive them: one call per table element, the row chains in 64-column tiles, rows and
// entries visited in a scrambled order. Everything is compared byte for byte. One line per image light: `env E texture T changed C
// w W h H blackRows B margIntegral M`, one line `classes changed N`, one line per comparison. Exit status 0: everything equal;
// 3: scene creation refuses OLD or NEW (the message says why).
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/lighting_update.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static int failures = 0;
static void same(const std::string& what, const void* a, const void* b, size_t n) {
  const bool ok = std::memcmp(a, b, n) == 0;
  std::printf("%s %s (%zu bytes)\n", ok ? "EQUAL" : "DIFFERENT", what.c_str(), n);
  if (!ok) failures++;
}
static std::vector<size_t> scrambled(size_t n, uint32_t seed) {
  std::vector<size_t> v(n);
  std::iota(v.begin(), v.end(), size_t(0));
  std::mt19937 rng(seed);
  for (size_t i = n; i > 1; i--) std::swap(v[i - 1], v[rng() % i]);
  return v;
}

// the tables of one image light in place, from the texels at `tex`: the kernels' passes in the kernels' order
static void rebuildEnv(HostImage& im, uint32_t env, const float* tex) {
  EnvDev& e = im.envs[env];
  const uint32_t w = e.w, h = e.h;
  float* D = im.envData.data();
  uint32_t* G = im.envGuide.data();
  // everything the update rewrites starts from garbage: whatever is equal afterwards was written
  for (size_t i = e.funcOffset; i < size_t(e.pairOffset) + size_t(h + 1u) * 4u + size_t(h) * (w + 1u) * 2u; i++) {
    if (i >= size_t(e.margCdfOffset) + h + 1u && i < e.pairOffset) continue;      // (create's alignment pad: not the update's)
    D[i] = -7.0f;
  }
  for (size_t i = 0; i < size_t(e.guideKh) + 1u + size_t(h) * (size_t(e.guideKw) + 1u); i++) G[e.guideOffset + i] = 0xdeadbeefu;
  e.margIntegral = -7.0f;
  for (size_t i : scrambled(size_t(w) * h, 1))                                      // k_lu_func
    D[e.funcOffset + i] = luFunc(tex + i * 3u, luSinTheta(uint32_t(i / w), h));
  for (size_t y : scrambled(h, 2)) {                                                // k_lu_rows: 64-column tiles
    float acc = 0.0f, tile[64];
    float* cdf = D + e.cdfOffset + y * (w + 1u);
    cdf[0] = 0.0f;
    for (uint32_t c0 = 0; c0 < w; c0 += 64u) {
      const uint32_t cols = w - c0 < 64u ? w - c0 : 64u;
      for (uint32_t c = 0; c < cols; c++) tile[c] = D[e.funcOffset + y * w + c0 + c];
      for (uint32_t c = 0; c < cols; c++) { acc = luChainStep(acc, tile[c], w); tile[c] = acc; }
      for (uint32_t c = 0; c < cols; c++) cdf[1u + c0 + c] = tile[c];
    }
    D[e.rowIntOffset + y] = fabsf(acc);
  }
  float* rowPairs = D + e.pairOffset + size_t(h + 1u) * 4u;
  for (size_t i : scrambled(size_t(w + 1u) * h, 3)) {                               // k_lu_norm
    const uint32_t y = uint32_t(i / (w + 1u)), k = uint32_t(i % (w + 1u));
    float v = 0.0f;
    if (k) { v = luNormalised(D[e.cdfOffset + i], k, w, D[e.rowIntOffset + y]); D[e.cdfOffset + i] = v; }
    luRowPair(rowPairs + i * 2u, k, w, v, D + e.funcOffset + size_t(y) * w);
  }
  {                                                                                 // k_lu_marginal
    float acc = 0.0f;
    float* marg = D + e.margCdfOffset;
    marg[0] = 0.0f;
    for (uint32_t k = 1; k <= h; k++) { acc = luChainStep(acc, fabsf(D[e.rowIntOffset + k - 1u]), h); marg[k] = acc; }
    e.margIntegral = acc;
    for (size_t k : scrambled(size_t(h) + 1u, 4)) {
      const float v = k ? luNormalised(marg[k], uint32_t(k), h, acc) : 0.0f;
      marg[k] = v;
      luMargPair(D + e.pairOffset + k * 4u, uint32_t(k), h, v, D + e.rowIntOffset, D + e.cdfOffset, w);
    }
  }
  const size_t first = size_t(e.guideKh) + 1u;                                      // k_lu_guide
  for (size_t i : scrambled(first + size_t(h) * (size_t(e.guideKw) + 1u), 5)) {
    if (i < first) { G[e.guideOffset + i] = luGuideEntry(D + e.margCdfOffset, h, uint32_t(i), e.guideKh); continue; }
    const uint32_t y = uint32_t((i - first) / (e.guideKw + 1u)), j = uint32_t((i - first) % (e.guideKw + 1u));
    G[e.guideOffset + i] = luGuideEntry(D + e.cdfOffset + size_t(y) * (w + 1u), w, j, e.guideKw);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: lightingsim OLD.yscn NEW.yscn\n"); return 2; }
  auto a = loadSceneFile(argv[1]);
  auto b = loadSceneFile(argv[2]);
  HostImage old, want;
  try {
    old = buildHostImage(a->desc); want = buildHostImage(b->desc);
  } catch (const std::invalid_argument& e) {
    std::printf("REFUSED by scene creation: %s\n", e.what());
    return 3;
  }
  const YartSceneDesc& d = b->desc;
  if (a->desc.n_materials != d.n_materials || a->desc.n_lights != d.n_lights || a->desc.n_textures != d.n_textures || a->desc.n_meshes != d.n_meshes) {
    std::fprintf(stderr, "the scenes differ in their counts\n");
    return 2;
  }
  HostImage im = old;
  // ---- materials
  for (uint32_t i = 0; i < d.n_materials; i++) {
    const YartMaterialDesc& m = d.materials[i]; const YartMaterialDesc& o = a->desc.materials[i];
    if (m.tex_base != o.tex_base || m.tex_mr != o.tex_mr || m.tex_normal != o.tex_normal || m.tex_transmission != o.tex_transmission ||
        m.tex_clearcoat != o.tex_clearcoat || m.tex_emission != o.tex_emission || m.thin_transmission != o.thin_transmission ||
        luTransparent(m) != ((im.materials[i].flags & MAT_TRANSPARENT) != 0u)) {
      std::fprintf(stderr, "material %u: a change the update refuses\n", i);
      return 2;
    }
    luMaterial(im.materials[i], m);
  }
  same("materials", im.materials.data(), want.materials.data(), want.materials.size() * sizeof(MaterialDev));
  {
    const std::vector<uint8_t> c0 = luLobeClasses(old.materials), c1 = luLobeClasses(im.materials), cw = luLobeClasses(want.materials);
    uint32_t changed = 0;
    for (size_t i = 0; i < c0.size(); i++) changed += c0[i] != c1[i];
    std::printf("classes changed %u\n", changed);
    same("lobe classes", c1.data(), cw.data(), cw.size());
  }
  // ---- the image lights' maps
  std::vector<LuSum> sums(im.envs.size(), LuSum{0.0f, 0.0f, 0.0f});
  for (uint32_t i = 0; i < d.n_lights; i++) {
    if (d.lights[i].type != LIGHT_IMAGE_INF) continue;
    const uint32_t t = uint32_t(d.lights[i].texture), env = im.lights[i].envOffset;
    const TexDev& td = im.textures[t];
    const float* px = static_cast<const float*>(d.textures[t].data);
    const size_t n = size_t(td.width) * td.height * 3u;
    if (d.textures[t].width != td.width || d.textures[t].height != td.height) { std::fprintf(stderr, "texture %u: resized\n", t); return 2; }
    for (size_t k = 0; k < n; k++) if (!luTexelWordOk(px[k])) { std::fprintf(stderr, "texture %u: a texel the update refuses\n", t); return 2; }
    const bool changed = std::memcmp(px, a->desc.textures[t].data, n * 4u) != 0;
    std::memcpy(im.texF32.data() + td.offset, px, n * 4u);
    rebuildEnv(im, env, im.texF32.data() + td.offset);
    sums[env] = luTexelSum(px, n / 3u);
    uint32_t black = 0;
    for (uint32_t y = 0; y < td.height; y++) black += im.envData[im.envs[env].rowIntOffset + y] == 0.0f;
    std::printf("env %u texture %u changed %d w %u h %u blackRows %u margIntegral %g\n", env, t, int(changed), td.width, td.height, black,
                double(im.envs[env].margIntegral));
  }
  same("texF32", im.texF32.data(), want.texF32.data(), want.texF32.size() * 4u);
  same("envs", im.envs.data(), want.envs.data(), want.envs.size() * sizeof(EnvDev));
  same("envData", im.envData.data(), want.envData.data(), want.envData.size() * 4u);
  same("envGuide", im.envGuide.data(), want.envGuide.data(), want.envGuide.size() * 4u);
  // ---- lights
  luRederiveLights(im, d.lights, im.nLights, sums.data());
  same("lights", im.lights.data(), want.lights.data(), want.lights.size() * sizeof(LightDev));
  same("areaPowerCdf", im.areaPowerCdf.data(), want.areaPowerCdf.data(), want.areaPowerCdf.size() * 4u);
  same("totalPower", &im.totalPower, &want.totalPower, 4);
  {
    uint32_t equalCdf = 0;
    for (size_t k = 1; k < im.nArea; k++) equalCdf += im.areaPowerCdf[k] == im.areaPowerCdf[k - 1];
    std::printf("power cdf: %u entries, %u equal to their predecessor, total %g\n", im.nArea, equalCdf, double(im.totalPower));
  }
  // what the update leaves alone is the new scene's too (the two descriptions differ in nothing else)
  same("textures", im.textures.data(), want.textures.data(), want.textures.size() * sizeof(TexDev));
  same("leaf records", im.leafTris.data(), want.leafTris.data(), want.leafTris.size() * sizeof(LeafTri));
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
