// aovsim.cpp — TEST INFRASTRUCTURE for tests/test_aovs.py, never part of libyart_hip.so.
//
// The product's device headers (yart_amd/csrc/*.hpp) compiled as host C++, as tests/hostsim does, for two questions the feature
// buffer tests ask:
//   camrays <scene.yscn> <params.txt> <in> <out>    in: n x {u32 px, u32 py, f32 film.x, film.y, lens.x, lens.y}; out: n x 6 f32,
//                                                   cameraRay of csrc/integrator.hpp for those jitter / lens values
//   hits    <scene.yscn> <params.txt> <in> <out>    in: n x {u32 px, u32 py, u32 sample}; out: n x 22 words — bounce 0 of that
//                                                   sample as integrator.hpp::samplePixel / pathRadiance run it: sampler start, film
//                                                   and lens draw, camera ray, the general closest-hit walk WITH the sampler (the
//                                                   stochastic alpha test draws from it), finalizeHit, matBase:
//                                                   ray o, d (6 f32) | hit (u32) | t | p (3) | n (3) | albedo (3) |
//                                                   node, mesh, material, triangle (i32, -1: miss) | 0
// It is written out here step by step and does not call aov.hpp, so that the comparison is between two statements.
#include <cstdio>
#include <string>
#include <vector>

#include "../../oracle/params.hpp"
#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/integrator.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static std::vector<uint32_t> readWords(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot read ") + path);
  std::vector<uint32_t> v;
  uint32_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 4, 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}
static float asFloat(uint32_t u) { return __builtin_bit_cast(float, u); }
static uint32_t asWord(float f) { return __builtin_bit_cast(uint32_t, f); }

int main(int argc, char** argv) {
  if (argc != 6) { std::fprintf(stderr, "usage: aovsim camrays|hits <scene.yscn> <params.txt> <in> <out>\n"); return 1; }
  try {
    const std::string mode = argv[1];
    auto loaded = loadSceneFile(argv[2]);
    auto p = params::load(argv[3]);
    HostImage im = buildHostImage(loaded->desc);
    const SceneDev sc = im.view();
    YartCameraDesc cd{};
    cd.width = p.width; cd.height = p.height; cd.focal_length = p.focal; cd.f_number = p.fnumber;
    cd.sensor[0] = p.sensor[0]; cd.sensor[1] = p.sensor[1];
    for (int i = 0; i < 3; i++) { cd.position[i] = p.eye[i]; cd.target[i] = p.target[i]; cd.up[i] = p.up[i]; }
    cd.exposure = p.exposure; cd.aperture_sides = p.apertureSides;
    const CameraDev cam = makeCamera(cd);
    const SamplerConfig cfg = makeSamplerConfig(p.spp, p.tile);
    const uint32_t* sobol = reinterpret_cast<const uint32_t*>(sc.lut + LutDev::sobol);
    const std::vector<uint32_t> in = readWords(argv[4]);
    std::vector<uint32_t> out;
    if (mode == "camrays") {
      for (size_t i = 0; i + 6 <= in.size(); i += 6) {
        f3 o, d;
        cameraRay(cam, in[i], in[i + 1], mk2(asFloat(in[i + 2]), asFloat(in[i + 3])), mk2(asFloat(in[i + 4]), asFloat(in[i + 5])), o, d);
        for (float v : {o.x, o.y, o.z, d.x, d.y, d.z}) out.push_back(asWord(v));
      }
    } else if (mode == "hits") {
      uint64_t stack[kRefStackDepth];
      TravStack stk;
      stk.lds = stack; stk.ldsStride = 1; stk.ldsDepth = kRefStackDepth; stk.spill = nullptr; stk.spillStride = 0;
      for (size_t i = 0; i + 3 <= in.size(); i += 3) {
        const uint32_t px = in[i], py = in[i + 1];
        Sampler smp;
        startPixelSample(smp, cfg, px, py, in[i + 2]);
        const f2 uvFilm = get2D(smp, cfg, sobol);
        const f2 uvLens = get2D(smp, cfg, sobol);
        f3 o, d;
        cameraRay(cam, px, py, uvFilm, uvLens, o, d);
        HitRec hr;
        hr.t = kInf; hr.u = hr.v = 0; hr.tri = 0; hr.node = 0; hr.backSide = 0;
        f3 dummy = mk3(1.0f);
        AlphaCtx ac; ac.sampler = &smp; ac.cfg = cfg;
        const bool didHit = traverseScene<false>(sc, o, d, 0.001f, hr, dummy, stk, ac);
        for (float v : {o.x, o.y, o.z, d.x, d.y, d.z}) out.push_back(asWord(v));
        out.push_back(didHit ? 1u : 0u);
        if (didHit) {
          const Hit h = finalizeHit(sc, hr, o, d);
          const f3 base = matBase(sc, sc.materials[h.material], h.uv);
          for (float v : {h.t, h.p.x, h.p.y, h.p.z, h.n.x, h.n.y, h.n.z, base.x, base.y, base.z}) out.push_back(asWord(v));
          out.push_back(hr.node); out.push_back(uint32_t(sc.nodes[hr.node].mesh)); out.push_back(h.material);
          out.push_back(localTri(sc, hr));
        } else {
          for (int k = 0; k < 10; k++) out.push_back(0u);
          for (int k = 0; k < 4; k++) out.push_back(0xffffffffu);
        }
        out.push_back(0u);
      }
    } else {
      std::fprintf(stderr, "aovsim: unknown mode %s\n", mode.c_str());
      return 1;
    }
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "aovsim: %s\n", e.what());
    return 2;
  }
}
