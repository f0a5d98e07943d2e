// momentsim.cpp — TEST INFRASTRUCTURE for tests/test_moments.py, tests/test_denoise_var.py and tools/denoise_var_sweep.py, never
// part of libyart_hip.so.
//
// The product's device headers compiled as host C++ (as tests/hostsim, tests/aovsim and tests/denoisesim compile them):
//   reduce <in> <out>      csrc/moments.hpp over caller-supplied per-sample records.
//                          in: 3 words {u32 n_pixels, u32 spp, f32 exposure_scale}, then n_pixels * spp records of 4 f32
//                          (pixel-major, samples ascending); out: per pixel 5 words {mean r, g, b, variance (f32), count (u32)}
//   render <scene.yscn> <params.txt> <frame out> <moments out>
//                          the host path tracer per sample (csrc/integrator.hpp samplePixel, as tests/hostsim `render` runs it: one
//                          wave, the GMoN estimator) with every sample also reduced by csrc/moments.hpp.
//                          frame out: w * h * 4 f32 — the very frame hostsim `render` writes; moments out: per pixel 5 words as above
//   denoisevar <in> <out>  csrc/denoise.hpp's variance-guided filter, driven the way csrc/postprocess.inc drives the kernels
//                          (tests/denoisesim/dn_host.hpp, which states the file format).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../oracle/params.hpp"
#include "../../yart_amd/csrc/estimator.hpp"
#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/integrator.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"
#include "../../yart_amd/csrc/moments.hpp"
#include "../denoisesim/dn_host.hpp"

using namespace yart_hip;

static void putMoments(const MomentState& st, uint32_t* o) {
  float mean[3], variance;
  uint32_t count;
  momentFinish(st, mean, variance, count);
  o[0] = asWord(mean[0]); o[1] = asWord(mean[1]); o[2] = asWord(mean[2]); o[3] = asWord(variance); o[4] = count;
}

static int doReduce(const char* inPath, const char* outPath) {
  const std::vector<float> in = readFloats(inPath);
  if (in.size() < 3) throw std::runtime_error("short header");
  const uint32_t n = asWord(in[0]), spp = asWord(in[1]);
  const float scale = in[2];
  if (in.size() != 3 + size_t(n) * spp * 4) throw std::runtime_error("input size does not match the header");
  std::vector<uint32_t> out(size_t(n) * 5);
  for (uint32_t p = 0; p < n; p++) {
    MomentState st{};
    for (uint32_t s = 0; s < spp; s++) {
      const float* q = &in[3 + (size_t(p) * spp + s) * 4];
      const MomentSample m = momentSample(mk3(q[0], q[1], q[2]), scale);
      if (m.ok) momentAdd(st, m.w.x, m.w.y, m.w.z, m.y);
    }
    putMoments(st, &out[size_t(p) * 5]);
  }
  writeWords(outPath, out.data(), out.size());
  return 0;
}

static int doRender(const char* scenePath, const char* paramPath, const char* framePath, const char* momentPath) {
  auto loaded = loadSceneFile(scenePath);
  auto p = params::load(paramPath);
  HostImage im = buildHostImage(loaded->desc);
  const SceneDev sc = im.view();
  YartCameraDesc cd{};
  cd.width = p.width; cd.height = p.height; cd.focal_length = p.focal; cd.f_number = p.fnumber;
  cd.sensor[0] = p.sensor[0]; cd.sensor[1] = p.sensor[1];
  for (int i = 0; i < 3; i++) { cd.position[i] = p.eye[i]; cd.target[i] = p.target[i]; cd.up[i] = p.up[i]; }
  cd.exposure = p.exposure; cd.aperture_sides = p.apertureSides;
  const CameraDev cam = makeCamera(cd);
  RenderConst rc{};
  rc.sampler = makeSamplerConfig(p.spp, p.tile);
  rc.maxDepth = p.depth;
  rc.background = mk3(p.background[0], p.background[1], p.background[2]);
  const uint32_t W = p.width, H = p.height;
  std::vector<float> img(size_t(W) * H * 4, 0.0f);
  std::vector<uint32_t> mom(size_t(W) * H * 5, 0u);
  const unsigned nt = std::max(1u, p.threads ? p.threads : std::thread::hardware_concurrency());
  const uint32_t bound = std::max(kRefStackDepth, im.stackBound);
  std::atomic<uint32_t> nextRow{0};
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++)
    th.emplace_back([&] {
      std::unique_ptr<uint64_t[]> stack(new uint64_t[bound]);
      PathCtx px;
      px.sc = &sc;
      px.sobol = reinterpret_cast<const uint32_t*>(sc.lut + LutDev::sobol);
      px.stk.lds = stack.get(); px.stk.ldsStride = 1; px.stk.ldsDepth = bound; px.stk.spill = nullptr; px.stk.spillStride = 0;
      px.rc = rc;
      uint32_t rays = 0;
      const int m = gmonBuckets(int32_t(p.spp));
      for (;;) {
        const uint32_t y = nextRow++;
        if (y >= H) break;
        for (uint32_t x = 0; x < W; x++) {
          f3 acc[kGmonMax]; uint32_t cnt[kGmonMax];
          for (int b = 0; b < kGmonMax; b++) { acc[b] = mk3(0); cnt[b] = 0; }
          MomentState st{};
          for (uint32_t s = 0; s < p.spp; s++) {
            const f3 L = samplePixel(px, cam, x, y, s, rays);
            const f3 v = L * cam.exposureScale;
            const int b = int(s % uint32_t(m));
            if (gmonAccepts(v)) { acc[b] += v; cnt[b]++; }
            const MomentSample ms = momentSample(L, cam.exposureScale);
            if (ms.ok) momentAdd(st, ms.w.x, ms.w.y, ms.w.z, ms.y);
          }
          const f3 v = gmonFinish(acc, cnt, m);
          float* o = &img[(size_t(y) * W + x) * 4];
          o[0] = 0.0f * 0.0f + v.x * 1.0f; o[1] = 0.0f * 0.0f + v.y * 1.0f; o[2] = 0.0f * 0.0f + v.z * 1.0f;   // (one wave, as hostsim blends it)
          o[3] = 1.0f;
          putMoments(st, &mom[(size_t(y) * W + x) * 5]);
        }
      }
    });
  for (auto& t : th) t.join();
  writeWords(framePath, img.data(), img.size());
  writeWords(momentPath, mom.data(), mom.size());
  return 0;
}

int main(int argc, char** argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "reduce" && argc == 4) return doReduce(argv[2], argv[3]);
    if (mode == "render" && argc == 6) return doRender(argv[2], argv[3], argv[4], argv[5]);
    if (mode == "denoisevar" && argc == 4) { dnHostRunFile<true>(argv[2], argv[3]); return 0; }
    std::fprintf(stderr, "usage: momentsim reduce <in> <out> | render <scene.yscn> <params.txt> <frame> <moments> | denoisevar <in> <out>\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "momentsim: %s\n", e.what());
    return 2;
  }
}
