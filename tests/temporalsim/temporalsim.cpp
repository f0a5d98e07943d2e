// temporalsim.cpp — TEST INFRASTRUCTURE for tests/test_temporal.py and tools/temporal_sweep.py, never part of libyart_hip.so.
//
// The product's device headers compiled as host C++ (as tests/hostsim, tests/aovsim, tests/denoisesim and tests/momentsim
// compile them):
//   accumulate <in> <out>   csrc/temporal.hpp over a sequence of frames, driven the way csrc/postprocess.inc drives the kernel (two history
//                           images of three record planes, the previous frame's camera through makeCamera / tpCamera).
//                           in: 9 words {u32 width, height, frames, flags (1 demodulate), in_place, max_history, f32 alpha_min,
//                           normal_cos_min, plane_tolerance}, then per frame {u32 reset_before, YartCameraDesc (17 words), rgba
//                           (w*h*4 f32), variance (w*h), position (w*h*3), normal (w*h*3), depth (w*h), coverage (w*h), ids (w*h*4
//                           i32), albedo (w*h*3)}; out: per frame {rgba (w*h*4), variance (w*h), length (w*h u32)}
//   render <scene.yscn> <params.txt> <eye.x> <eye.y> <eye.z> <out>
//                           the host path tracer per sample (csrc/integrator.hpp samplePixel, as tests/momentsim `render` runs it:
//                           one wave, the GMoN estimator, csrc/moments.hpp) from the params' camera moved to `eye`, plus bounce 0
//                           of every sample replayed as tests/aovsim `hits` does and reduced as the feature buffers are defined
//                           (float32 sums over the hitting samples in ascending order, one division by float(samples); ids of
//                           sample 0). out: per pixel 20 words {rgba (4), variance, albedo (3), normal (3), position (3), depth,
//                           coverage, ids (4 i32)}
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
#include "../../yart_amd/csrc/temporal.hpp"

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
static void writeWords(const char* path, const void* p, size_t words) {
  FILE* f = std::fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
  std::fwrite(p, 4, words, f);
  std::fclose(f);
}
static float asFloat(uint32_t u) { return __builtin_bit_cast(float, u); }
static uint32_t asWord(float f) { return __builtin_bit_cast(uint32_t, f); }

struct HostHist {
  const f4 *r0, *r1, *r2;
  f4 rec0(size_t q) const { return r0[q]; }
  f4 rec1(size_t q) const { return r1[q]; }
  f4 rec2(size_t q) const { return r2[q]; }
};

static int doAccumulate(const char* inPath, const char* outPath) {
  std::vector<uint32_t> in = readWords(inPath);
  if (in.size() < 9) throw std::runtime_error("short header");
  const uint32_t w = in[0], h = in[1], frames = in[2], flags = in[3], inPlace = in[4], maxHistory = in[5];
  if (w == 0 || h == 0 || w > 4096 || h > 4096 || frames > 64 || flags > 1u || maxHistory == 0) throw std::runtime_error("bad header");
  const size_t n = size_t(w) * h, perFrame = 18 + n * 20;
  if (in.size() != 9 + perFrame * frames) throw std::runtime_error("input size does not match the header");
  TpConst k{};
  k.alphaMin = asFloat(in[6]); k.normalCosMin = asFloat(in[7]); k.planeTolerance = asFloat(in[8]);
  k.maxHistory = maxHistory; k.width = w; k.height = h;
  std::vector<f4> hist(n * 6);
  uint32_t current = 0;
  bool have = false;
  YartCameraDesc prev{};
  std::vector<uint32_t> out;
  out.reserve(n * 6 * frames);
  for (uint32_t fi = 0; fi < frames; fi++) {
    uint32_t* words = in.data() + 9 + perFrame * fi;
    if (words[0]) have = false;
    YartCameraDesc cam;
    static_assert(sizeof(YartCameraDesc) == 68, "YartCameraDesc is 17 words");
    std::memcpy(&cam, words + 1, 68);
    if (cam.width != w || cam.height != h) throw std::runtime_error("a camera's image size is not the header's");
    float* fw = reinterpret_cast<float*>(words + 18);
    float* rgba = fw; fw += n * 4;
    float* variance = fw; fw += n;
    const float* position = fw; fw += n * 3;
    const float* normal = fw; fw += n * 3;
    const float* depth = fw; fw += n;
    const float* coverage = fw; fw += n;
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(fw); fw += n * 4;
    const float* albedo = (flags & 1u) ? fw : nullptr;
    std::vector<float> sepRgba(inPlace ? 0 : n * 4), sepVar(inPlace ? 0 : n);
    float* oRgba = inPlace ? rgba : sepRgba.data();
    float* oVar = inPlace ? variance : sepVar.data();
    std::vector<uint32_t> oLen(n);
    k.haveHistory = have ? 1u : 0u;
    TpCamera pc{};
    if (have) pc = tpCamera(makeCamera(prev));
    const f4* hin = hist.data() + size_t(current) * n * 3;
    f4* hout = hist.data() + size_t(current ^ 1u) * n * 3;
    HostHist hh{hin, hin + n, hin + 2 * n};
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) {
        const size_t p = size_t(y) * w + x;
        TpIn pi;
        pi.rgba = dnF4(rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]);
        pi.variance = variance[p]; pi.depth = depth[p]; pi.coverage = coverage[p]; pi.node = ids[4 * p];
        pi.P = mk3(position[3 * p], position[3 * p + 1], position[3 * p + 2]);
        pi.n = mk3(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]);
        const TpOut o = tpAccumulatePixel(hh, k, pc, pi, albedo != nullptr,
                                           albedo ? mk3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]) : mk3(1.0f));
        hout[p] = o.rec0; hout[n + p] = o.rec1; hout[2 * n + p] = o.rec2;
        oRgba[4 * p] = o.rgba.x; oRgba[4 * p + 1] = o.rgba.y; oRgba[4 * p + 2] = o.rgba.z; oRgba[4 * p + 3] = o.rgba.w;
        oVar[p] = o.variance;
        oLen[p] = o.length;
      }
    current ^= 1u; have = true; prev = cam;
    for (size_t i = 0; i < n * 4; i++) out.push_back(asWord(oRgba[i]));
    for (size_t i = 0; i < n; i++) out.push_back(asWord(oVar[i]));
    out.insert(out.end(), oLen.begin(), oLen.end());
  }
  writeWords(outPath, out.data(), out.size());
  return 0;
}

static int doRender(const char* scenePath, const char* paramPath, const float eye[3], const char* outPath) {
  auto loaded = loadSceneFile(scenePath);
  auto p = params::load(paramPath);
  HostImage im = buildHostImage(loaded->desc);
  const SceneDev sc = im.view();
  YartCameraDesc cd{};
  cd.width = p.width; cd.height = p.height; cd.focal_length = p.focal; cd.f_number = p.fnumber;
  cd.sensor[0] = p.sensor[0]; cd.sensor[1] = p.sensor[1];
  for (int i = 0; i < 3; i++) { cd.position[i] = eye[i]; cd.target[i] = p.target[i]; cd.up[i] = p.up[i]; }
  cd.exposure = p.exposure; cd.aperture_sides = p.apertureSides;
  const CameraDev cam = makeCamera(cd);
  RenderConst rc{};
  rc.sampler = makeSamplerConfig(p.spp, p.tile);
  rc.maxDepth = p.depth;
  rc.background = mk3(p.background[0], p.background[1], p.background[2]);
  const SamplerConfig cfg = rc.sampler;
  const uint32_t W = p.width, H = p.height;
  std::vector<uint32_t> out(size_t(W) * H * 20, 0u);
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
          f3 sAlb = mk3(0), sNrm = mk3(0), sPos = mk3(0);
          float sDep = 0.0f;
          uint32_t hits = 0;
          int32_t ids[4] = {-1, -1, -1, -1};
          for (uint32_t s = 0; s < p.spp; s++) {
            const f3 L = samplePixel(px, cam, x, y, s, rays);
            const f3 v = L * cam.exposureScale;
            const int b = int(s % uint32_t(m));
            if (gmonAccepts(v)) { acc[b] += v; cnt[b]++; }
            const MomentSample ms = momentSample(L, cam.exposureScale);
            if (ms.ok) momentAdd(st, ms.w.x, ms.w.y, ms.w.z, ms.y);
            // bounce 0 again, as tests/aovsim `hits`
            Sampler smp;
            startPixelSample(smp, cfg, x, y, s);
            const f2 uvFilm = get2D(smp, cfg, px.sobol);
            const f2 uvLens = get2D(smp, cfg, px.sobol);
            f3 o, d;
            cameraRay(cam, x, y, uvFilm, uvLens, o, d);
            HitRec hr;
            hr.t = kInf; hr.u = hr.v = 0; hr.tri = 0; hr.node = 0; hr.backSide = 0;
            f3 dummy = mk3(1.0f);
            AlphaCtx ac; ac.sampler = &smp; ac.cfg = cfg;
            if (traverseScene<false>(sc, o, d, 0.001f, hr, dummy, px.stk, ac)) {
              const Hit hit = finalizeHit(sc, hr, o, d);
              const f3 base = matBase(sc, sc.materials[hit.material], hit.uv);
              sAlb = sAlb + base; sNrm = sNrm + hit.n; sPos = sPos + hit.p; sDep = sDep + hit.t;
              hits++;
              if (s == 0) { ids[0] = int32_t(hr.node); ids[1] = sc.nodes[hr.node].mesh; ids[2] = int32_t(hit.material); ids[3] = int32_t(localTri(sc, hr)); }
            }
          }
          const f3 v = gmonFinish(acc, cnt, m);
          float mean[3], variance;
          uint32_t count;
          momentFinish(st, mean, variance, count);
          const float ns = float(p.spp);
          uint32_t* o = &out[(size_t(y) * W + x) * 20];
          const float vals[16] = {0.0f * 0.0f + v.x * 1.0f, 0.0f * 0.0f + v.y * 1.0f, 0.0f * 0.0f + v.z * 1.0f, 1.0f, variance,
                                  sAlb.x / ns, sAlb.y / ns, sAlb.z / ns, sNrm.x / ns, sNrm.y / ns, sNrm.z / ns,
                                  sPos.x / ns, sPos.y / ns, sPos.z / ns, sDep / ns, float(hits) / ns};
          for (int i = 0; i < 16; i++) o[i] = asWord(vals[i]);
          for (int i = 0; i < 4; i++) o[16 + i] = uint32_t(ids[i]);
        }
      }
    });
  for (auto& t : th) t.join();
  writeWords(outPath, out.data(), out.size());
  return 0;
}

int main(int argc, char** argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "accumulate" && argc == 4) return doAccumulate(argv[2], argv[3]);
    if (mode == "render" && argc == 8) {
      const float eye[3] = {std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)};
      return doRender(argv[2], argv[3], eye, argv[7]);
    }
    std::fprintf(stderr, "usage: temporalsim accumulate <in> <out> | render <scene.yscn> <params.txt> <eye.x> <eye.y> <eye.z> <out>\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "temporalsim: %s\n", e.what());
    return 2;
  }
}
