// temporalsim_moments.cpp — TEST INFRASTRUCTURE for tests/test_temporal_moments.py, never part of libyart_hip.so.
//
// The moments form of the temporal accumulation (csrc/temporal.hpp: tpAccumulatePixel<true>, then tpSpatialVariance) compiled as
// host C++ over a sequence of frames, driven the way csrc/postprocess.inc drives the two kernels: two history images of four record planes,
// the previous frame's camera through makeCamera / tpCamera, pass 2 over the whole image after pass 1 has written all of it.
//
//   temporalsim_moments <in> <out>
//     in: 10 words {u32 width, height, frames, flags (1 demodulate), in_place, max_history, min_moment_history, f32 alpha_min,
//     normal_cos_min, plane_tolerance}, then per frame what tests/temporalsim `accumulate` takes: {u32 reset_before, YartCameraDesc
//     (17 words), rgba (w*h*4 f32), variance (w*h), position (w*h*3), normal (w*h*3), depth (w*h), coverage (w*h), ids (w*h*4 i32),
//     albedo (w*h*3)}; out: per frame {rgba (w*h*4), variance (w*h), length (w*h u32)}
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
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
static float asFloat(uint32_t u) { return __builtin_bit_cast(float, u); }
static uint32_t asWord(float f) { return __builtin_bit_cast(uint32_t, f); }

struct HostHist {
  const f4 *r0, *r1, *r2, *r3;
  f4 rec0(size_t q) const { return r0[q]; }
  f4 rec1(size_t q) const { return r1[q]; }
  f4 rec2(size_t q) const { return r2[q]; }
  f4 rec3(size_t q) const { return r3[q]; }
};

static int run(const char* inPath, const char* outPath) {
  std::vector<uint32_t> in = readWords(inPath);
  constexpr size_t kHead = 10;
  if (in.size() < kHead) throw std::runtime_error("short header");
  const uint32_t w = in[0], h = in[1], frames = in[2], flags = in[3], inPlace = in[4], maxHistory = in[5], minMoment = in[6];
  if (w == 0 || h == 0 || w > 4096 || h > 4096 || frames > 64 || flags > 1u || maxHistory == 0 || minMoment < 2)
    throw std::runtime_error("bad header");
  const size_t n = size_t(w) * h, perFrame = 18 + n * 20;
  if (in.size() != kHead + perFrame * frames) throw std::runtime_error("input size does not match the header");
  TpConst k{};
  k.alphaMin = asFloat(in[7]); k.normalCosMin = asFloat(in[8]); k.planeTolerance = asFloat(in[9]);
  k.maxHistory = maxHistory; k.minMomentHistory = minMoment; k.width = w; k.height = h;
  std::vector<f4> hist(n * 8);
  uint32_t current = 0;
  bool have = false;
  YartCameraDesc prev{};
  std::vector<uint32_t> out;
  out.reserve(n * 6 * frames);
  for (uint32_t fi = 0; fi < frames; fi++) {
    uint32_t* words = in.data() + kHead + perFrame * fi;
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
    const f4* hin = hist.data() + size_t(current) * n * 4;
    f4* hout = hist.data() + size_t(current ^ 1u) * n * 4;
    const HostHist hh{hin, hin + n, hin + 2 * n, hin + 3 * n};
    auto albedoOf = [&](size_t p) { return albedo ? mk3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]) : mk3(1.0f); };
    // pass 1
    for (size_t p = 0; p < n; p++) {
      TpIn pi;
      pi.rgba = dnF4(rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]);
      pi.variance = variance[p]; pi.depth = depth[p]; pi.coverage = coverage[p]; pi.node = ids[4 * p];
      pi.P = mk3(position[3 * p], position[3 * p + 1], position[3 * p + 2]);
      pi.n = mk3(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]);
      const TpOut o = tpAccumulatePixel<true>(hh, k, pc, pi, albedo != nullptr, albedoOf(p));
      hout[p] = o.rec0; hout[n + p] = o.rec1; hout[2 * n + p] = o.rec2; hout[3 * n + p] = o.rec3;
      oRgba[4 * p] = o.rgba.x; oRgba[4 * p + 1] = o.rgba.y; oRgba[4 * p + 2] = o.rgba.z; oRgba[4 * p + 3] = o.rgba.w;
      oVar[p] = o.variance;
      oLen[p] = o.length;
    }
    // pass 2, on the image pass 1 wrote: reads rec1 / rec2 / rec3, writes the pixel's own rec0.w and variance
    const HostHist nh{hout, hout + n, hout + 2 * n, hout + 3 * n};
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) {
        const size_t p = size_t(y) * w + x;
        float vAcc;
        if (!tpSpatialVariance(nh, k, x, y, depth[p], vAcc)) continue;
        hout[p].w = vAcc;
        const f3 d = tpDivisor(albedo != nullptr, albedoOf(p));
        const float ld = dnLuma(d.x, d.y, d.z);
        oVar[p] = vAcc * (ld * ld);
      }
    current ^= 1u; have = true; prev = cam;
    for (size_t i = 0; i < n * 4; i++) out.push_back(asWord(oRgba[i]));
    for (size_t i = 0; i < n; i++) out.push_back(asWord(oVar[i]));
    out.insert(out.end(), oLen.begin(), oLen.end());
  }
  FILE* f = std::fopen(outPath, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + outPath);
  std::fwrite(out.data(), 4, out.size(), f);
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 3) return run(argv[1], argv[2]);
    std::fprintf(stderr, "usage: temporalsim_moments <in> <out>\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "temporalsim_moments: %s\n", e.what());
    return 2;
  }
}
