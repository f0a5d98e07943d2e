// temporalclipsim.cpp — TEST INFRASTRUCTURE for tests/test_temporal_clip.py, never part of libyart_hip.so.
//
// Both forms of the temporal accumulation with the clip of the history to the frame's neighbourhood (csrc/temporal.hpp:
// tpAccumulatePixel<MOMENTS> with a Frame, then tpSpatialVariance in the moments form) compiled as host C++ over a sequence of
// frames, driven the way csrc/postprocess.inc drives the kernels: two history images of three (four) record planes, the previous
// frame's camera through makeCamera / tpCamera, a per-node or a per-pixel motion through its accessor, and — as the driver stages
// the frame of a call whose output aliases it — a copy of the frame for the neighbours' reads when the outputs are written in place.
//
//   temporalclipsim <in> <out>
//     in: 13 words {u32 width, height, frames, flags (1 demodulate), in_place, max_history, min_moment_history (0: the plain form),
//     n_nodes, clip_radius (0: no clip), f32 alpha_min, normal_cos_min, plane_tolerance, clip_gamma}, then per frame {u32
//     reset_before, motion (0 none, 1 per node, 2 per pixel), YartCameraDesc (17 words), rgba (w*h*4 f32), variance (w*h), position
//     (w*h*3), normal (w*h*3), depth (w*h), coverage (w*h), ids (w*h*4 i32), albedo (w*h*3), and the motion's records (n_nodes*24
//     words per node, or w*h*8 per pixel)}; out: per frame {rgba (w*h*4), variance (w*h), length (w*h u32)}
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
struct HostMotion {
  static constexpr bool kNone = false;
  const float* rec;
  uint32_t n;
  uint32_t nodes() const { return n; }
  f4 word(uint32_t node, uint32_t i) const {
    const float* p = rec + (size_t(node) * kTpMotionWords + i) * 4;
    return dnF4(p[0], p[1], p[2], p[3]);
  }
};
struct HostPixelMotion {
  static constexpr bool kNone = false, kPixel = true;
  const float* rec;                               // the pixel's 8 floats
  f4 word(uint32_t i) const { return dnF4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]); }
};
// the neighbourhood of pixel (x, y) in the frame: every texel is formed on the fetch
struct HostFrame {
  static constexpr bool kNone = false;
  const float *rgba, *albedo;                     // albedo: null unless the call demodulates
  uint32_t w, h, x, y, r;
  float g;
  uint32_t radius() const { return r; }
  float gamma() const { return g; }
  f4 texel(int dx, int dy) const {
    const int qx = int(x) + dx, qy = int(y) + dy;
    if (qx < 0 || qx >= int(w) || qy < 0 || qy >= int(h)) return dnF4(0.0f, 0.0f, 0.0f, 0.0f);
    const size_t q = size_t(qy) * w + size_t(qx);
    const f3 alb = albedo ? mk3(albedo[3 * q], albedo[3 * q + 1], albedo[3 * q + 2]) : mk3(1.0f);
    return tpTexel(albedo != nullptr, rgba[4 * q], rgba[4 * q + 1], rgba[4 * q + 2], alb);
  }
};

template <bool MOMENTS>
static int run(std::vector<uint32_t>& in, const char* outPath) {
  constexpr size_t kHead = 13, planes = MOMENTS ? 4 : 3;
  const uint32_t w = in[0], h = in[1], frames = in[2], flags = in[3], inPlace = in[4], maxHistory = in[5], nNodes = in[7];
  const uint32_t clipRadius = in[8];
  const float clipGamma = asFloat(in[12]);
  const size_t n = size_t(w) * h;
  TpConst k{};
  k.alphaMin = asFloat(in[9]); k.normalCosMin = asFloat(in[10]); k.planeTolerance = asFloat(in[11]);
  k.maxHistory = maxHistory; k.minMomentHistory = in[6]; k.width = w; k.height = h;
  std::vector<f4> hist(n * planes * 2);
  uint32_t current = 0;
  bool have = false;
  YartCameraDesc prev{};
  std::vector<uint32_t> out;
  out.reserve(n * 6 * frames);
  size_t at = kHead;
  for (uint32_t fi = 0; fi < frames; fi++) {
    if (in.size() < at + 19 + n * 20) throw std::runtime_error("input ends inside a frame");
    uint32_t* words = in.data() + at;
    if (words[0]) have = false;
    const uint32_t motionKind = words[1];
    if (motionKind > 2u) throw std::runtime_error("a frame's motion is neither 0, 1 nor 2");
    YartCameraDesc cam;
    static_assert(sizeof(YartCameraDesc) == 68, "YartCameraDesc is 17 words");
    std::memcpy(&cam, words + 2, 68);
    if (cam.width != w || cam.height != h) throw std::runtime_error("a camera's image size is not the header's");
    float* fw = reinterpret_cast<float*>(words + 19);
    float* rgba = fw; fw += n * 4;
    float* variance = fw; fw += n;
    const float* position = fw; fw += n * 3;
    const float* normal = fw; fw += n * 3;
    const float* depth = fw; fw += n;
    const float* coverage = fw; fw += n;
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(fw); fw += n * 4;
    const float* albedo = (flags & 1u) ? fw : nullptr;
    fw += n * 3;
    at += 19 + n * 20;
    const float* records = fw;
    const size_t recordWords = motionKind == 1u ? size_t(nNodes) * 24 : motionKind == 2u ? n * 8 : 0;
    if (in.size() < at + recordWords) throw std::runtime_error("input ends inside a motion");
    at += recordWords;
    std::vector<float> sepRgba(inPlace ? 0 : n * 4), sepVar(inPlace ? 0 : n);
    float* oRgba = inPlace ? rgba : sepRgba.data();
    float* oVar = inPlace ? variance : sepVar.data();
    std::vector<float> staged;                     // the neighbours are read from a copy when the outputs overwrite the frame
    if (inPlace && clipRadius) staged.assign(rgba, rgba + n * 4);
    const float* frameRgba = staged.empty() ? rgba : staged.data();
    std::vector<uint32_t> oLen(n);
    k.haveHistory = have ? 1u : 0u;
    TpCamera pc{};
    if (have) pc = tpCamera(makeCamera(prev));
    const f4* hin = hist.data() + size_t(current) * n * planes;
    f4* hout = hist.data() + size_t(current ^ 1u) * n * planes;
    const HostHist hh{hin, hin + n, hin + 2 * n, hin + 3 * n};
    auto albedoOf = [&](size_t p) { return albedo ? mk3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]) : mk3(1.0f); };
    for (size_t p = 0; p < n; p++) {
      TpIn pi;
      pi.rgba = dnF4(frameRgba[4 * p], frameRgba[4 * p + 1], frameRgba[4 * p + 2], frameRgba[4 * p + 3]);
      pi.variance = variance[p]; pi.depth = depth[p]; pi.coverage = coverage[p]; pi.node = ids[4 * p];
      pi.P = mk3(position[3 * p], position[3 * p + 1], position[3 * p + 2]);
      pi.n = mk3(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]);
      auto withFrame = [&](const auto& motion) {
        if (clipRadius) {
          const HostFrame frame{frameRgba, albedo, w, h, uint32_t(p % w), uint32_t(p / w), clipRadius, clipGamma};
          return tpAccumulatePixel<MOMENTS>(hh, motion, frame, k, pc, pi, albedo != nullptr, albedoOf(p));
        }
        return tpAccumulatePixel<MOMENTS>(hh, motion, k, pc, pi, albedo != nullptr, albedoOf(p));
      };
      const TpOut o = motionKind == 1u   ? withFrame(HostMotion{records, nNodes})
                      : motionKind == 2u ? withFrame(HostPixelMotion{records + p * 8})
                                         : withFrame(TpNoMotion{});
      hout[p] = o.rec0; hout[n + p] = o.rec1; hout[2 * n + p] = o.rec2;
      if (MOMENTS) hout[3 * n + p] = o.rec3;
      oRgba[4 * p] = o.rgba.x; oRgba[4 * p + 1] = o.rgba.y; oRgba[4 * p + 2] = o.rgba.z; oRgba[4 * p + 3] = o.rgba.w;
      oVar[p] = o.variance;
      oLen[p] = o.length;
    }
    if (MOMENTS) {               // pass 2, on the image pass 1 wrote: neither a motion nor a clip in it
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
    }
    current ^= 1u; have = true; prev = cam;
    for (size_t i = 0; i < n * 4; i++) out.push_back(asWord(oRgba[i]));
    for (size_t i = 0; i < n; i++) out.push_back(asWord(oVar[i]));
    out.insert(out.end(), oLen.begin(), oLen.end());
  }
  if (at != in.size()) throw std::runtime_error("input size does not match the header");
  FILE* f = std::fopen(outPath, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + outPath);
  std::fwrite(out.data(), 4, out.size(), f);
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc != 3) {
      std::fprintf(stderr, "usage: temporalclipsim <in> <out>\n");
      return 1;
    }
    std::vector<uint32_t> in = readWords(argv[1]);
    if (in.size() < 13) throw std::runtime_error("short header");
    if (in[0] == 0 || in[1] == 0 || in[0] > 4096 || in[1] > 4096 || in[2] > 64 || in[3] > 1u || in[5] == 0 || in[6] == 1u ||
        in[7] == 0 || in[7] >= kTpMotionMaxNodes || in[8] > kTpClipMaxRadius)
      throw std::runtime_error("bad header");
    return in[6] ? run<true>(in, argv[2]) : run<false>(in, argv[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "temporalclipsim: %s\n", e.what());
    return 2;
  }
}
