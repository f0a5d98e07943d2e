// dn_host.hpp — TEST INFRASTRUCTURE shared by tests/denoisesim (the plain filter) and tests/momentsim `denoisevar` (the
// variance-guided one), never part of libyart_hip.so.
//
// yart_amd/csrc/denoise.hpp — the arithmetic of the à-trous filter that the device kernels call — compiled as host C++ and driven
// the way csrc/postprocess.inc drives the kernels: prepare pass, the iterations between two working images, finish pass, with the library's
// 48 bytes per pixel. VAR chooses the form, as in denoise.hpp.
//   in:  9 words {u32 width, height, iterations, flags, guides (1 albedo | 2 normal | 4 depth), in_place,
//                 f32 sigma_color (VAR: sigma_luma), sigma_normal, sigma_depth}, then the frame (w*h*4 f32), with VAR the variance
//        (w*h), and the guides that are present, in that order (w*h*3, w*h*3, w*h)
//   out: the filtered frame (w*h*4 f32); with in_place != 0 it is the input buffer itself that is filtered and written.
#pragma once
#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/denoise.hpp"

inline std::vector<float> readFloats(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot read ") + path);
  std::vector<float> v;
  float buf[4096];
  size_t n;
  while ((n = std::fread(buf, 4, 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}
inline void writeWords(const char* path, const void* p, size_t words) {
  FILE* f = std::fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
  std::fwrite(p, 4, words, f);
  std::fclose(f);
}
inline uint32_t asWord(float f) { return __builtin_bit_cast(uint32_t, f); }

struct DnHostSrc {
  const yart_hip::f4 *c, *g;
  yart_hip::f4 colour(size_t q) const { return c[q]; }
  yart_hip::f4 guide(size_t q) const { return g[q]; }
};

// albedo: only when the call demodulates; variance: only with VAR; out may be rgba
template <bool VAR>
void dnHostFilter(const float* rgba, const float* variance, const float* albedo, const float* normal, const float* depth, uint32_t w,
                  uint32_t h, uint32_t iterations, const yart_hip::DnConst& k, float* out) {
  using namespace yart_hip;
  const size_t n = size_t(w) * h;
  if (iterations == 0) {
    if (out != rgba) std::copy(rgba, rgba + n * 4, out);
    return;
  }
  std::vector<f4> scratch(n * 3);                    // working colour image 0 | image 1 | guide records
  f4 *img[2] = {scratch.data(), scratch.data() + n}, *guide = scratch.data() + 2 * n;
  for (size_t p = 0; p < n; p++)
    dnPrepare<VAR>(dnF4(rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]), albedo ? albedo + 3 * p : nullptr,
                   normal ? normal + 3 * p : nullptr, depth ? depth + p : nullptr, img[0][p], guide[p], VAR ? variance[p] : 0.0f);
  for (uint32_t i = 0; i < iterations; i++) {
    DnHostSrc src{img[i & 1u], guide};
    f4* dst = img[(i + 1u) & 1u];
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) dst[size_t(y) * w + x] = dnFilterPixel<VAR>(src, w, h, x, y, i, k);
  }
  const f4* last = img[iterations & 1u];
  for (size_t p = 0; p < n; p++) {
    const f4 o = dnFinish(last[p], albedo ? albedo + 3 * p : nullptr, rgba[4 * p + 3]);
    out[4 * p] = o.x; out[4 * p + 1] = o.y; out[4 * p + 2] = o.z; out[4 * p + 3] = o.w;
  }
}

// the input file, filtered, to the output file
template <bool VAR>
void dnHostRunFile(const char* inPath, const char* outPath) {
  std::vector<float> in = readFloats(inPath);        // (header words are decoded from their bit patterns)
  if (in.size() < 9) throw std::runtime_error("short header");
  const uint32_t w = asWord(in[0]), h = asWord(in[1]), iterations = asWord(in[2]), flags = asWord(in[3]), guides = asWord(in[4]);
  const uint32_t inPlace = asWord(in[5]);
  if (w == 0 || h == 0 || w > 4096 || h > 4096 || iterations > 8 || guides > 7u || flags > 1u || ((flags & 1u) && !(guides & 1u)))
    throw std::runtime_error("bad header");
  const size_t n = size_t(w) * h;
  const size_t need = 9 + n * (VAR ? 5 : 4) + ((guides & 1u) ? n * 3 : 0) + ((guides & 2u) ? n * 3 : 0) + ((guides & 4u) ? n : 0);
  if (in.size() != need) throw std::runtime_error("input size does not match the header");
  float* words = in.data() + 9;
  float* rgba = words; words += n * 4;
  const float *variance = nullptr, *albedo = nullptr, *normal = nullptr, *depth = nullptr;
  if (VAR) { variance = words; words += n; }
  if (guides & 1u) { albedo = words; words += n * 3; }
  if (guides & 2u) { normal = words; words += n * 3; }
  if (guides & 4u) { depth = words; words += n; }
  std::vector<float> separate(inPlace ? 0 : n * 4);
  float* out = inPlace ? rgba : separate.data();
  const yart_hip::DnConst k = yart_hip::dnConstants<VAR>(in[6], in[7], in[8], normal != nullptr, depth != nullptr);
  dnHostFilter<VAR>(rgba, variance, (flags & 1u) ? albedo : nullptr, normal, depth, w, h, iterations, k, out);
  writeWords(outPath, out, n * 4);
}
