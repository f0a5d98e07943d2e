// denoisesim.cpp — TEST INFRASTRUCTURE for tests/test_denoise.py, never part of libyart_hip.so.
//
// yart_amd/csrc/denoise.hpp — the arithmetic of the à-trous filter that the device kernels call — compiled as host C++ (as
// tests/hostsim and tests/aovsim compile the other device headers) and driven the way yart_hip.hip drives the kernels: prepare
// pass, the iterations between two working images, finish pass, with the library's 48 bytes per pixel.
//   denoisesim <in> <out>
//   in:  9 words {u32 width, height, iterations, flags, guides (1 albedo | 2 normal | 4 depth), in_place,
//                 f32 sigma_color, sigma_normal, sigma_depth}, then the frame (w*h*4 f32) and the guides that are present, in that
//        order (w*h*3, w*h*3, w*h)
//   out: the filtered frame (w*h*4 f32); with in_place != 0 it is the input buffer itself that is filtered and written.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/denoise.hpp"

using namespace yart_hip;

struct HostSrc {
  const f4 *c, *g;
  f4 colour(size_t q) const { return c[q]; }
  f4 guide(size_t q) const { return g[q]; }
};

static void denoise(const float* rgba, const float* albedo, const float* normal, const float* depth, uint32_t w, uint32_t h,
                    uint32_t iterations, bool demodulate, float sc, float sn, float sd, float* out) {
  const size_t n = size_t(w) * h;
  if (iterations == 0) {
    if (out != rgba) for (size_t k = 0; k < n * 4; k++) out[k] = rgba[k];
    return;
  }
  DnConst k;
  k.icol = dnInvSigma2(sc);
  k.inrm = normal ? dnInvSigma2(sn) : 0.0f;
  k.idep = depth ? dnInvSigma2(sd) : 0.0f;
  k.terms = (sc > 0.0f ? kDnColor : 0u) | (normal && sn > 0.0f ? kDnNormal : 0u) | (depth && sd > 0.0f ? kDnDepth : 0u);
  const float* alb = demodulate ? albedo : nullptr;
  std::vector<f4> scratch(n * 3);                    // colour image 0 | colour image 1 | guide records
  f4 *img[2] = {scratch.data(), scratch.data() + n}, *guide = scratch.data() + 2 * n;
  for (size_t p = 0; p < n; p++)
    dnPrepare(dnF4(rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]), alb ? alb + 3 * p : nullptr,
              normal ? normal + 3 * p : nullptr, depth ? depth + p : nullptr, img[0][p], guide[p]);
  for (uint32_t i = 0; i < iterations; i++) {
    HostSrc src{img[i & 1u], guide};
    f4* dst = img[(i + 1u) & 1u];
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) dst[size_t(y) * w + x] = dnFilterPixel(src, w, h, x, y, i, k);
  }
  const f4* last = img[iterations & 1u];
  for (size_t p = 0; p < n; p++) {
    const f4 o = dnFinish(last[p], alb ? alb + 3 * p : nullptr, rgba[4 * p + 3]);
    out[4 * p] = o.x; out[4 * p + 1] = o.y; out[4 * p + 2] = o.z; out[4 * p + 3] = o.w;
  }
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: denoisesim <in> <out>\n"); return 1; }
  try {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) throw std::runtime_error(std::string("cannot read ") + argv[1]);
    std::vector<float> in;                           // (header words are decoded from their bit patterns)
    float buf[4096];
    size_t got;
    while ((got = std::fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    if (in.size() < 9) throw std::runtime_error("short header");
    auto word = [&](size_t k) { return __builtin_bit_cast(uint32_t, in[k]); };
    const uint32_t w = word(0), h = word(1), iterations = word(2), flags = word(3), guides = word(4), inPlace = word(5);
    const float sc = in[6], sn = in[7], sd = in[8];
    if (w == 0 || h == 0 || w > 4096 || h > 4096 || iterations > 8 || guides > 7u || flags > 1u || ((flags & 1u) && !(guides & 1u)))
      throw std::runtime_error("bad header");
    const size_t n = size_t(w) * h;
    const size_t need = 9 + n * 4 + ((guides & 1u) ? n * 3 : 0) + ((guides & 2u) ? n * 3 : 0) + ((guides & 4u) ? n : 0);
    if (in.size() != need) throw std::runtime_error("input size does not match the header");
    float* words = in.data() + 9;
    float* rgba = words; words += n * 4;
    const float *albedo = nullptr, *normal = nullptr, *depth = nullptr;
    if (guides & 1u) { albedo = words; words += n * 3; }
    if (guides & 2u) { normal = words; words += n * 3; }
    if (guides & 4u) { depth = words; words += n; }
    std::vector<float> separate(inPlace ? 0 : n * 4);
    float* out = inPlace ? rgba : separate.data();
    denoise(rgba, albedo, normal, depth, w, h, iterations, (flags & 1u) != 0u, sc, sn, sd, out);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 2;
    std::fwrite(out, 4, n * 4, g);
    std::fclose(g);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "denoisesim: %s\n", e.what());
    return 2;
  }
}
