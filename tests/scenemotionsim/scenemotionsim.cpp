// scenemotionsim.cpp — TEST INFRASTRUCTURE for tests/test_pixel_motion.py, never part of libyart_hip.so.
//
// csrc/scene_motion.hpp (smNodeChain, smPixel) and csrc/temporal.hpp with a per-pixel Motion, compiled as host C++ and driven the way
// csrc/scene_motion_kernels.inc and csrc/postprocess.inc drive the kernels.
//
//   scenemotionsim motion <in> <out>
//     in: 6 words {u32 width, height, n_nodes, n_meshes, n_tris, n_verts}, then the previous node array (n_nodes NodeDev records of 44
//     words), the current one, the mesh records (n_meshes MeshDev of 16 words), triVerts (n_tris * 4 u32), the current vPos (n_verts * 4
//     f32), the previous vPos, position (w*h*3 f32), normal (w*h*3), coverage (w*h), ids (w*h*4 i32); out: the records (w*h*8 words)
//   scenemotionsim <in> <out>
//     the input and output of tests/temporalmotionsim, except that a frame's motion is its per-pixel records (w*h*8 words; the
//     header's n_nodes is not looked at)
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/scene_motion.hpp"
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
static void writeWords(const char* path, const std::vector<uint32_t>& out) {
  FILE* f = std::fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
  std::fwrite(out.data(), 4, out.size(), f);
  std::fclose(f);
}
static float asFloat(uint32_t u) { return __builtin_bit_cast(float, u); }
static uint32_t asWord(float f) { return __builtin_bit_cast(uint32_t, f); }

// ---------------------------------------------------------------------------------------------------------------------
// motion
// ---------------------------------------------------------------------------------------------------------------------
struct HostScene {
  const f4* chains; const MeshDev* meshes; const u4* triVerts; const f4 *vCur, *vPrev;
  uint32_t nNodes;
  uint32_t nodes() const { return nNodes; }
  f4 chain(uint32_t node, uint32_t i) const { return chains[size_t(node) * kSmChainWords + i]; }
  u4 mesh(uint32_t m, uint32_t i) const { return reinterpret_cast<const u4*>(meshes + m)[i]; }
  u4 tri(size_t t) const { return triVerts[t]; }
  f4 cur(size_t v) const { return vCur[v]; }
  f4 prev(size_t v) const { return vPrev[v]; }
};

static int runMotion(const std::vector<uint32_t>& in, const char* outPath) {
  static_assert(sizeof(NodeDev) == 176 && sizeof(MeshDev) == 64, "NodeDev is 44 words and MeshDev 16");
  if (in.size() < 6) throw std::runtime_error("short header");
  const uint32_t w = in[0], h = in[1], nNodes = in[2], nMeshes = in[3], nTris = in[4], nVerts = in[5];
  const size_t n = size_t(w) * h;
  if (w == 0 || h == 0 || w > 4096 || h > 4096 || nNodes == 0) throw std::runtime_error("bad header");
  const size_t want = 6 + size_t(nNodes) * 88 + size_t(nMeshes) * 16 + size_t(nTris) * 4 + size_t(nVerts) * 8 + n * 11;
  if (in.size() != want) throw std::runtime_error("input size does not match the header");
  // (copies: the records need their own alignment)
  std::vector<NodeDev> prev(nNodes), cur(nNodes);
  std::vector<MeshDev> meshes(nMeshes);
  std::vector<u4> tris(nTris);
  std::vector<f4> vCur(nVerts), vPrev(nVerts);
  const uint32_t* at = in.data() + 6;
  auto take = [&](void* dst, size_t words) { std::memcpy(dst, at, words * 4); at += words; };
  take(prev.data(), size_t(nNodes) * 44); take(cur.data(), size_t(nNodes) * 44);
  take(meshes.data(), size_t(nMeshes) * 16); take(tris.data(), size_t(nTris) * 4);
  take(vCur.data(), size_t(nVerts) * 4); take(vPrev.data(), size_t(nVerts) * 4);
  const float* position = reinterpret_cast<const float*>(at);
  const float* normal = position + n * 3;
  const float* coverage = normal + n * 3;
  const uint32_t* ids = at + n * 7;
  for (uint32_t i = 0; i < nNodes; i++) {
    if (cur[i].parent >= int32_t(i) || cur[i].parent != prev[i].parent || cur[i].mesh >= int32_t(nMeshes)) throw std::runtime_error("bad node");
  }
  for (const MeshDev& m : meshes)
    if (size_t(m.triOffset) + m.nTris > nTris || size_t(m.vertOffset) + m.nVerts > nVerts) throw std::runtime_error("bad mesh");
  for (uint32_t m = 0; m < nMeshes; m++)
    for (uint32_t t = 0; t < meshes[m].nTris; t++) {
      const u4 tv = tris[meshes[m].triOffset + t];
      if (tv.x >= meshes[m].nVerts || tv.y >= meshes[m].nVerts || tv.z >= meshes[m].nVerts) throw std::runtime_error("bad triangle");
    }
  std::vector<f4> chains(size_t(nNodes) * kSmChainWords);
  for (uint32_t i = 0; i < nNodes; i++) smNodeChain(prev.data(), cur.data(), i, chains.data() + size_t(i) * kSmChainWords);
  const HostScene sc{chains.data(), meshes.data(), tris.data(), vCur.data(), vPrev.data(), nNodes};
  std::vector<uint32_t> out(n * 8);
  for (size_t p = 0; p < n; p++) {
    f4 w0, w1;
    smPixel(sc, mk3(position[3 * p], position[3 * p + 1], position[3 * p + 2]), mk3(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]),
            coverage[p], ids[4 * p], ids[4 * p + 3], w0, w1);
    const float r[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    for (int k = 0; k < 8; k++) out[8 * p + k] = asWord(r[k]);
  }
  writeWords(outPath, out);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// temporal
// ---------------------------------------------------------------------------------------------------------------------
struct HostHist {
  const f4 *r0, *r1, *r2, *r3;
  f4 rec0(size_t q) const { return r0[q]; }
  f4 rec1(size_t q) const { return r1[q]; }
  f4 rec2(size_t q) const { return r2[q]; }
  f4 rec3(size_t q) const { return r3[q]; }
};
struct HostPixelMotion {
  static constexpr bool kNone = false, kPixel = true;
  const float* rec;                      // the pixel's 8 floats
  f4 word(uint32_t i) const { return dnF4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]); }
};

template <bool MOMENTS>
static int runTemporal(std::vector<uint32_t>& in, const char* outPath) {
  constexpr size_t kHead = 11, planes = MOMENTS ? 4 : 3;
  const uint32_t w = in[0], h = in[1], frames = in[2], flags = in[3], inPlace = in[4], maxHistory = in[5];
  const size_t n = size_t(w) * h;
  TpConst k{};
  k.alphaMin = asFloat(in[8]); k.normalCosMin = asFloat(in[9]); k.planeTolerance = asFloat(in[10]);
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
    const bool haveMotion = words[1] != 0u;
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
    if (haveMotion) {
      if (in.size() < at + n * 8) throw std::runtime_error("input ends inside a motion");
      at += n * 8;
    }
    std::vector<float> sepRgba(inPlace ? 0 : n * 4), sepVar(inPlace ? 0 : n);
    float* oRgba = inPlace ? rgba : sepRgba.data();
    float* oVar = inPlace ? variance : sepVar.data();
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
      pi.rgba = dnF4(rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]);
      pi.variance = variance[p]; pi.depth = depth[p]; pi.coverage = coverage[p]; pi.node = ids[4 * p];
      pi.P = mk3(position[3 * p], position[3 * p + 1], position[3 * p + 2]);
      pi.n = mk3(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]);
      const TpOut o = haveMotion ? tpAccumulatePixel<MOMENTS>(hh, HostPixelMotion{records + 8 * p}, k, pc, pi, albedo != nullptr, albedoOf(p))
                                 : tpAccumulatePixel<MOMENTS>(hh, k, pc, pi, albedo != nullptr, albedoOf(p));
      hout[p] = o.rec0; hout[n + p] = o.rec1; hout[2 * n + p] = o.rec2;
      if (MOMENTS) hout[3 * n + p] = o.rec3;
      oRgba[4 * p] = o.rgba.x; oRgba[4 * p + 1] = o.rgba.y; oRgba[4 * p + 2] = o.rgba.z; oRgba[4 * p + 3] = o.rgba.w;
      oVar[p] = o.variance;
      oLen[p] = o.length;
    }
    if (MOMENTS) {               // pass 2, on the image pass 1 wrote: no motion in it
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
  writeWords(outPath, out);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 4 && std::string(argv[1]) == "motion") return runMotion(readWords(argv[2]), argv[3]);
    if (argc != 3) {
      std::fprintf(stderr, "usage: scenemotionsim [motion] <in> <out>\n");
      return 1;
    }
    std::vector<uint32_t> in = readWords(argv[1]);
    if (in.size() < 11) throw std::runtime_error("short header");
    if (in[0] == 0 || in[1] == 0 || in[0] > 4096 || in[1] > 4096 || in[2] > 64 || in[3] > 1u || in[5] == 0 || in[6] == 1u)
      throw std::runtime_error("bad header");
    return in[6] ? runTemporal<true>(in, argv[2]) : runTemporal<false>(in, argv[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "scenemotionsim: %s\n", e.what());
    return 2;
  }
}
