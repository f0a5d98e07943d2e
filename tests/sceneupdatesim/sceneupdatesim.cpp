// sceneupdatesim — csrc/scene_update.hpp on the host against host_scene.hpp::buildHostImage (tests/test_scene_update_host.py).
//
//   sceneupdatesim OLD.yscn NEW.yscn [seed]
//
// OLD and NEW are one scene with two sets of node / light transforms. The program builds buildHostImage(NEW) — what a freshly created
// scene holds — and re-derives it from buildHostImage(OLD) with NEW's transforms through the functions of scene_update.hpp, byte for
// byte: the NodeDev records, the nodeWorld pairs, the lights, the power CDF, the total power, allIdentity, and the top-level hierarchy
// rebuilt by buildTopLevel. The fold of the children's contributions runs four ways: suRederiveHost (the library's path for deep
// scenes), children in ascending order, in descending order, and in a seeded shuffle split into 7 partial folds that are then
// combined. It prints one line per comparison and `SIGNED_ZERO_TIE node bound` wherever two candidates of one bound are equal as
// floats and differ in bits. Exit status 0: everything equal.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static int failures = 0;
static void same(const char* what, const void* a, const void* b, size_t n) {
  const bool ok = std::memcmp(a, b, n) == 0;
  std::printf("%s %s (%zu bytes)\n", ok ? "EQUAL" : "DIFFERENT", what, n);
  if (!ok) failures++;
}

enum Order { kAscending, kDescending, kShuffled7 };

// steps 1-3 with the fold of every parent in the given order (scene_update.hpp's functions, level by level as the kernels run them)
static void rederive(HostImage& im, const YartNodeDesc* desc, Order order, uint32_t seed, bool reportTies) {
  const uint32_t nn = uint32_t(im.nodes.size());
  std::vector<uint32_t> flags(nn);
  im.allIdentity = suIdentityFlags(desc, nn, flags.data());
  std::vector<std::vector<uint32_t>> children(nn);
  uint32_t levels = 0;
  for (uint32_t i = 0; i < nn; i++) {
    NodeDev& nd = im.nodes[i];
    std::memcpy(nd.xf.fwd, desc[i].fwd, 64); std::memcpy(nd.xf.inv, desc[i].inv, 64);
    nd.pad[0] = flags[i];
    const SuBox own = nd.mesh >= 0 ? im.meshBox[nd.mesh] : suEmptyBox();
    for (int c = 0; c < 3; c++) { nd.bmin[c] = own.mn[c]; nd.bmax[c] = own.mx[c]; }
    if (i > 0) children[nd.parent].push_back(i);
    levels = std::max(levels, nd.depth + 1u);
  }
  std::mt19937 rng(seed);
  for (uint32_t level = levels; level-- > 0u;)
    for (uint32_t p = 0; p < nn; p++) {
      if (im.nodes[p].depth != level || children[p].empty()) continue;
      std::vector<uint32_t> ch = children[p];
      if (order == kDescending) std::reverse(ch.begin(), ch.end());
      if (order == kShuffled7) std::shuffle(ch.begin(), ch.end(), rng);
      std::vector<SuFold> cand;
      for (uint32_t c : ch) cand.push_back(suFoldOf(suChildContribution(im.nodes[c].xf.fwd, im.nodes[c].bmin, im.nodes[c].bmax), c));
      SuBox own;
      for (int c = 0; c < 3; c++) { own.mn[c] = im.nodes[p].bmin[c]; own.mx[c] = im.nodes[p].bmax[c]; }
      const SuFold ownFold = suFoldOf(own, kSuOwnBox);
      if (reportTies) {
        std::vector<SuFold> all = cand;
        all.push_back(ownFold);
        for (int b = 0; b < 6; b++) {
          bool tie = false;
          for (size_t x = 0; x < all.size(); x++)
            for (size_t y = x + 1; y < all.size(); y++) {
              const float u = b < 3 ? all[x].mn[b] : all[x].mx[b - 3], v = b < 3 ? all[y].mn[b] : all[y].mx[b - 3];
              if (u == v && std::memcmp(&u, &v, 4) != 0) tie = true;
            }
          if (tie) std::printf("SIGNED_ZERO_TIE %u %d\n", p, b);
        }
      }
      SuFold f = suFoldIdentity();
      if (order == kShuffled7) {
        SuFold part[7];
        for (SuFold& q : part) q = suFoldIdentity();
        for (size_t k = 0; k < cand.size(); k++) suFoldJoin(part[k % 7], cand[k]);
        std::vector<int> po = {3, 6, 0, 5, 1, 4, 2};
        for (int k : po) suFoldJoin(f, part[k]);
        SuFold g = ownFold;                                // ... and the own box as the LEFT operand
        suFoldJoin(g, f);
        f = g;
      } else {
        for (const SuFold& q : cand) suFoldJoin(f, q);
        suFoldJoin(f, ownFold);
      }
      for (int c = 0; c < 3; c++) { im.nodes[p].bmin[c] = f.mn[c]; im.nodes[p].bmax[c] = f.mx[c]; }
    }
  for (uint32_t i = 0; i < nn; i++) suWorldBox(im.nodes.data(), i, &im.nodeWorld[2 * i].x, &im.nodeWorld[2 * i + 1].x);
}

static void compare(const char* tag, const HostImage& got, const HostImage& want) {
  std::string t(tag);
  same((t + " nodes").c_str(), got.nodes.data(), want.nodes.data(), want.nodes.size() * sizeof(NodeDev));
  same((t + " nodeWorld").c_str(), got.nodeWorld.data(), want.nodeWorld.data(), want.nodeWorld.size() * sizeof(f4));
  const uint32_t a = got.allIdentity, b = want.allIdentity;
  same((t + " allIdentity").c_str(), &a, &b, 4);
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: sceneupdatesim OLD.yscn NEW.yscn [seed]\n"); return 2; }
  const uint32_t seed = argc > 3 ? uint32_t(std::atoi(argv[3])) : 1u;
  auto a = loadSceneFile(argv[1]);
  auto b = loadSceneFile(argv[2]);
  const HostImage old = buildHostImage(a->desc), want = buildHostImage(b->desc);
  if (a->desc.n_nodes != b->desc.n_nodes || a->desc.n_lights != b->desc.n_lights) { std::fprintf(stderr, "the scenes differ in their counts\n"); return 2; }
  const uint32_t nn = b->desc.n_nodes;
  std::printf("nodes %u levels %u lights %u tlas %zu\n", nn, old.maxNodeDepth + 1u, old.nLights, old.tlas.size());
  {
    HostImage im = old;
    std::vector<uint32_t> flags(nn);
    im.allIdentity = suIdentityFlags(b->desc.nodes, nn, flags.data());
    std::vector<SuFold> scratch(nn);
    suRederiveHost(im.nodes.data(), im.nodeWorld.data(), nn, b->desc.nodes, flags.data(), im.meshBox.data(), scratch.data());
    compare("host-path", im, want);
    // the top-level hierarchy rebuilt from the re-derived world boxes, and the lights
    const uint32_t height = buildTopLevel(im.nodes, im.nodeWorld, im.tlas);
    if (im.tlas.empty()) im.tlas.resize(1);
    same("rebuilt tlas", im.tlas.data(), want.tlas.data(), want.tlas.size() * sizeof(TlasNode));
    same("tlas height", &height, &want.tlasHeight, 4);
    rederiveLights(im, b->desc.lights, b->desc.n_lights);
    same("lights", im.lights.data(), want.lights.data(), want.lights.size() * sizeof(LightDev));
    same("areaPowerCdf", im.areaPowerCdf.data(), want.areaPowerCdf.data(), want.areaPowerCdf.size() * 4);
    same("totalPower", &im.totalPower, &want.totalPower, 4);
  }
  const char* names[3] = {"ascending", "descending", "shuffled-7"};
  for (int o = 0; o < 3; o++) {
    HostImage im = old;
    rederive(im, b->desc.nodes, Order(o), seed, o == 0);
    compare(names[o], im, want);
  }
  {   // and back: OLD's transforms over NEW's image give OLD's image
    HostImage im = want;
    rederive(im, a->desc.nodes, kShuffled7, seed + 1u, false);
    compare("round-trip", im, old);
  }
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
