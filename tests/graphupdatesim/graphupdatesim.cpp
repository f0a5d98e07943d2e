// graphupdatesim — csrc/graph_update.hpp on the host against host_scene.hpp::buildHostImage (tests/test_graph_update_host.py).
//
//   graphupdatesim OLD.yscn NEW.yscn
//
// OLD and NEW are one scene with two node lists (meshes, materials, textures and lights alike). The program builds
// buildHostImage(NEW) — what a freshly created scene holds — and derives it from buildHostImage(OLD) with NEW's node list the way
// yart_hip_scene_update_graph does: guDerive + guApplyHost for the topology, scene_update.hpp for what depends on the transforms,
// buildTopLevel for the hierarchy. Two ways: `host-path` with suRederiveHost (the library's path for graphs of more than
// kSceneUpdateMaxLevels levels), and `tables` level by level over guDerive's CSR and level tables, as the kernels walk them (graphs
// within that limit). Then the way back, NEW's image with OLD's list. One line per comparison; exit status 0: everything equal.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/graph_update.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static int failures = 0;
static void same(const std::string& what, const void* a, const void* b, size_t n) {
  const bool ok = n == 0 || std::memcmp(a, b, n) == 0;          // (an empty vector's data() may be null)
  std::printf("%s %s (%zu bytes)\n", ok ? "EQUAL" : "DIFFERENT", what.c_str(), n);
  if (!ok) failures++;
}
static void sameCount(const std::string& what, size_t a, size_t b) {
  std::printf("%s %s (%zu, %zu)\n", a == b ? "EQUAL" : "DIFFERENT", what.c_str(), a, b);
  if (a != b) failures++;
}

constexpr uint32_t kFanOut = 32;                      // scene_update_kernels.inc::kSuFanOut

// what the update leaves in the image besides the node records: sizes, hierarchy, stack bound, identity
static void finish(HostImage& im, const GuDerived& g) {
  im.tlasHeight = buildTopLevel(im.nodes, im.nodeWorld, im.tlas);
  if (im.tlas.empty()) im.tlas.resize(1);
  im.maxNodeDepth = g.maxNodeDepth;
  im.stackBound = im.tlasHeight;
  for (uint32_t need : im.meshStackNeed) im.stackBound = std::max(im.stackBound, need);
  im.allIdentity = g.allIdentity;
}

static void hostPath(HostImage& im, const YartNodeDesc* desc, uint32_t nn, const GuDerived& g) {
  im.nodes.resize(nn); im.nodeWorld.resize(size_t(nn) * 2u);
  guApplyHost(g, im.nodes.data(), im.nodeWorld.data());
  std::vector<SuFold> scratch(nn);
  suRederiveHost(im.nodes.data(), im.nodeWorld.data(), nn, desc, g.flags.data(), im.meshBox.data(), scratch.data());
  finish(im, g);
}

// k_gu_topology, k_su_scatter, k_su_fold per level over the tables, k_su_world — one loop iteration per lane or workgroup
static void tablePath(HostImage& im, const YartNodeDesc* desc, uint32_t nn, const GuDerived& g) {
  im.nodes.assign(nn, NodeDev{}); im.nodeWorld.assign(size_t(nn) * 2u, f4{});        // (a grown buffer holds nothing of the old list)
  for (uint32_t i = 0; i < nn; i++) guApplyNode(g.topo[i], i, nn, im.nodes[i], im.nodeWorld[2u * i], im.nodeWorld[2u * i + 1u]);
  for (uint32_t i = 0; i < nn; i++) {
    NodeDev& nd = im.nodes[i];
    std::memcpy(nd.xf.fwd, desc[i].fwd, 64); std::memcpy(nd.xf.inv, desc[i].inv, 64);
    nd.pad[0] = g.flags[i];
    const SuBox own = nd.mesh >= 0 ? im.meshBox[nd.mesh] : suEmptyBox();
    for (int c = 0; c < 3; c++) { nd.bmin[c] = own.mn[c]; nd.bmax[c] = own.mx[c]; }
  }
  for (uint32_t l = g.levels; l-- > 0u;)
    for (uint32_t k = 0; k < g.levelBig[l] + g.levelSmall[l]; k++) {
      const uint32_t p = g.parents[g.levelFirst[l] + k];
      const uint32_t nc = g.childOff[p + 1u] - g.childOff[p];
      if (im.nodes[p].depth != l || nc == 0u || (k < g.levelBig[l]) != (nc >= kFanOut)) { std::printf("DIFFERENT tables: parent %u in the wrong list\n", p); failures++; }
      SuFold f = suFoldIdentity();
      for (uint32_t q = g.childOff[p]; q < g.childOff[p + 1u]; q++) {
        const NodeDev& cn = im.nodes[g.childIdx[q]];
        if (uint32_t(cn.parent) != p) { std::printf("DIFFERENT tables: child %u of %u\n", g.childIdx[q], p); failures++; }
        suFoldJoin(f, suFoldOf(suChildContribution(cn.xf.fwd, cn.bmin, cn.bmax), g.childIdx[q]));
      }
      SuBox own;
      for (int c = 0; c < 3; c++) { own.mn[c] = im.nodes[p].bmin[c]; own.mx[c] = im.nodes[p].bmax[c]; }
      suFoldJoin(f, suFoldOf(own, kSuOwnBox));
      for (int c = 0; c < 3; c++) { im.nodes[p].bmin[c] = f.mn[c]; im.nodes[p].bmax[c] = f.mx[c]; }
    }
  for (uint32_t i = 0; i < nn; i++) suWorldBox(im.nodes.data(), i, &im.nodeWorld[2u * i].x, &im.nodeWorld[2u * i + 1u].x);
  finish(im, g);
}

static void compare(const std::string& t, const HostImage& got, const HostImage& want) {
  sameCount(t + " node count", got.nodes.size(), want.nodes.size());
  if (got.nodes.size() != want.nodes.size()) return;
  same(t + " nodes", got.nodes.data(), want.nodes.data(), want.nodes.size() * sizeof(NodeDev));
  same(t + " nodeWorld", got.nodeWorld.data(), want.nodeWorld.data(), want.nodeWorld.size() * sizeof(f4));
  sameCount(t + " tlas records", got.tlas.size(), want.tlas.size());
  if (got.tlas.size() == want.tlas.size()) same(t + " tlas", got.tlas.data(), want.tlas.data(), want.tlas.size() * sizeof(TlasNode));
  same(t + " tlasHeight", &got.tlasHeight, &want.tlasHeight, 4);
  same(t + " stackBound", &got.stackBound, &want.stackBound, 4);
  same(t + " maxNodeDepth", &got.maxNodeDepth, &want.maxNodeDepth, 4);
  const uint32_t a = got.allIdentity, b = want.allIdentity;
  same(t + " allIdentity", &a, &b, 4);
}

static void derive(const std::string& tag, const HostImage& from, const YartSceneDesc& d, const HostImage& want) {
  GuDerived g;
  guDerive(d.nodes, d.n_nodes, kFanOut, g);
  // the shape of the hierarchy, known before it is built
  std::vector<int32_t> mesh(d.n_nodes);
  for (uint32_t i = 0; i < d.n_nodes; i++) mesh[i] = d.nodes[i].mesh;
  const std::vector<uint32_t> leafIds = tlasLeafIds(mesh.data(), d.n_nodes);
  sameCount(tag + "leaf count", g.leafIds.size(), leafIds.size());
  if (g.leafIds.size() == leafIds.size()) same(tag + "leafIds", g.leafIds.data(), leafIds.data(), leafIds.size() * 4u);
  const bool hasTree = want.tlas.size() > 1u || want.tlas[0].b;
  sameCount(tag + "predicted tlas records", g.tlasRecords, hasTree ? want.tlas.size() : 0u);
  sameCount(tag + "predicted tlas height", g.tlasHeight, want.tlasHeight);
  {
    HostImage im = from;
    hostPath(im, d.nodes, d.n_nodes, g);
    compare(tag + "host-path", im, want);
  }
  if (g.levels <= kSceneUpdateMaxLevels) {
    HostImage im = from;
    tablePath(im, d.nodes, d.n_nodes, g);
    compare(tag + "tables", im, want);
  } else {
    std::printf("NOTE %s%u levels: no tables, the host path alone\n", tag.c_str(), g.levels);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: graphupdatesim OLD.yscn NEW.yscn\n"); return 2; }
  auto a = loadSceneFile(argv[1]);
  auto b = loadSceneFile(argv[2]);
  if (a->desc.n_meshes != b->desc.n_meshes || a->desc.n_lights != b->desc.n_lights) { std::fprintf(stderr, "the scenes differ in their meshes or lights\n"); return 2; }
  const HostImage old = buildHostImage(a->desc), want = buildHostImage(b->desc);
  std::printf("nodes %u -> %u levels %u -> %u tlas %zu -> %zu\n", a->desc.n_nodes, b->desc.n_nodes, old.maxNodeDepth + 1u, want.maxNodeDepth + 1u,
              old.tlas.size(), want.tlas.size());
  derive("", old, b->desc, want);
  derive("round-trip ", want, a->desc, old);
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
