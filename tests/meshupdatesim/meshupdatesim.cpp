// meshupdatesim — csrc/mesh_update.hpp on the host against host_scene.hpp::buildHostImage (tests/test_mesh_update_host.py).
//
//   meshupdatesim OLD.yscn NEW.yscn
//
// OLD and NEW are one scene with two sets of vertex positions (and normals / tangents). The program builds buildHostImage(NEW) — what
// a freshly created scene holds — and re-derives, from buildHostImage(OLD) and NEW's vertices, what yart_hip_scene_update_meshes
// re-derives, by the host statement of mesh_update.hpp fed with the host builder's tree: per mesh the link-word node array, the leaf
// records, the alpha flag, the stack need and the vertex box; then the scene's stack bound, the lights (rederiveLights over the new
// vertices) and the nodes' boxes and world boxes (suRederiveHost over the new vertex boxes). Everything is compared byte for byte.
// One line per mesh: `mesh I changed C nodes N was M need D was E alpha A`, `NEGATIVE_ZERO mesh I` where a vertex-box word is -0.0f, one
// line per comparison. Exit status 0: everything equal.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/mesh_update.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static int failures = 0;
static void same(const std::string& what, const void* a, const void* b, size_t n) {
  const bool ok = std::memcmp(a, b, n) == 0;
  std::printf("%s %s (%zu bytes)\n", ok ? "EQUAL" : "DIFFERENT", what.c_str(), n);
  if (!ok) failures++;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: meshupdatesim OLD.yscn NEW.yscn\n"); return 2; }
  auto a = loadSceneFile(argv[1]);
  auto b = loadSceneFile(argv[2]);
  const HostImage old = buildHostImage(a->desc), want = buildHostImage(b->desc);
  if (a->desc.n_meshes != b->desc.n_meshes || a->desc.n_nodes != b->desc.n_nodes || a->desc.n_lights != b->desc.n_lights) {
    std::fprintf(stderr, "the scenes differ in their counts\n");
    return 2;
  }
  HostImage im = old;
  std::vector<uint32_t> flags;
  for (const MaterialDev& m : im.materials) flags.push_back(m.flags);
  std::printf("meshes %u stackBound %u was %u\n", b->desc.n_meshes, want.stackBound, old.stackBound);
  for (uint32_t mi = 0; mi < b->desc.n_meshes; mi++) {
    const YartMeshDesc& m = b->desc.meshes[mi];
    const MeshDev& md = im.meshes[mi];
    const MeshDev& wd = want.meshes[mi];
    if (m.n_vertices != md.nVerts || m.n_faces != md.nTris || md.leafOffset != wd.leafOffset || md.triOffset != wd.triOffset) {
      std::fprintf(stderr, "mesh %u: the scenes differ in its counts\n", mi);
      return 2;
    }
    const bool changed = std::memcmp(m.positions, a->desc.meshes[mi].positions, size_t(m.n_vertices) * 12) != 0;
    // the host builder's tree over the new vertices and the image's own faces
    SahBvhBuilder hb;
    hb.setThreads(1);
    hb.build(m.positions, reinterpret_cast<const uint32_t*>(im.triVerts.data() + md.triOffset), 4, md.nTris);
    std::vector<BvhNode> nodes(hb.nodes.size());
    std::vector<LeafTri> leaf(md.nTris);
    const MuDerived d = muDeriveHost(hb.nodes.data(), uint32_t(hb.nodes.size()), hb.indices.data(), md.nTris, m.positions, im.triVerts.data() + md.triOffset,
                                     md.triOffset, flags.data(), nodes.data(), leaf.data());
    const SuBox box = muVertexBox(m.positions, m.n_vertices);
    std::printf("mesh %u changed %d nodes %zu was %u need %u was %u alpha %u\n", mi, int(changed), nodes.size(), md.nNodes, d.stackNeed,
                old.meshStackNeed[mi], d.hasAlpha);
    for (int c = 0; c < 3; c++) {
      uint32_t lo, hi;
      std::memcpy(&lo, &box.mn[c], 4); std::memcpy(&hi, &box.mx[c], 4);
      if (lo == 0x80000000u || hi == 0x80000000u) std::printf("NEGATIVE_ZERO mesh %u\n", mi);
    }
    const std::string t = "mesh " + std::to_string(mi) + " ";
    const uint32_t nn = uint32_t(nodes.size());
    same(t + "node count", &nn, &wd.nNodes, 4);
    if (nn == wd.nNodes) same(t + "nodes", nodes.data(), want.bvhNodes.data() + wd.nodeOffset, nodes.size() * sizeof(BvhNode));
    same(t + "leaves", leaf.data(), want.leafTris.data() + wd.leafOffset, leaf.size() * sizeof(LeafTri));
    same(t + "hasAlpha", &d.hasAlpha, &wd.hasAlpha, 4);
    same(t + "stack need", &d.stackNeed, &want.meshStackNeed[mi], 4);
    const uint32_t viaCreate = bvhStackNeed(hb.nodes.data(), hb.nodes.size());
    same(t + "stack need (bvhStackNeed)", &d.stackNeed, &viaCreate, 4);
    same(t + "vertex box", &box, &want.meshBox[mi], sizeof(SuBox));
    same(t + "indices", hb.indices.data(), want.bvhIndices[mi].data(), size_t(md.nTris) * 4);
    // into the image, as the library keeps its host copy
    im.meshStackNeed[mi] = d.stackNeed;
    im.meshBox[mi] = box;
    for (uint32_t v = 0; v < m.n_vertices; v++) {
      f4& p = im.vPos[md.vertOffset + v];
      p.x = m.positions[3 * v]; p.y = m.positions[3 * v + 1]; p.z = m.positions[3 * v + 2]; p.w = 0;
    }
  }
  uint32_t bound = im.tlasHeight;
  for (uint32_t need : im.meshStackNeed) bound = std::max(bound, need);
  same("stack bound", &bound, &want.stackBound, 4);
  same("vPos", im.vPos.data(), want.vPos.data(), want.vPos.size() * sizeof(f4));
  {
    const std::vector<YartLightDesc> desc = im.lightDesc;
    rederiveLights(im, desc.data(), im.nLights);
    same("lights", im.lights.data(), want.lights.data(), want.lights.size() * sizeof(LightDev));
    same("areaPowerCdf", im.areaPowerCdf.data(), want.areaPowerCdf.data(), want.areaPowerCdf.size() * 4);
    same("totalPower", &im.totalPower, &want.totalPower, 4);
  }
  {
    const uint32_t nn = uint32_t(im.nodes.size());
    std::vector<uint32_t> nf(nn);
    (void)suIdentityFlags(b->desc.nodes, nn, nf.data());
    std::vector<SuFold> scratch(nn);
    suRederiveHost(im.nodes.data(), im.nodeWorld.data(), nn, b->desc.nodes, nf.data(), im.meshBox.data(), scratch.data());
    same("nodes", im.nodes.data(), want.nodes.data(), want.nodes.size() * sizeof(NodeDev));
    same("nodeWorld", im.nodeWorld.data(), want.nodeWorld.data(), want.nodeWorld.size() * sizeof(f4));
    std::vector<TlasNode> tlas;
    (void)buildTopLevel(im.nodes, im.nodeWorld, tlas);
    if (tlas.empty()) tlas.resize(1);
    same("rebuilt tlas", tlas.data(), want.tlas.data(), want.tlas.size() * sizeof(TlasNode));
  }
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
