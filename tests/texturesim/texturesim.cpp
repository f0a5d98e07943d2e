// texturesim — csrc/texture_update.hpp on the host against host_scene.hpp::buildHostImage (tests/test_texture_update_host.py).
//
//   texturesim OLD.yscn NEW.yscn
//
// OLD and NEW are one scene with two sets of texels in its 8-bit textures. The program builds buildHostImage(NEW) — what a freshly
// created scene holds — and re-derives it from buildHostImage(OLD) and NEW's texels the way yart_hip_scene_update_textures does, with
// the functions of texture_update.hpp driven as the kernels of texture_update_kernels.inc drive them: one call per RGBA word, per
// leaf record and per node, records and nodes visited in a scrambled order, the link words rewritten in place on the final node
// array. texU8, materials, leaf records, BVH nodes, mesh records and texture records are compared byte for byte. One line `texture T
// changed C places P` per 8-bit texture, `material M alpha A was B` per material with a 4-channel base map that changed, `mesh K
// nodes N withBit A withoutBit B chain C maxSpan S` per mesh (of the updated image; C: the chain ran; S: its longest leaf), `flipped F`,
// one line per comparison.
// Exit status 0: everything equal; 3: scene creation refuses OLD or NEW.
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"
#include "../../yart_amd/csrc/texture_update.hpp"

using namespace yart_hip;

static int failures = 0;
static void same(const std::string& what, const void* a, const void* b, size_t n) {
  const bool ok = std::memcmp(a, b, n) == 0;
  std::printf("%s %s (%zu bytes)\n", ok ? "EQUAL" : "DIFFERENT", what.c_str(), n);
  if (!ok) failures++;
}
static std::vector<size_t> scrambled(size_t n, uint32_t seed) {
  std::vector<size_t> v(n);
  std::iota(v.begin(), v.end(), size_t(0));
  std::mt19937 rng(seed);
  for (size_t i = n; i > 1; i--) std::swap(v[i - 1], v[rng() % i]);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: texturesim OLD.yscn NEW.yscn\n"); return 2; }
  auto a = loadSceneFile(argv[1]);
  auto b = loadSceneFile(argv[2]);
  HostImage old, want;
  try {
    old = buildHostImage(a->desc); want = buildHostImage(b->desc);
  } catch (const std::invalid_argument& e) {
    std::printf("REFUSED by scene creation: %s\n", e.what());
    return 3;
  }
  const YartSceneDesc& d = b->desc;
  if (a->desc.n_materials != d.n_materials || a->desc.n_textures != d.n_textures || a->desc.n_meshes != d.n_meshes) {
    std::fprintf(stderr, "the scenes differ in their counts\n");
    return 2;
  }
  HostImage im = old;
  // ---- texels, and the materials' alpha flag from the words just written
  std::vector<uint8_t> flipped(d.n_materials, 0);
  uint32_t nFlipped = 0;
  for (uint32_t t = 0; t < d.n_textures; t++) {
    const TexDev& td = im.textures[t];
    if (td.isFloat) continue;
    const YartTextureDesc& nt = d.textures[t];
    if (nt.width != td.width || nt.height != td.height || nt.channels != td.channels || nt.is_float || tuIsClone(td)) {
      std::fprintf(stderr, "texture %u: a change the update refuses\n", t);
      return 2;
    }
    const size_t nTexels = size_t(td.width) * td.height, bytes = nTexels * td.channels;
    const bool changed = std::memcmp(nt.data, a->desc.textures[t].data, bytes) != 0;
    std::printf("texture %u changed %d places %zu\n", t, int(changed), tuPlaces(im.textures, t).size());
    if (!changed) continue;
    std::memcpy(im.texU8.data() + td.offset, nt.data, bytes);
    if (td.channels != 4u) continue;
    for (uint32_t m = 0; m < d.n_materials; m++) {
      if (d.materials[m].tex_base != int32_t(t)) continue;
      const bool now = tuAnyAlpha(im.texU8.data() + td.offset, nTexels), was = (im.materials[m].flags & MAT_HAS_ALPHA) != 0u;
      std::printf("material %u alpha %d was %d\n", m, int(now), int(was));
      if (now == was) continue;
      im.materials[m].flags = (im.materials[m].flags & ~uint32_t(MAT_HAS_ALPHA)) | (now ? uint32_t(MAT_HAS_ALPHA) : 0u);
      flipped[m] = 1; nFlipped++;
    }
  }
  std::printf("flipped %u\n", nFlipped);
  // ---- the chain, for the meshes with a face of a flipped material
  for (size_t mi = 0; mi < im.meshes.size(); mi++) {
    MeshDev& md = im.meshes[mi];
    bool affected = false;
    for (uint32_t f = 0; f < md.nTris; f++) affected |= flipped[im.triVerts[md.triOffset + f].w] != 0;
    if (affected) {
      LeafTri* leaves = im.leafTris.data() + md.leafOffset;
      BvhNode* nodes = im.bvhNodes.data() + md.nodeOffset;
      for (size_t k : scrambled(md.nTris, 1)) leaves[k].matFlags = tuLeafFlags(leaves[k].matFlags, im.materials[leaves[k].material].flags);   // k_tu_leaves
      std::vector<uint32_t> prefix(size_t(md.nTris) + 1u, 0u);                                                      // k_mu_alpha_scan
      for (uint32_t k = 0; k < md.nTris; k++) prefix[k + 1u] = prefix[k] + ((leaves[k].matFlags & MAT_HAS_ALPHA) ? 1u : 0u);
      for (size_t n : scrambled(md.nNodes, 2)) {                                                                    // k_tu_links
        uint32_t first = 0, end = 0;
        if (!tuNodeRange(nodes, md.nNodes, leaves, md.nTris, uint32_t(n), first, end)) { std::printf("mesh %zu node %zu: no range\n", mi, n); failures++; continue; }
        const bool alpha = prefix[end] != prefix[first];
        nodes[n].leftFirst = tuLinkWord(nodes[n].leftFirst, alpha);
        if (n == 0) md.hasAlpha = alpha ? 1u : 0u;
      }
    }
    uint32_t with = 0, maxSpan = 0;
    for (uint32_t n = 0; n < md.nNodes; n++) {
      with += (im.bvhNodes[md.nodeOffset + n].leftFirst & kLinkAlphaBit) ? 1u : 0u;
      maxSpan = std::max(maxSpan, im.bvhNodes[md.nodeOffset + n].span);
    }
    std::printf("mesh %zu nodes %u withBit %u withoutBit %u chain %d maxSpan %u\n", mi, md.nNodes, with, md.nNodes - with, int(affected), maxSpan);
  }
  same("texU8", im.texU8.data(), want.texU8.data(), want.texU8.size());
  same("materials", im.materials.data(), want.materials.data(), want.materials.size() * sizeof(MaterialDev));
  same("leaf records", im.leafTris.data(), want.leafTris.data(), want.leafTris.size() * sizeof(LeafTri));
  same("bvh nodes", im.bvhNodes.data(), want.bvhNodes.data(), want.bvhNodes.size() * sizeof(BvhNode));
  same("meshes", im.meshes.data(), want.meshes.data(), want.meshes.size() * sizeof(MeshDev));
  same("textures", im.textures.data(), want.textures.data(), want.textures.size() * sizeof(TexDev));
  if (im.texU8.size() != want.texU8.size() || im.leafTris.size() != want.leafTris.size() || im.bvhNodes.size() != want.bvhNodes.size()) failures++;
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
