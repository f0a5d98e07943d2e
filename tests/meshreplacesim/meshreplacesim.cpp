// meshreplacesim — csrc/mesh_replace.hpp on the host against host_scene.hpp::buildHostImage (tests/test_mesh_replace_host.py).
//
//   meshreplacesim OLD.yscn NEW.yscn
//
// OLD and NEW are two scenes with the same materials, nodes and mesh count; a mesh whose description differs between them — counts,
// vertex arrays or faces — is "listed", as a caller of yart_hip_scene_replace_meshes would list it. The program builds
// buildHostImage(NEW) — what a freshly created scene holds — and derives the same pools from buildHostImage(OLD) and the listed
// meshes of NEW by the statements the library runs: mrLayout, mrSegments, per listed mesh the host builder's tree through
// muDeriveHost (with the mesh's NEW triOffset) and mrShadeRecord, then mrRepackHost per pool — the triIdx delta, the zero pad
// records and the two tail records of bvhNodes included. Every pool, the MeshDev records, the stack bound, the vertex boxes and the
// re-derived node boxes are compared byte for byte. One line per mesh:
// `mesh I listed L tris N was M verts N was M nodes N was M base B was C delta D`, one line per comparison. Exit status 0: all equal.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/mesh_replace.hpp"
#include "../../yart_amd/csrc/mesh_update.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static int failures = 0;
static void same(const std::string& what, const void* a, const void* b, size_t n) {
  const bool ok = std::memcmp(a, b, n) == 0;
  std::printf("%s %s (%zu bytes)\n", ok ? "EQUAL" : "DIFFERENT", what.c_str(), n);
  if (!ok) failures++;
}
template <class T>
static void samePool(const std::string& what, const std::vector<T>& got, const std::vector<T>& want) {
  const size_t a = got.size(), b = want.size();
  same(what + " size", &a, &b, sizeof(size_t));
  if (a == b) same(what, got.data(), want.data(), a * sizeof(T));
}

static bool sameMesh(const YartMeshDesc& a, const YartMeshDesc& b) {
  if (a.n_vertices != b.n_vertices || a.n_faces != b.n_faces) return false;
  const size_t nv = a.n_vertices, nf = a.n_faces;
  return !std::memcmp(a.positions, b.positions, nv * 12) && !std::memcmp(a.normals, b.normals, nv * 12) && !std::memcmp(a.tangents, b.tangents, nv * 16) &&
         !std::memcmp(a.uvs, b.uvs, nv * 8) && !std::memcmp(a.faces, b.faces, nf * 16);
}

struct Staged {
  std::vector<BvhNode> nodes; std::vector<LeafTri> leaf; std::vector<ShadeTri> shade; std::vector<u4> faces; std::vector<int32_t> light;
  std::vector<f4> vPos, vNormal, vTangent; std::vector<f2> vUV;
  std::vector<uint32_t> indices;
  uint32_t need = 0;
};

template <class Record>
static std::vector<Record> repack(const std::vector<MrSegment>& segs, const std::vector<Record>& oldPool, const std::vector<Staged>& st,
                                  std::vector<Record> Staged::*member, uint32_t total) {
  std::vector<const Record*> pools;
  for (const Staged& s : st) pools.push_back((s.*member).data());
  std::vector<MrSource> src;
  mrResolve<Record>(segs, oldPool.data(), pools, src);
  std::vector<Record> out;
  mrRepackHost(src, total, out);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: meshreplacesim OLD.yscn NEW.yscn\n"); return 2; }
  auto a = loadSceneFile(argv[1]);
  auto b = loadSceneFile(argv[2]);
  if (a->desc.n_meshes != b->desc.n_meshes || a->desc.n_nodes != b->desc.n_nodes || a->desc.n_materials != b->desc.n_materials) {
    std::fprintf(stderr, "the scenes differ in their counts\n");
    return 2;
  }
  const HostImage old = buildHostImage(a->desc), want = buildHostImage(b->desc);
  const uint32_t nm = b->desc.n_meshes;
  std::vector<int32_t> stageOf(nm, -1);
  std::vector<MrStaged> counts;
  for (uint32_t mi = 0; mi < nm; mi++)
    if (!sameMesh(a->desc.meshes[mi], b->desc.meshes[mi])) {
      stageOf[mi] = int32_t(counts.size());
      counts.push_back(MrStaged{b->desc.meshes[mi].n_faces, b->desc.meshes[mi].n_vertices, 0u, 0u});
    }
  const MrLayout early = mrLayout(old.meshes, stageOf, counts);
  std::vector<uint32_t> flags;
  for (const MaterialDev& m : old.materials) flags.push_back(m.flags);
  std::vector<Staged> st(counts.size());
  HostImage im = old;
  for (uint32_t mi = 0; mi < nm; mi++) {
    if (stageOf[mi] < 0) continue;
    const YartMeshDesc& m = b->desc.meshes[mi];
    Staged& s = st[size_t(stageOf[mi])];
    const u4* faces = reinterpret_cast<const u4*>(m.faces);
    SahBvhBuilder hb;
    hb.setThreads(1);
    hb.build(m.positions, m.faces, 4, m.n_faces);
    s.nodes.resize(hb.nodes.size()); s.leaf.resize(m.n_faces);
    const MuDerived d = muDeriveHost(hb.nodes.data(), uint32_t(hb.nodes.size()), hb.indices.data(), m.n_faces, m.positions, faces,
                                     early.meshes[mi].triOffset, flags.data(), s.nodes.data(), s.leaf.data());
    s.indices = hb.indices; s.need = d.stackNeed;
    s.faces.assign(faces, faces + m.n_faces);
    s.light.assign(m.n_faces, -1);
    s.shade.resize(m.n_faces);
    for (uint32_t f = 0; f < m.n_faces; f++) {
      std::memset(static_cast<void*>(&s.shade[f]), 0xa5, sizeof(ShadeTri));       // (the record is written whole: no byte of this survives)
      mrShadeRecord(s.shade[f], m.normals, m.tangents, m.uvs, faces[f]);
    }
    for (uint32_t v = 0; v < m.n_vertices; v++) {
      f4 p; p.x = m.positions[3 * v]; p.y = m.positions[3 * v + 1]; p.z = m.positions[3 * v + 2]; p.w = 0;
      f4 n; n.x = m.normals[3 * v]; n.y = m.normals[3 * v + 1]; n.z = m.normals[3 * v + 2]; n.w = 0;
      f4 t; t.x = m.tangents[4 * v]; t.y = m.tangents[4 * v + 1]; t.z = m.tangents[4 * v + 2]; t.w = m.tangents[4 * v + 3];
      s.vPos.push_back(p); s.vNormal.push_back(n); s.vTangent.push_back(t); s.vUV.push_back(mk2(m.uvs[2 * v], m.uvs[2 * v + 1]));
    }
    counts[size_t(stageOf[mi])].nNodes = uint32_t(s.nodes.size());
    counts[size_t(stageOf[mi])].hasAlpha = d.hasAlpha;
    im.meshStackNeed[mi] = d.stackNeed;
    im.meshBox[mi] = muVertexBox(m.positions, m.n_vertices);
    const std::string t = "mesh " + std::to_string(mi) + " ";
    same(t + "stack need", &d.stackNeed, &want.meshStackNeed[mi], 4);
    same(t + "vertex box", &im.meshBox[mi], &want.meshBox[mi], sizeof(SuBox));
    same(t + "indices", s.indices.data(), want.bvhIndices[mi].data(), size_t(m.n_faces) * 4);
  }
  const MrLayout now = mrLayout(old.meshes, stageOf, counts);
  std::printf("meshes %u listed %zu stackBound %u was %u\n", nm, counts.size(), want.stackBound, old.stackBound);
  for (uint32_t mi = 0; mi < nm; mi++) {
    const MeshDev& o = old.meshes[mi]; const MeshDev& n = now.meshes[mi];
    std::printf("mesh %u listed %d tris %u was %u verts %u was %u nodes %u was %u base %u was %u delta %d\n", mi, int(stageOf[mi] >= 0), n.nTris, o.nTris,
                n.nVerts, o.nVerts, n.nNodes, o.nNodes, n.nodeOffset, o.nodeOffset, int32_t(n.triOffset - o.triOffset));
  }
  samePool("meshes", now.meshes, want.meshes);
  const std::vector<MrSegment> segTris = mrSegments(old.meshes, now.meshes, stageOf, MR_TRIS), segLeaves = mrSegments(old.meshes, now.meshes, stageOf, MR_LEAVES),
                               segVerts = mrSegments(old.meshes, now.meshes, stageOf, MR_VERTS), segNodes = mrSegments(old.meshes, now.meshes, stageOf, MR_NODES);
  samePool("shadeTris", repack(segTris, old.shadeTris, st, &Staged::shade, now.nTris), want.shadeTris);
  samePool("leafTris", repack(segLeaves, old.leafTris, st, &Staged::leaf, now.nTris), want.leafTris);
  samePool("triVerts", repack(segTris, old.triVerts, st, &Staged::faces, now.nTris), want.triVerts);
  samePool("triLight", repack(segTris, old.triLight, st, &Staged::light, now.nTris), want.triLight);
  samePool("vPos", repack(segVerts, old.vPos, st, &Staged::vPos, now.nVerts), want.vPos);
  samePool("vNormal", repack(segVerts, old.vNormal, st, &Staged::vNormal, now.nVerts), want.vNormal);
  samePool("vTangent", repack(segVerts, old.vTangent, st, &Staged::vTangent, now.nVerts), want.vTangent);
  samePool("vUV", repack(segVerts, old.vUV, st, &Staged::vUV, now.nVerts), want.vUV);
  samePool("bvhNodes", repack(segNodes, old.bvhNodes, st, &Staged::nodes, now.nNodes), want.bvhNodes);
  uint32_t bound = im.tlasHeight;
  for (uint32_t need : im.meshStackNeed) bound = std::max(bound, need);
  same("stack bound", &bound, &want.stackBound, 4);
  {
    const uint32_t nn = uint32_t(im.nodes.size());
    std::vector<uint32_t> nf(nn);
    (void)suIdentityFlags(b->desc.nodes, nn, nf.data());
    std::vector<SuFold> scratch(nn);
    suRederiveHost(im.nodes.data(), im.nodeWorld.data(), nn, b->desc.nodes, nf.data(), im.meshBox.data(), scratch.data());
    same("nodes", im.nodes.data(), want.nodes.data(), want.nodes.size() * sizeof(NodeDev));
    same("nodeWorld", im.nodeWorld.data(), want.nodeWorld.data(), want.nodeWorld.size() * sizeof(f4));
  }
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
