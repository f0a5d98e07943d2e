// mesh_replace.hpp — the layout arithmetic of yart_hip_scene_replace_meshes: where host_scene.hpp::buildHostImage puts the records
// of every mesh when some meshes come with new triangle and vertex counts, and how the pools that are indexed by triangle, by
// vertex and by BVH node are repacked to get there. Stated here for the library and the host simulator (tests/meshreplacesim) alike:
// the library's host side and the simulator run mrLayout, mrSegments and mrResolve, the library's host image and the simulator
// mrRepackHost (mrRecord, mrAddDelta), the kernels mrFindSegment, mrCovers and mrShadeRecord — k_mr_repack restates the copy, the
// delta and the zero fill per 16-byte unit, and the GPU tests compare its pools with create's. buildHostImage keeps its own code,
// and the tests compare the two byte for byte.
//
//   mrLayout          create's four offsets of every mesh from the meshes' counts: triOffset, leafOffset and vertOffset are running
//                     sums; a mesh's nodeOffset is the running node count made odd by one zero pad record (the children pair of a
//                     node then lies in one 64-byte line); two zero records stand behind the last mesh
//   mrSegments        one table per pool family (MR_TRIS: shadeTris / triVerts / triLight, MR_LEAVES: leafTris, MR_VERTS: the four
//                     vertex arrays, MR_NODES: bvhNodes): per mesh the destination offset, the count, the source — the old pool at
//                     the old offset, or the staging arrays of listed mesh k — and what is added to LeafTri::triIdx, a scene-wide
//                     index: the distance the mesh's ShadeTri records move (staged records are derived with the new offset)
//   mrResolve         a table with its sources as pointers into one pool and its staging arrays
//   mrFindSegment     the segment a destination record lies in or behind: a binary search over the destination offsets
//   mrCovers          whether it lies in it
//   mrRecord          one destination record: copied with the delta added where the record has a triIdx, zero where no segment
//                     covers it (the pad records and the two tail records of bvhNodes)
//   mrRepackHost      mrRecord over a whole pool, out of place
//   mrShadeRecord     the ShadeTri of a face: normals, tangents and uvs of its three vertices, its material, no light, zero pads
#pragma once
#include <cstring>
#include <stdexcept>
#include <vector>

#include "scene_types.hpp"

namespace yart_hip {

enum MrFamily : int { MR_TRIS = 0, MR_LEAVES = 1, MR_VERTS = 2, MR_NODES = 3 };

// What a listed mesh brings: its counts (nNodes known once its tree is built) and its alpha flag
struct MrStaged { uint32_t nTris, nVerts, nNodes, hasAlpha; };

struct MrLayout {
  std::vector<MeshDev> meshes;
  uint32_t nTris = 0, nVerts = 0, nNodes = 0;              // the pools' logical sizes (nNodes: pads and the two tail records included)
};

// stageOf[mesh]: the index of the mesh in the list, -1 for a mesh that stays
inline MrLayout mrLayout(const std::vector<MeshDev>& old, const std::vector<int32_t>& stageOf, const std::vector<MrStaged>& staged) {
  MrLayout l;
  l.meshes = old;
  uint64_t tris = 0, verts = 0, nodes = 0;
  for (size_t mi = 0; mi < old.size(); mi++) {
    MeshDev& md = l.meshes[mi];
    if (stageOf[mi] >= 0) {
      const MrStaged& st = staged[size_t(stageOf[mi])];
      md.nTris = st.nTris; md.nVerts = st.nVerts; md.nNodes = st.nNodes; md.hasAlpha = st.hasAlpha;
    }
    if (nodes % 2u == 0u) nodes++;                         // (create: a zero record in front of a mesh whose base would be even)
    md.nodeOffset = uint32_t(nodes); md.leafOffset = uint32_t(tris); md.triOffset = uint32_t(tris); md.vertOffset = uint32_t(verts);
    tris += md.nTris; verts += md.nVerts; nodes += md.nNodes;
  }
  nodes += 2u;                                             // (create: two zero records behind the last mesh)
  if (tris >= (uint64_t(1) << 32) || verts >= (uint64_t(1) << 32) || nodes >= (uint64_t(1) << 32))
    throw std::invalid_argument("the scene's triangles, vertices or BVH nodes no longer fit 32-bit offsets");
  l.nTris = uint32_t(tris); l.nVerts = uint32_t(verts); l.nNodes = uint32_t(nodes);
  return l;
}

struct MrSegment {
  uint32_t dst, count;                                     // destination records [dst, dst + count)
  uint32_t src;                                            // stage < 0: the first record in the old pool; else 0 (a staging array starts at its mesh)
  int32_t stage;                                           // the listed mesh the records come from, -1: the old pool
  uint32_t delta;                                          // added to LeafTri::triIdx (modulo 2^32: a mesh that moves down has a "negative" one)
};

inline std::vector<MrSegment> mrSegments(const std::vector<MeshDev>& old, const std::vector<MeshDev>& now, const std::vector<int32_t>& stageOf,
                                         MrFamily family) {
  std::vector<MrSegment> segs(old.size());
  for (size_t mi = 0; mi < old.size(); mi++) {
    const MeshDev& o = old[mi]; const MeshDev& n = now[mi];
    MrSegment& s = segs[mi];
    s.stage = stageOf[mi];
    switch (family) {
      case MR_TRIS: s.dst = n.triOffset; s.count = n.nTris; s.src = o.triOffset; break;
      case MR_LEAVES: s.dst = n.leafOffset; s.count = n.nTris; s.src = o.leafOffset; break;
      case MR_VERTS: s.dst = n.vertOffset; s.count = n.nVerts; s.src = o.vertOffset; break;
      default: s.dst = n.nodeOffset; s.count = n.nNodes; s.src = o.nodeOffset; break;
    }
    s.delta = 0u;
    if (family == MR_LEAVES && s.stage < 0) s.delta = n.triOffset - o.triOffset;
    if (s.stage >= 0) s.src = 0u;
  }
  return segs;
}

// A segment as the repack reads it: the source resolved to a pointer (the host simulator's, or device memory for the kernels)
struct MrSource {
  const void* src;
  uint32_t dst, count, delta, pad;
};
template <class Record>
inline void mrResolve(const std::vector<MrSegment>& segs, const Record* oldPool, const std::vector<const Record*>& stagePools, std::vector<MrSource>& out) {
  for (const MrSegment& s : segs) {
    MrSource r;
    r.src = s.stage >= 0 ? stagePools[size_t(s.stage)] : oldPool + s.src;
    r.dst = s.dst; r.count = s.count; r.delta = s.delta; r.pad = 0u;
    out.push_back(r);
  }
}

// The last segment whose destination offset is not behind record i (the tables are in mesh order: dst ascends; n >= 1 and
// segs[0].dst <= 1); the record lies in it, or — bvhNodes only — in the gap behind it
YART_HD uint32_t mrFindSegment(const MrSource* segs, uint32_t n, uint32_t i) {
  uint32_t lo = 0u, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (segs[mid].dst <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// What is added to a record on its way: LeafTri alone carries an index into another pool
template <class Record> YART_HD void mrAddDelta(Record&, uint32_t) {}
template <> YART_HD void mrAddDelta<LeafTri>(LeafTri& lt, uint32_t delta) { lt.triIdx += delta; }

// Does the segment hold destination record i? (mrFindSegment's answer may lie in front of it: the pad records, the tail)
YART_HD bool mrCovers(const MrSource& s, uint32_t i) { return i >= s.dst && i - s.dst < s.count; }

// Destination record i of a pool; false: no segment covers it, the record is zero
template <class Record>
YART_HD bool mrRecord(const MrSource* segs, uint32_t n, uint32_t i, Record& out) {
  const MrSource& s = segs[mrFindSegment(segs, n, i)];
  if (!mrCovers(s, i)) return false;
  out = static_cast<const Record*>(s.src)[i - s.dst];
  mrAddDelta(out, s.delta);
  return true;
}

template <class Record>
inline void mrRepackHost(const std::vector<MrSource>& segs, uint32_t total, std::vector<Record>& out) {
  out.resize(total);
  for (uint32_t i = 0; i < total; i++)
    if (!mrRecord(segs.data(), uint32_t(segs.size()), i, out[i])) std::memset(static_cast<void*>(&out[i]), 0, sizeof(Record));
}

// create's ShadeTri of face tv (x, y, z: vertices, w: material) from the caller's packed arrays: 3 / 4 / 2 floats per vertex. A
// replaced mesh has no lights (yart_hip.h): light = -1.
YART_HD void mrShadeRecord(ShadeTri& st, const float* normals, const float* tangents, const float* uvs, u4 tv) {
  const uint32_t vi[3] = {tv.x, tv.y, tv.z};
  for (int k = 0; k < 3; k++) {
    for (int c = 0; c < 3; c++) st.n[k][c] = normals[3u * size_t(vi[k]) + c];
    for (int c = 0; c < 4; c++) st.t[k][c] = tangents[4u * size_t(vi[k]) + c];
    for (int c = 0; c < 2; c++) st.uv[k][c] = uvs[2u * size_t(vi[k]) + c];
  }
  st.material = tv.w; st.light = -1;
  st.pad[0] = st.pad[1] = st.pad[2] = 0u;
}

}  // namespace yart_hip
