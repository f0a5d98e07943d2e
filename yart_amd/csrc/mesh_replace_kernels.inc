// mesh_replace_kernels.inc — yart_hip_scene_replace_meshes: whole new meshes, with triangle and vertex counts of their own, for a
// scene that is on the device (included by yart_hip.hip, unit 0, behind mesh_update_kernels.inc: the entry stages its meshes
// through muStageCore and ends in muRederiveScene). The layout and the segment tables are csrc/mesh_replace.hpp's. Per listed mesh:
//
//   (copies)         the caller's positions / normals / tangents / uvs / faces into the mesh's staging arrays
//   muStageCore      the BVH build over the staged positions and faces, the LeafTri records with the mesh's NEW triOffset, the alpha
//                    scan, the link words (mesh_update_kernels.inc)
//   k_mr_shade       the ShadeTri records of the faces: normals, tangents and uvs of the three vertices, material, light -1
//   k_mr_verts       the vPos / vNormal / vTangent / vUV entries
//   (memset)         the triLight entries: -1
//
// and only once every listed mesh has built and is no deeper than kMaxStackBound, the scene is touched. If a listed mesh changes its
// triangle, vertex or node count:
//
//   k_mr_repack<R>   one launch per pool — shadeTris, leafTris, triVerts, triLight, vPos, vNormal, vTangent, vUV, bvhNodes —, out of
//                    place into the pool's second array (a shrinking mesh makes source and destination ranges overlap forwards): a
//                    workgroup owns kMrChunk consecutive 16-byte words of the destination (whole records for the 4-byte triLight
//                    and the 8-byte vUV), finds the segment of its first record by binary search over the destination offsets and
//                    walks on from there; LeafTri records get their segment's triIdx delta, bvhNodes records outside every segment
//                    (the pads, the two tail records) are zero. Then the two arrays of each pool are swapped. Of the header the
//                    kernel runs mrFindSegment and mrCovers on the tables mrSegments / mrResolve made; the copy, the delta and the
//                    zero fill are restated per 16-byte unit here (the header's mrRecord / mrAddDelta state them per record for the
//                    host image and the simulator), and it is the GPU tests that hold the two together, pool by pool on bytes.
//
// otherwise the staged records are copied into place and nothing else moves. Then muRederiveScene: the MeshDev records, the stack
// bound, and the scene-update chain with the scene's current transforms over the new vertex boxes.
namespace {

struct MrShadeArgs { const float *nrm, *tan, *uv; const u4* faces; ShadeTri* shade; uint32_t n, nVerts; };
__global__ void __launch_bounds__(kBlock) k_mr_shade(MrShadeArgs a) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n) return;
  const u4 tv = a.faces[f];
  if (tv.x >= a.nVerts || tv.y >= a.nVerts || tv.z >= a.nVerts) return;   // (the entry checked the faces: cannot happen)
  ShadeTri st;
  mrShadeRecord(st, a.nrm, a.tan, a.uv, tv);
  a.shade[f] = st;
}

struct MrVertArgs { const float *pos, *nrm, *tan, *uv; f4 *vPos, *vNormal, *vTangent; f2* vUV; uint32_t n; };
__global__ void __launch_bounds__(kBlock) k_mr_verts(MrVertArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  f4 p; p.x = a.pos[3u * size_t(i)]; p.y = a.pos[3u * size_t(i) + 1u]; p.z = a.pos[3u * size_t(i) + 2u]; p.w = 0.0f;
  f4 n; n.x = a.nrm[3u * size_t(i)]; n.y = a.nrm[3u * size_t(i) + 1u]; n.z = a.nrm[3u * size_t(i) + 2u]; n.w = 0.0f;
  f4 t; t.x = a.tan[4u * size_t(i)]; t.y = a.tan[4u * size_t(i) + 1u]; t.z = a.tan[4u * size_t(i) + 2u]; t.w = a.tan[4u * size_t(i) + 3u];
  a.vPos[i] = p; a.vNormal[i] = n; a.vTangent[i] = t;
  a.vUV[i] = mk2(a.uv[2u * size_t(i)], a.uv[2u * size_t(i) + 1u]);
}

// The unit a lane moves: 16 bytes where the record is a multiple of that, the record itself otherwise (triLight, vUV)
constexpr uint32_t kMrChunk = 1024;                          // units of the destination per workgroup: 4 per lane
template <class Record> struct MrUnit {
  static constexpr bool wide = sizeof(Record) % 16u == 0u;
  using T = std::conditional_t<wide, uint4, Record>;
  static constexpr uint32_t perRecord = uint32_t(sizeof(Record) / sizeof(T));
};
static_assert(offsetof(LeafTri, triIdx) == 12, "k_mr_repack adds the delta to the fourth word of a LeafTri's first 16 bytes");

template <class Record>
__global__ void __launch_bounds__(kBlock) k_mr_repack(const MrSource* segs, uint32_t nSegs, Record* out, uint32_t total) {
  using Unit = typename MrUnit<Record>::T;
  constexpr uint32_t per = MrUnit<Record>::perRecord;
  const uint64_t first = uint64_t(blockIdx.x) * kMrChunk, all = uint64_t(total) * per;
  const uint64_t end = first + kMrChunk < all ? first + kMrChunk : all;
  if (first >= end) return;
  const uint32_t sFirst = mrFindSegment(segs, nSegs, uint32_t(first / per));
  Unit* dst = reinterpret_cast<Unit*>(out);
  for (uint64_t e = first + threadIdx.x; e < end; e += kBlock) {
    const uint32_t r = uint32_t(e / per), q = uint32_t(e % per);
    uint32_t si = sFirst;
    while (si + 1u < nSegs && segs[si + 1u].dst <= r) si++;  // (a chunk spans few meshes)
    const MrSource s = segs[si];
    const bool covered = mrCovers(s, r);
    const Unit v = covered ? static_cast<const Unit*>(s.src)[uint64_t(r - s.dst) * per + q] : Unit{};
    // (the patched unit is built as a new value: a write to v.w made the compiler split the load and keep three words per lane in LDS)
    if constexpr (std::is_same_v<Record, LeafTri>) dst[e] = make_uint4(v.x, v.y, v.z, v.w + (covered && q == 0u ? s.delta : 0u));
    else dst[e] = v;
  }
}

constexpr UpdateCheck mrCheck{"scene_replace_meshes: "};

void mrValidateArguments(const YartSceneMeshReplace& u) {
  mrCheck(u.meshes != nullptr, "meshes pointer is null");
  checkUpdateFlags(mrCheck, u.flags);
  mrCheck(u.n_meshes >= 1u, "n_meshes is 0");
}

// ... and what compares the update with the scene; boxes: the vertex box of every listed mesh
void mrValidateAgainstScene(const YartScene& scene, const YartSceneMeshReplace& u, std::vector<SuBox>& boxes) {
  const HostImage& h = scene.host;
  mrCheck(u.n_meshes <= h.meshes.size(), "n_meshes is " + std::to_string(u.n_meshes) + ", the scene has " + std::to_string(h.meshes.size()) + " meshes");
  std::vector<uint8_t> listed(h.meshes.size(), 0);
  for (uint32_t k = 0; k < u.n_meshes; k++) {                // the counts and the pointers of every entry, before an array is read
    const YartMeshReplace& m = u.meshes[k];
    const YartMeshDesc& d = m.desc;
    const std::string name = "mesh " + std::to_string(m.mesh);
    mrCheck(m.mesh < h.meshes.size(), name + ": index out of range");
    mrCheck(!listed[m.mesh], name + " is listed twice");
    listed[m.mesh] = 1;
    mrCheck(d.n_faces > 0u, name + ": n_faces is 0");
    mrCheck(d.n_faces < (1u << 25), name + ": 2^25 triangles and more per mesh are not supported");
    mrCheck(d.n_vertices > 0u, name + ": n_vertices is 0");
    mrCheck(d.positions && d.normals && d.tangents && d.uvs && d.faces, name + ": positions, normals, tangents, uvs or faces pointer is null");
  }
  boxes.resize(u.n_meshes);
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const YartMeshReplace& m = u.meshes[k];
    const YartMeshDesc& d = m.desc;
    const std::string name = "mesh " + std::to_string(m.mesh);
    for (uint32_t f = 0; f < d.n_faces; f++) {               // (the messages are built for a face that fails only)
      const uint32_t* w = d.faces + 4u * size_t(f);
      if (w[0] >= d.n_vertices || w[1] >= d.n_vertices || w[2] >= d.n_vertices) mrCheck(false, name + ": face " + std::to_string(f) + ": vertex index out of range");
      if (w[3] >= h.nMaterials) mrCheck(false, name + ": face " + std::to_string(f) + ": material index out of range");
    }
    const size_t nv = d.n_vertices;
    mrCheck(finiteWords(d.positions, nv * 3u), name + ": a position word is not finite");
    mrCheck(finiteWords(d.normals, nv * 3u), name + ": a normal word is not finite");
    mrCheck(finiteWords(d.tangents, nv * 4u), name + ": a tangent word is not finite");
    mrCheck(finiteWords(d.uvs, nv * 2u), name + ": a uv word is not finite");
    boxes[k] = muVertexBox(d.positions, d.n_vertices);
  }
  checkMeshBoxes(mrCheck, h, listed.data());
  // emissive meshes change the light list, which no entry does: neither the mesh as it is nor the mesh as given may have a light
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const YartMeshReplace& m = u.meshes[k];
    const std::string name = "mesh " + std::to_string(m.mesh);
    bool named = false, had = false, has = false;
    for (uint32_t i = 0; i < h.nLights; i++) named |= h.lights[i].type == LIGHT_AREA && h.lights[i].mesh == int32_t(m.mesh);
    mrCheck(!named, name + ": a light of the scene is on this mesh (an emissive mesh is re-created, not replaced)");
    const MeshDev& md = h.meshes[m.mesh];
    for (uint32_t f = 0; f < md.nTris; f++) had |= h.triLight[md.triOffset + f] != -1;
    mrCheck(!had, name + ": the mesh has a face_light entry (an emissive mesh is re-created, not replaced)");
    if (m.desc.face_light)
      for (uint32_t f = 0; f < m.desc.n_faces; f++) has |= m.desc.face_light[f] != -1;
    mrCheck(!has, name + ": face_light has an entry other than -1");
  }
}

// One pool into its second array (sized by the caller), and the two swapped; view: the pool's pointer in SceneDev
template <class Record>
void mrRepackPool(DevBuf<Record>& pool, DevBuf<Record>& alt, const Record*& view, const MrSource* segs, uint32_t nSegs, uint32_t total, UpdateCall& call) {
  const uint64_t units = uint64_t(total) * MrUnit<Record>::perRecord;
  hipLaunchKernelGGL(k_mr_repack<Record>, dim3(uint32_t((units + kMrChunk - 1u) / kMrChunk)), dim3(kBlock), 0, call.stream, segs, nSegs, alt.p, total);
  call.launched();
  std::swap(pool.p, alt.p); std::swap(pool.n, alt.n);
  view = pool.p;
}
// A pool's segment table with its sources as device pointers: the pool itself and the staging arrays `member` of the listed meshes
template <class Record, class Member>
void mrResolvePool(const std::vector<MrSegment>& segs, const Record* oldPool, const std::vector<std::unique_ptr<MeshStage>>& stages, uint32_t nStages,
                   Member member, std::vector<MrSource>& table) {
  std::vector<const Record*> pools;
  for (uint32_t k = 0; k < nStages; k++) pools.push_back(((*stages[k]).*member).p);
  mrResolve<Record>(segs, oldPool, pools, table);
}
// A second array that holds `total` records: grown by half beyond that when it is too small
template <class Record> void mrEnsure(DevBuf<Record>& alt, size_t total) {
  if (alt.n < total) alt.ensure(total + total / 2u);
}

void mrUpdate(YartScene& s, const YartSceneMeshReplace& u, const std::vector<SuBox>& boxes, hipStream_t stream, YartSceneUpdateStats* stats) {
  std::vector<YartNodeDesc> nodes;                           // (copies read the three: before the frame)
  std::vector<uint32_t> flags;
  std::vector<MrSource> table;
  UpdateCall call(WallClock::now(), s.device, stream);
  HostImage& h = s.host;
  MeshUpdateState& mu = s.meshUp;
  const uint32_t nm = uint32_t(h.meshes.size());
  std::vector<int32_t> stageOf(nm, -1);
  std::vector<MrStaged> staged(u.n_meshes);
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    stageOf[u.meshes[k].mesh] = int32_t(k);
    staged[k] = MrStaged{u.meshes[k].desc.n_faces, u.meshes[k].desc.n_vertices, 0u, 0u};
  }
  // (the triangle offsets do not depend on the node counts: known before a tree is built, and the leaf records are derived with them)
  const MrLayout early = mrLayout(h.meshes, stageOf, staged);
  while (mu.stages.size() < u.n_meshes) mu.stages.push_back(std::make_unique<MeshStage>());
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const YartMeshReplace& m = u.meshes[k];
    const YartMeshDesc& d = m.desc;
    MeshStage& st = *mu.stages[k];
    const uint32_t nv = d.n_vertices, nt = d.n_faces;
    st.faces.ensure(nt); st.uv.ensure(size_t(nv) * 2u);
    st.light.ensure(nt); st.shade.ensure(nt);
    st.vPos.ensure(nv); st.vNormal.ensure(nv); st.vTangent.ensure(nv); st.vUV.ensure(nv);
    HIP_CHECK(hipMemcpyAsync(st.faces.p, d.faces, size_t(nt) * 16u, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(st.uv.p, d.uvs, size_t(nv) * 8u, hipMemcpyHostToDevice, stream));
    bool alpha = false;                                      // does a new face have an alpha-tested material?
    for (uint32_t f = 0; f < nt && !alpha; f++) alpha = (h.materials[d.faces[4u * size_t(f) + 3u]].flags & MAT_HAS_ALPHA) != 0u;
    const MuStageIn in{m.mesh, nv, nt, early.meshes[m.mesh].triOffset, d.positions, d.normals, d.tangents, reinterpret_cast<const u4*>(d.faces),
                       st.faces.p, alpha};
    muStageCore(s, in, st, call, mrCheck);
    MrShadeArgs sa{st.nrm.p, st.tan.p, st.uv.p, st.faces.p, st.shade.p, nt, nv};
    hipLaunchKernelGGL(k_mr_shade, dim3((nt + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, sa);
    call.launched();
    MrVertArgs va{st.pos.p, st.nrm.p, st.tan.p, st.uv.p, st.vPos.p, st.vNormal.p, st.vTangent.p, st.vUV.p, nv};
    hipLaunchKernelGGL(k_mr_verts, dim3((nv + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, va);
    call.launched();
    HIP_CHECK(hipMemsetAsync(st.light.p, 0xff, size_t(nt) * 4u, stream));   // (-1)
    staged[k].nNodes = st.nNodes; staged[k].hasAlpha = st.hasAlpha;
  }
  const MrLayout now = mrLayout(h.meshes, stageOf, staged);
  bool repack = false;
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const MeshDev& o = h.meshes[u.meshes[k].mesh];
    repack |= o.nTris != staged[k].nTris || o.nVerts != staged[k].nVerts || o.nNodes != staged[k].nNodes;
  }
  const std::vector<MrSegment> segTris = mrSegments(h.meshes, now.meshes, stageOf, MR_TRIS), segLeaves = mrSegments(h.meshes, now.meshes, stageOf, MR_LEAVES),
                               segVerts = mrSegments(h.meshes, now.meshes, stageOf, MR_VERTS), segNodes = mrSegments(h.meshes, now.meshes, stageOf, MR_NODES);
  if (repack) {
    // every allocation first: nothing of the scene is written before the last of them has succeeded
    MeshReplacePools& alt = mu.alt;
    mrEnsure(alt.shadeTris, now.nTris); mrEnsure(alt.leafTris, now.nTris); mrEnsure(alt.triVerts, now.nTris); mrEnsure(alt.triLight, now.nTris);
    mrEnsure(alt.vPos, now.nVerts); mrEnsure(alt.vNormal, now.nVerts); mrEnsure(alt.vTangent, now.nVerts); mrEnsure(alt.vUV, now.nVerts);
    mrEnsure(mu.nodesAlt, now.nNodes);
    alt.segments.ensure(size_t(nm) * 9u);
    auto resolve = [&](const std::vector<MrSegment>& segs, const auto* oldPool, auto member) { mrResolvePool(segs, oldPool, mu.stages, u.n_meshes, member, table); };
    resolve(segTris, s.shadeTris.p, &MeshStage::shade); resolve(segLeaves, s.leafTris.p, &MeshStage::leaf);
    resolve(segTris, s.triVerts.p, &MeshStage::faces); resolve(segTris, s.triLight.p, &MeshStage::light);
    resolve(segVerts, s.vPos.p, &MeshStage::vPos); resolve(segVerts, s.vNormal.p, &MeshStage::vNormal);
    resolve(segVerts, s.vTangent.p, &MeshStage::vTangent); resolve(segVerts, s.vUV.p, &MeshStage::vUV);
    resolve(segNodes, s.bvhNodes.p, &MeshStage::nodes);
    // (the table buffer is the scene's, not the stream's: the next call may overwrite it because every entry returns synchronised — call.close())
    HIP_CHECK(hipMemcpyAsync(alt.segments.p, table.data(), table.size() * sizeof(MrSource), hipMemcpyHostToDevice, stream));
    const MrSource* seg = alt.segments.p;
    // ---- from here on the scene is written
    mrRepackPool(s.shadeTris, alt.shadeTris, s.dev.shadeTris, seg, nm, now.nTris, call);
    mrRepackPool(s.leafTris, alt.leafTris, s.dev.leafTris, seg + nm, nm, now.nTris, call);
    mrRepackPool(s.triVerts, alt.triVerts, s.dev.triVerts, seg + 2u * nm, nm, now.nTris, call);
    mrRepackPool(s.triLight, alt.triLight, s.dev.triLight, seg + 3u * nm, nm, now.nTris, call);
    mrRepackPool(s.vPos, alt.vPos, s.dev.vPos, seg + 4u * nm, nm, now.nVerts, call);
    mrRepackPool(s.vNormal, alt.vNormal, s.dev.vNormal, seg + 5u * nm, nm, now.nVerts, call);
    mrRepackPool(s.vTangent, alt.vTangent, s.dev.vTangent, seg + 6u * nm, nm, now.nVerts, call);
    mrRepackPool(s.vUV, alt.vUV, s.dev.vUV, seg + 7u * nm, nm, now.nVerts, call);
    mrRepackPool(s.bvhNodes, mu.nodesAlt, s.dev.bvhNodes, seg + 8u * nm, nm, now.nNodes, call);
  } else {
    // no count changed, so no record of another mesh moves: the staged records into place
    for (uint32_t k = 0; k < u.n_meshes; k++) {
      const MeshStage& st = *mu.stages[k];
      const MeshDev& md = now.meshes[u.meshes[k].mesh];
      auto place = [&](auto* to, const auto* from, size_t n) { HIP_CHECK(hipMemcpyAsync(to, from, n * sizeof(*to), hipMemcpyDeviceToDevice, stream)); };
      place(s.bvhNodes.p + md.nodeOffset, st.nodes.p, md.nNodes);
      place(s.leafTris.p + md.leafOffset, st.leaf.p, md.nTris);
      place(s.shadeTris.p + md.triOffset, st.shade.p, md.nTris);
      place(s.triVerts.p + md.triOffset, st.faces.p, md.nTris);
      place(s.triLight.p + md.triOffset, st.light.p, md.nTris);
      place(s.vPos.p + md.vertOffset, st.vPos.p, md.nVerts);
      place(s.vNormal.p + md.vertOffset, st.vNormal.p, md.nVerts);
      place(s.vTangent.p + md.vertOffset, st.vTangent.p, md.nVerts);
      place(s.vUV.p + md.vertOffset, st.vUV.p, md.nVerts);
    }
  }
  // the host image: what the library reads after create — the faces (the next update_meshes builds over them, update_textures lists
  // their materials, the lights' triangles), triLight, the positions, and per mesh the record, permutation, stack need and vertex box
  {
    std::vector<std::vector<u4>> faces(u.n_meshes);
    std::vector<std::vector<int32_t>> light(u.n_meshes);
    std::vector<std::vector<f4>> pos(u.n_meshes);
    std::vector<const u4*> facePools; std::vector<const int32_t*> lightPools; std::vector<const f4*> posPools;
    for (uint32_t k = 0; k < u.n_meshes; k++) {
      const YartMeshDesc& d = u.meshes[k].desc;
      faces[k].assign(reinterpret_cast<const u4*>(d.faces), reinterpret_cast<const u4*>(d.faces) + d.n_faces);
      light[k].assign(d.n_faces, -1);
      pos[k].resize(d.n_vertices);
      for (uint32_t v = 0; v < d.n_vertices; v++) {
        f4& p = pos[k][v];
        p.x = d.positions[3u * size_t(v)]; p.y = d.positions[3u * size_t(v) + 1u]; p.z = d.positions[3u * size_t(v) + 2u]; p.w = 0.0f;
      }
      facePools.push_back(faces[k].data()); lightPools.push_back(light[k].data()); posPools.push_back(pos[k].data());
    }
    std::vector<MrSource> src;
    std::vector<u4> triVerts; std::vector<int32_t> triLight; std::vector<f4> vPos;
    mrResolve<u4>(segTris, h.triVerts.data(), facePools, src); mrRepackHost(src, now.nTris, triVerts); src.clear();
    mrResolve<int32_t>(segTris, h.triLight.data(), lightPools, src); mrRepackHost(src, now.nTris, triLight); src.clear();
    mrResolve<f4>(segVerts, h.vPos.data(), posPools, src); mrRepackHost(src, now.nVerts, vPos);
    h.triVerts.swap(triVerts); h.triLight.swap(triLight); h.vPos.swap(vPos);
  }
  h.meshes = now.meshes;
  std::vector<uint32_t> listed;
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const uint32_t mesh = u.meshes[k].mesh;
    MeshStage& st = *mu.stages[k];
    h.meshStackNeed[mesh] = st.need;
    h.meshBox[mesh] = boxes[k];
    h.bvhIndices[mesh] = st.idxHost;
    listed.push_back(mesh);
    // what was remembered about the mesh's faces, and the kept frame (its vertex array is indexed by scene-wide vertex)
    if (mesh < mu.meshAlpha.size()) mu.meshAlpha[mesh] = int8_t(-1);
  }
  s.texUp.meshMaterials.clear();
  s.havePrevious = false;
  muRederiveScene(s, listed, u.flags, nodes, flags, call);
  call.finish(stats);
}

}  // namespace

extern "C" {

int yart_hip_scene_replace_meshes(YartScene* scene, const YartSceneMeshReplace* update, void* stream, YartSceneUpdateStats* stats) {
  std::vector<SuBox> boxes;                                  // (the listed meshes' vertex boxes: from the checks to the run)
  return updateEntry(
      mrCheck, "YartSceneMeshReplace", scene, update, stream, stats,
      [&](const YartSceneMeshReplace& u) { mrValidateArguments(u); checkDeviceRebuildHandle(mrCheck, u.flags, scene); },
      [&](const YartScene& s, const YartSceneMeshReplace& u) { mrValidateAgainstScene(s, u, boxes); },
      [&](YartScene& s, const YartSceneMeshReplace& u, hipStream_t st, YartSceneUpdateStats* out) { mrUpdate(s, u, boxes, st, out); });
}

int yart_hip_probe_geometry(YartScene* scene, YartGeometryProbe* p) {
  return guarded([&] {
    require(scene, "probe_geometry: scene pointer is null");
    require(p && p->struct_size >= sizeof(YartGeometryProbe), "probe_geometry: probe pointer is null or its struct_size too small");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    const HostImage& h = s.host;
    HIP_CHECK(hipSetDevice(s.device));
    // the sizes from the layout: behind the last mesh the pools end (bvhNodes: two records later)
    size_t tris = 0, verts = 0, nodes = 0;
    if (!h.meshes.empty()) {
      const MeshDev& last = h.meshes.back();
      tris = size_t(last.triOffset) + last.nTris; verts = size_t(last.vertOffset) + last.nVerts; nodes = size_t(last.nodeOffset) + last.nNodes;
    }
    nodes += 2u;
    p->stack_bound = h.stackBound;
    p->n_bvh_nodes = nodes; p->n_leaf_tris = p->n_shade_tris = p->n_tri_verts = p->n_tri_light = tris;
    p->n_vpos = p->n_vnormal = p->n_vtangent = p->n_vuv = verts; p->n_meshes = h.meshes.size();
    auto copy = [&](void* out, const void* dev, size_t bytes) { if (out && bytes) HIP_CHECK(hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost)); };
    copy(p->bvh_nodes, s.bvhNodes.p, nodes * sizeof(BvhNode));
    copy(p->leaf_tris, s.leafTris.p, tris * sizeof(LeafTri));
    copy(p->shade_tris, s.shadeTris.p, tris * sizeof(ShadeTri));
    copy(p->tri_verts, s.triVerts.p, tris * sizeof(u4));
    copy(p->tri_light, s.triLight.p, tris * 4u);
    copy(p->vpos, s.vPos.p, verts * sizeof(f4));
    copy(p->vnormal, s.vNormal.p, verts * sizeof(f4));
    copy(p->vtangent, s.vTangent.p, verts * sizeof(f4));
    copy(p->vuv, s.vUV.p, verts * sizeof(f2));
    copy(p->meshes, s.meshes.p, h.meshes.size() * sizeof(MeshDev));
  });
}

}  // extern "C"
