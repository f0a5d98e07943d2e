// mesh_update_kernels.inc — yart_hip_scene_update_meshes: new vertices for meshes of a scene that is on the device, and the kernels
// that re-derive what buildHostImage derives from a mesh's vertices and its BVH (included by yart_hip.hip, unit 0, behind
// scene_update_kernels.inc: the entry ends in suRun). The arithmetic is csrc/mesh_update.hpp's; per listed mesh:
//
//   (copies)         the caller's positions / normals / tangents into the mesh's staging arrays, packed as the caller has them
//   devbvh::buildCore  the reference's binned-SAH build over the staged positions and the scene's own faces (triVerts + triOffset),
//                    node array and permutation into the mesh's staging arrays
//   k_mu_leaves      the LeafTri records through the permutation
//   k_mu_alpha_scan  (meshes with an alpha-tested material only) prefix sum of the records' MAT_HAS_ALPHA over the leaf order
//   k_mu_links       one lane per build node: the link word (alpha bit from the prefix sum over the node's index range, saturated
//                    span) into the emitted node, the long-span word into a leaf's first record, the leaf's depth (a walk up the
//                    parent links) into the mesh's stack need, the root's alpha flag
//
// and only once every listed mesh has built and is no deeper than kMaxStackBound, the scene is touched:
//
//   (copies)         staged nodes and leaf records into bvhNodes / leafTris — bvhNodes repacked as create packs it (odd bases, two
//                    zero records behind the last mesh) into a second array when a node count changed, and the two arrays swapped
//   k_mu_verts       vPos / vNormal / vTangent entries from the staged arrays
//   k_mu_shade       (normals or tangents given) the ShadeTri normals / tangents of the mesh's faces
//   suRun            the scene-update chain with the scene's current transforms over the new vertex boxes
//
// The staging (muStageCore) and what follows the meshes' own records (muRederiveScene: MeshDev records, stack bound, suRun) are
// yart_hip_scene_replace_meshes' too (mesh_replace_kernels.inc), which brings faces and counts of its own.
//
// A mesh the device build refuses (more than devbvh::kMaxLevels levels) — and every mesh under the environment variable
// YART_HOST_BVH, as at scene creation — is built and derived on the host (muDeriveHost) and uploaded into the same staging arrays.
namespace {

struct MuVertArgs { const float *pos, *nrm, *tan; f4 *vPos, *vNormal, *vTangent; uint32_t n; };   // (the f4 arrays start at the mesh's vertOffset)
__global__ void __launch_bounds__(kBlock) k_mu_verts(MuVertArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  f4 p; p.x = a.pos[3u * size_t(i)]; p.y = a.pos[3u * size_t(i) + 1u]; p.z = a.pos[3u * size_t(i) + 2u]; p.w = 0.0f;
  a.vPos[i] = p;
  if (a.nrm) { f4 n; n.x = a.nrm[3u * size_t(i)]; n.y = a.nrm[3u * size_t(i) + 1u]; n.z = a.nrm[3u * size_t(i) + 2u]; n.w = 0.0f; a.vNormal[i] = n; }
  if (a.tan) { f4 t; t.x = a.tan[4u * size_t(i)]; t.y = a.tan[4u * size_t(i) + 1u]; t.z = a.tan[4u * size_t(i) + 2u]; t.w = a.tan[4u * size_t(i) + 3u]; a.vTangent[i] = t; }
}

struct MuShadeArgs { const float *nrm, *tan; const u4* triVerts; ShadeTri* shade; uint32_t n, nVerts; };   // (triVerts / shade start at the mesh's triOffset)
__global__ void __launch_bounds__(kBlock) k_mu_shade(MuShadeArgs a) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n) return;
  const u4 tv = a.triVerts[f];
  const uint32_t vi[3] = {tv.x, tv.y, tv.z};
  ShadeTri& st = a.shade[f];
  for (int k = 0; k < 3; k++) {
    if (vi[k] >= a.nVerts) continue;                       // (create checked the faces: cannot happen)
    if (a.nrm) for (int c = 0; c < 3; c++) st.n[k][c] = a.nrm[3u * size_t(vi[k]) + c];
    if (a.tan) for (int c = 0; c < 4; c++) st.t[k][c] = a.tan[4u * size_t(vi[k]) + c];
  }
}

struct MuLeafArgs { const float* pos; const u4* triVerts; const MaterialDev* materials; const uint32_t* idx; LeafTri* leaf; uint32_t triOffset, n, nVerts, nMaterials; uint32_t* result; };
__global__ void __launch_bounds__(kBlock) k_mu_leaves(MuLeafArgs a) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.n) return;
  const uint32_t t = a.idx[k];
  if (t >= a.n) { a.result[1] = 2u; return; }              // (not a permutation: the update is then refused, not trusted)
  const u4 tv = a.triVerts[t];
  if (tv.x >= a.nVerts || tv.y >= a.nVerts || tv.z >= a.nVerts || tv.w >= a.nMaterials) { a.result[1] = 2u; return; }
  LeafTri lt;
  muLeafRecord(lt, a.pos + size_t(tv.x) * 3, a.pos + size_t(tv.y) * 3, a.pos + size_t(tv.z) * 3, a.triOffset + t, tv.w, a.materials[tv.w].flags);
  a.leaf[k] = lt;
}

// prefix[k] = records with MAT_HAS_ALPHA among the first k of the leaf order (n + 1 entries): one workgroup walks the array in chunks
// of its size and carries the count (alpha-tested meshes are foliage and cards, not the large meshes of a scene)
constexpr uint32_t kMuScanBlock = 1024;
__global__ void __launch_bounds__(kMuScanBlock) k_mu_alpha_scan(const LeafTri* leaf, uint32_t* prefix, uint32_t n) {
  __shared__ uint32_t waveSum[kMuScanBlock / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  if (threadIdx.x == 0) prefix[0] = 0u;
  for (uint32_t base = 0; base < n; base += kMuScanBlock) {
    const uint32_t p = base + threadIdx.x;
    const bool flag = p < n && (leaf[p].matFlags & MAT_HAS_ALPHA) != 0u;
    const unsigned long long m = __ballot(flag);
    const uint32_t inWave = uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
    __syncthreads();                                       // (the previous chunk's sums have been read)
    if (lane == 0) waveSum[wave] = uint32_t(__popcll(m));
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kMuScanBlock / 64; w++) { const uint32_t c = waveSum[w]; if (w < wave) before += c; all += c; }
    if (p < n) prefix[p + 1u] = carry + before + inWave + (flag ? 1u : 0u);
    carry += all;
  }
}

// result words: [0] the deepest leaf (= bvhStackNeed), [1] error (1 a leaf span that does not fit the long-span word, 2 internal),
// [2] the root's alpha flag
struct MuLinkArgs { devbvh::Args b; const uint32_t* prefix; LeafTri* leaf; uint32_t* result; uint32_t nNodes; };
__global__ void __launch_bounds__(kBlock) k_mu_links(MuLinkArgs a, uint32_t base, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const devbvh::BNode nd = a.b.nodes[base + i];
  const bool leaf = nd.left == devbvh::kNoChild;
  // (k_emit's placement: the children pair of an inner node of rank k stands at 1 + 2 k)
  const uint32_t at = nd.parent == devbvh::kNoChild ? 0u : 1u + 2u * devbvh::globalRank(a.b, a.b.nodes[nd.parent]) + (nd.info & devbvh::NODE_RIGHT ? 1u : 0u);
  if (at >= a.nNodes || nd.first + nd.span > a.b.n || nd.span == 0u) { a.result[1] = 2u; return; }
  const bool alpha = a.prefix != nullptr && a.prefix[nd.first + nd.span] != a.prefix[nd.first];
  a.b.out[at].leftFirst = leaf ? muLinkWord(nd.first, nd.span, alpha) : muLinkWord(1u + 2u * devbvh::globalRank(a.b, nd), 0u, alpha);
  if (nd.parent == devbvh::kNoChild) a.result[2] = alpha ? 1u : 0u;
  if (!leaf) return;
  if (!muLeafSpanFits(nd.span)) { a.result[1] = 1u; return; }
  a.leaf[nd.first].matFlags |= muLongSpanWord(nd.span);
  uint32_t depth = 0;
  for (uint32_t p = nd.parent; p != devbvh::kNoChild && p < a.b.n * 4u && depth < 4096u; p = a.b.nodes[p].parent) depth++;   // (at most kMaxLevels + kLocalStack)
  atomicMax(a.result, depth);
}

constexpr UpdateCheck muCheck{"scene_update_meshes: "};

// Everything that can refuse an update before a mesh is built (behind updateHead's checks)
void muValidateArguments(const YartSceneMeshUpdate& u) {
  muCheck(u.meshes != nullptr, "meshes pointer is null");
  checkUpdateFlags(muCheck, u.flags);
  muCheck(u.n_meshes >= 1u, "n_meshes is 0");
}
// ... and what compares it with the scene; boxes: the new vertex box of every listed mesh
void muValidateAgainstScene(const YartScene& scene, const YartSceneMeshUpdate& u, std::vector<SuBox>& boxes) {
  const HostImage& h = scene.host;
  muCheck(u.n_meshes <= h.meshes.size(), "n_meshes is " + std::to_string(u.n_meshes) + ", the scene has " + std::to_string(h.meshes.size()) + " meshes");
  std::vector<uint8_t> listed(h.meshes.size(), 0);
  boxes.resize(u.n_meshes);
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const YartMeshUpdate& m = u.meshes[k];
    const std::string name = "mesh " + std::to_string(m.mesh);
    muCheck(m.mesh < h.meshes.size(), name + ": index out of range");
    muCheck(!listed[m.mesh], name + " is listed twice");
    listed[m.mesh] = 1;
    muCheck(m.n_vertices == h.meshes[m.mesh].nVerts, name + ": n_vertices is " + std::to_string(m.n_vertices) + ", the mesh has " +
                                                         std::to_string(h.meshes[m.mesh].nVerts) + " (the vertex count cannot change)");
    muCheck(m.positions != nullptr, name + ": positions pointer is null");
    const size_t nv = m.n_vertices;
    muCheck(finiteWords(m.positions, nv * 3u), name + ": a position word is not finite");
    muCheck(!m.normals || finiteWords(m.normals, nv * 3u), name + ": a normal word is not finite");
    muCheck(!m.tangents || finiteWords(m.tangents, nv * 4u), name + ": a tangent word is not finite");
    boxes[k] = muVertexBox(m.positions, m.n_vertices);
  }
  checkMeshBoxes(muCheck, h, listed.data());
}

// What a mesh is staged from: its counts, the caller's vertex arrays (host), its faces on the host and on the device (x, y, z vertices,
// w material), the offset its ShadeTri records will have, and whether a face has an alpha-tested material. yart_hip_scene_update_meshes
// takes faces, counts and offset from the scene; yart_hip_scene_replace_meshes (mesh_replace_kernels.inc) from its caller.
struct MuStageIn {
  uint32_t mesh, nVerts, nTris, triOffset;
  const float *positions, *normals, *tangents;
  const u4 *facesHost, *facesDev;
  bool alpha;
};

// One listed mesh into its staging arrays: upload, build, derive. Nothing of the scene is written. check: the entry's.
void muStageCore(YartScene& s, const MuStageIn& m, MeshStage& st, UpdateCall& call, const UpdateCheck& check) {
  const hipStream_t stream = call.stream;
  const HostImage& h = s.host;
  MeshUpdateState& mu = s.meshUp;
  const uint32_t nv = m.nVerts, nt = m.nTris;
  st.pos.ensure(size_t(nv) * 3u);
  HIP_CHECK(hipMemcpyAsync(st.pos.p, m.positions, size_t(nv) * 12u, hipMemcpyHostToDevice, stream));
  if (m.normals) { st.nrm.ensure(size_t(nv) * 3u); HIP_CHECK(hipMemcpyAsync(st.nrm.p, m.normals, size_t(nv) * 12u, hipMemcpyHostToDevice, stream)); }
  if (m.tangents) { st.tan.ensure(size_t(nv) * 4u); HIP_CHECK(hipMemcpyAsync(st.tan.p, m.tangents, size_t(nv) * 16u, hipMemcpyHostToDevice, stream)); }
  st.nodes.ensure(size_t(nt) * 2u); st.idx.ensure(nt); st.leaf.ensure(nt);
  mu.result.ensure(4);
  const uint32_t* faces = reinterpret_cast<const uint32_t*>(m.facesDev);
  devbvh::Built built;
  uint32_t res[3] = {0u, 0u, 0u};
  st.idxHost.resize(nt);
  const bool hostBuild = std::getenv("YART_HOST_BVH") != nullptr;      // (as scene creation: the host builder on request)
  if (!hostBuild && devbvh::buildCore(mu.scratch, st.pos.p, faces, 4u, nt, st.nodes.p, st.idx.p, stream, built, nullptr)) {
    call.launchedBy(built.launches);
    st.nNodes = built.nNodes();
    HIP_CHECK(hipMemsetAsync(mu.result.p, 0, 16, stream));
    MuLeafArgs la{st.pos.p, m.facesDev, s.materials.p, st.idx.p, st.leaf.p, m.triOffset, nt, nv, uint32_t(h.materials.size()), mu.result.p};
    hipLaunchKernelGGL(k_mu_leaves, dim3((nt + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, la);
    call.launched();
    const bool alpha = m.alpha;
    if (alpha) {
      mu.prefix.ensure(size_t(nt) + 1u);
      hipLaunchKernelGGL(k_mu_alpha_scan, dim3(1), dim3(kMuScanBlock), 0, stream, st.leaf.p, mu.prefix.p, nt);
      call.launched();
    }
    MuLinkArgs ka{built.args, alpha ? mu.prefix.p : nullptr, st.leaf.p, mu.result.p, st.nNodes};
    hipLaunchKernelGGL(k_mu_links, dim3((built.created + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, ka, 0u, built.created);
    call.launched();
    if (built.createdLocal) {
      hipLaunchKernelGGL(k_mu_links, dim3((built.createdLocal + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, ka, nt * 2u, built.createdLocal);
      call.launched();
    }
    HIP_CHECK(hipMemcpyAsync(res, mu.result.p, 12, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(st.idxHost.data(), st.idx.p, size_t(nt) * 4u, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    check(res[1] != 1u, "mesh " + std::to_string(m.mesh) + ": a BVH leaf of 2^24 or more triangles is not supported");
    if (res[1]) throw HipError(std::string(check.prefix) + "the device build of mesh " + std::to_string(m.mesh) + " is inconsistent");
    st.need = res[0]; st.hasAlpha = res[2];
  } else {
    // more levels than the level kernels take, or YART_HOST_BVH: the host builder (the same bytes) and the host statement of the derivation
    call.launchedBy(built.launches);
    SahBvhBuilder hb;
    const char* e = std::getenv("YART_BVH_THREADS");
    hb.setThreads(e ? unsigned(std::atoi(e)) : 0u);
    hb.build(m.positions, reinterpret_cast<const uint32_t*>(m.facesHost), 4, nt);
    std::vector<uint32_t> flags;
    for (const MaterialDev& mt : h.materials) flags.push_back(mt.flags);
    std::vector<BvhNode> nodes(hb.nodes.size());
    std::vector<LeafTri> leaf(nt);
    const MuDerived d = muDeriveHost(hb.nodes.data(), uint32_t(hb.nodes.size()), hb.indices.data(), nt, m.positions, m.facesHost,
                                     m.triOffset, flags.data(), nodes.data(), leaf.data());
    st.nNodes = uint32_t(nodes.size()); st.need = d.stackNeed; st.hasAlpha = d.hasAlpha;
    st.idxHost = hb.indices;
    if (st.need <= kMaxStackBound) {
      HIP_CHECK(hipMemcpyAsync(st.nodes.p, nodes.data(), nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice, stream));
      HIP_CHECK(hipMemcpyAsync(st.leaf.p, leaf.data(), leaf.size() * sizeof(LeafTri), hipMemcpyHostToDevice, stream));
      HIP_CHECK(hipMemcpyAsync(st.idx.p, st.idxHost.data(), size_t(nt) * 4u, hipMemcpyHostToDevice, stream));
      HIP_CHECK(hipStreamSynchronize(stream));               // (the host arrays end with this block)
    }
  }
  checkStackBound(st.need, m.mesh);                          // create's message: "mesh N: its BVH is D levels deep, ..."
}

// ... a mesh of yart_hip_scene_update_meshes: the scene's own faces and counts
void muStageMesh(YartScene& s, const YartMeshUpdate& m, MeshStage& st, UpdateCall& call) {
  const HostImage& h = s.host;
  MeshUpdateState& mu = s.meshUp;
  const MeshDev& md = h.meshes[m.mesh];
  if (mu.meshAlpha.size() != h.meshes.size()) mu.meshAlpha.assign(h.meshes.size(), int8_t(-1));
  if (mu.meshAlpha[m.mesh] < 0) {                          // does a face of the mesh have an alpha-tested material? (kept until the faces or a flag change)
    int8_t any = 0;
    for (uint32_t f = 0; f < md.nTris && !any; f++) any = (h.materials[h.triVerts[md.triOffset + f].w].flags & MAT_HAS_ALPHA) ? 1 : 0;
    mu.meshAlpha[m.mesh] = any;
  }
  const MuStageIn in{m.mesh, md.nVerts, md.nTris, md.triOffset, m.positions, m.normals, m.tangents, h.triVerts.data() + md.triOffset,
                     s.triVerts.p + md.triOffset, mu.meshAlpha[m.mesh] > 0};
  muStageCore(s, in, st, call, muCheck);
}

// What follows the meshes' own records, for yart_hip_scene_update_meshes and yart_hip_scene_replace_meshes alike (the host image holds
// the new MeshDev records, stack needs and vertex boxes of the `listed` meshes): the MeshDev array, the stack bound, and the nodes'
// boxes, world boxes and top-level hierarchy through the scene-update chain. nodes / flags: the caller's, declared before its frame.
void muRederiveScene(YartScene& s, const std::vector<uint32_t>& listed, uint32_t updateFlags, std::vector<YartNodeDesc>& nodes,
                     std::vector<uint32_t>& flags, UpdateCall& call) {
  const hipStream_t stream = call.stream;
  HostImage& h = s.host;
  HIP_CHECK(hipMemcpyAsync(s.meshes.p, h.meshes.data(), h.meshes.size() * sizeof(MeshDev), hipMemcpyHostToDevice, stream));
  // the stack bound as create derives it: the deepest mesh, and the top-level hierarchy's height (a median split's: it depends on
  // the number of mesh nodes only)
  uint32_t bound = h.tlasHeight;
  for (uint32_t need : h.meshStackNeed) bound = std::max(bound, need);
  h.stackBound = bound;
  // the nodes' boxes, world boxes and the top-level hierarchy over the new vertex boxes: the scene-update chain, current transforms
  if (!s.su.ready) suBuildTables(s);                        // (uploads h.meshBox)
  else for (uint32_t mesh : listed)
    HIP_CHECK(hipMemcpyAsync(s.su.meshBox.p + mesh, &h.meshBox[mesh], sizeof(SuBox), hipMemcpyHostToDevice, stream));
  // (the chain takes transforms as the caller of yart_hip_scene_update gives them — its scatter kernel reads YartNodeDesc records —, so
  // the current ones go to it in that form)
  nodes.resize(h.nodes.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    nodes[i].parent = h.nodes[i].parent; nodes[i].mesh = h.nodes[i].mesh;
    std::memcpy(nodes[i].fwd, h.nodes[i].xf.fwd, 64); std::memcpy(nodes[i].inv, h.nodes[i].xf.inv, 64);
  }
  YartSceneUpdate su{};
  su.struct_size = sizeof(su); su.n_nodes = uint32_t(nodes.size()); su.nodes = nodes.data(); su.flags = updateFlags;
  flags.resize(nodes.size());
  suRun(s, su, flags, suIdentityFlags(su.nodes, su.n_nodes, flags.data()), call);
}

void muUpdate(YartScene& s, const YartSceneMeshUpdate& u, const std::vector<SuBox>& boxes, hipStream_t stream, YartSceneUpdateStats* stats) {
  std::vector<YartNodeDesc> nodes;                           // (copies read the two: before the frame)
  std::vector<uint32_t> flags;
  UpdateCall call(WallClock::now(), s.device, stream);
  HostImage& h = s.host;
  MeshUpdateState& mu = s.meshUp;
  while (mu.stages.size() < u.n_meshes) mu.stages.push_back(std::make_unique<MeshStage>());
  for (uint32_t k = 0; k < u.n_meshes; k++) muStageMesh(s, u.meshes[k], *mu.stages[k], call);

  // ---- every listed mesh has built: from here on the scene is written
  const uint32_t nm = uint32_t(h.meshes.size());
  bool countChanged = false;
  for (uint32_t k = 0; k < u.n_meshes; k++) countChanged |= mu.stages[k]->nNodes != h.meshes[u.meshes[k].mesh].nNodes;
  if (countChanged) {
    // bvhNodes as create packs it, into the second array: every mesh base odd, two zero records behind the last mesh. Both arrays
    // are sized once for the largest trees the meshes can have (2 nTris - 1 nodes and a pad record each)
    std::vector<int32_t> stageOf(nm, -1);
    for (uint32_t k = 0; k < u.n_meshes; k++) stageOf[u.meshes[k].mesh] = int32_t(k);
    size_t worst = 2u, size = 0;
    std::vector<uint32_t> offset(nm);
    for (uint32_t mi = 0; mi < nm; mi++) {
      worst += size_t(h.meshes[mi].nTris) * 2u;
      if (size % 2u == 0u) size++;
      offset[mi] = uint32_t(size);
      size += stageOf[mi] >= 0 ? mu.stages[stageOf[mi]]->nNodes : h.meshes[mi].nNodes;
    }
    size += 2u;
    muCheck(size <= worst, "internal: the repacked node array is larger than its bound");
    mu.nodesAlt.ensure(worst);
    HIP_CHECK(hipMemsetAsync(mu.nodesAlt.p, 0, size * sizeof(BvhNode), stream));
    for (uint32_t mi = 0; mi < nm; mi++) {
      const BvhNode* from = stageOf[mi] >= 0 ? mu.stages[stageOf[mi]]->nodes.p : s.bvhNodes.p + h.meshes[mi].nodeOffset;
      const uint32_t n = stageOf[mi] >= 0 ? mu.stages[stageOf[mi]]->nNodes : h.meshes[mi].nNodes;
      HIP_CHECK(hipMemcpyAsync(mu.nodesAlt.p + offset[mi], from, size_t(n) * sizeof(BvhNode), hipMemcpyDeviceToDevice, stream));
      h.meshes[mi].nodeOffset = offset[mi];
    }
    std::swap(s.bvhNodes.p, mu.nodesAlt.p); std::swap(s.bvhNodes.n, mu.nodesAlt.n);
    s.dev.bvhNodes = s.bvhNodes.p;
  }
  bool lightsChange = false;
  for (uint32_t k = 0; k < u.n_meshes; k++) {
    const YartMeshUpdate& m = u.meshes[k];
    MeshStage& st = *mu.stages[k];
    MeshDev& md = h.meshes[m.mesh];
    if (!countChanged)
      HIP_CHECK(hipMemcpyAsync(s.bvhNodes.p + md.nodeOffset, st.nodes.p, size_t(st.nNodes) * sizeof(BvhNode), hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(s.leafTris.p + md.leafOffset, st.leaf.p, size_t(md.nTris) * sizeof(LeafTri), hipMemcpyDeviceToDevice, stream));
    MuVertArgs va{st.pos.p, m.normals ? st.nrm.p : nullptr, m.tangents ? st.tan.p : nullptr, s.vPos.p + md.vertOffset, s.vNormal.p + md.vertOffset,
                  s.vTangent.p + md.vertOffset, md.nVerts};
    hipLaunchKernelGGL(k_mu_verts, dim3((md.nVerts + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, va);
    call.launched();
    if (m.normals || m.tangents) {
      MuShadeArgs sa{va.nrm, va.tan, s.triVerts.p + md.triOffset, s.shadeTris.p + md.triOffset, md.nTris, md.nVerts};
      hipLaunchKernelGGL(k_mu_shade, dim3((md.nTris + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, sa);
      call.launched();
    }
    // the host image: what the library reads after create (yart_hip_bvh_info / _copy, the lights' vertices, the next update's boxes)
    md.nNodes = st.nNodes; md.hasAlpha = st.hasAlpha;
    h.meshStackNeed[m.mesh] = st.need;
    h.meshBox[m.mesh] = boxes[k];
    h.bvhIndices[m.mesh] = st.idxHost;
    for (uint32_t v = 0; v < md.nVerts; v++) {
      f4& p = h.vPos[md.vertOffset + v];
      p.x = m.positions[3u * size_t(v)]; p.y = m.positions[3u * size_t(v) + 1u]; p.z = m.positions[3u * size_t(v) + 2u]; p.w = 0.0f;
    }
    for (uint32_t i = 0; i < h.nLights; i++) lightsChange |= h.lights[i].type == LIGHT_AREA && h.lights[i].mesh == int32_t(m.mesh);
  }
  std::vector<uint32_t> listed;
  for (uint32_t k = 0; k < u.n_meshes; k++) listed.push_back(u.meshes[k].mesh);
  muRederiveScene(s, listed, u.flags, nodes, flags, call);
  if (lightsChange) {                                        // area lights on an updated mesh: from the host's new vertices, as create derives them
    const std::vector<YartLightDesc> desc = h.lightDesc;
    rederiveLights(h, desc.data(), h.nLights);
    uploadLights(s, stream);
    call.close();                                            // (once more: suRun closed the frame before this upload)
  }
  call.finish(stats);
}

}  // namespace

extern "C" {

int yart_hip_scene_update_meshes(YartScene* scene, const YartSceneMeshUpdate* update, void* stream, YartSceneUpdateStats* stats) {
  std::vector<SuBox> boxes;                                  // (the listed meshes' new vertex boxes: from the checks to the run)
  return updateEntry(
      muCheck, "YartSceneMeshUpdate", scene, update, stream, stats,
      [&](const YartSceneMeshUpdate& u) { muValidateArguments(u); checkDeviceRebuildHandle(muCheck, u.flags, scene); },
      [&](const YartScene& s, const YartSceneMeshUpdate& u) { muValidateAgainstScene(s, u, boxes); },
      [&](YartScene& s, const YartSceneMeshUpdate& u, hipStream_t st, YartSceneUpdateStats* out) { muUpdate(s, u, boxes, st, out); });
}

int yart_hip_probe_mesh(YartScene* scene, uint32_t mesh, void* mesh_dev_out, void* nodes_out, void* leaf_out, void* shade_out, float* vpos_out,
                        float* vnormal_out, float* vtangent_out, uint32_t* stack_bound_out) {
  return guarded([&] {
    require(scene, "probe_mesh: scene pointer is null");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    require(mesh < s.host.meshes.size(), "probe_mesh: mesh index out of range");
    HIP_CHECK(hipSetDevice(s.device));
    MeshDev md;
    HIP_CHECK(hipMemcpy(&md, s.meshes.p + mesh, sizeof(md), hipMemcpyDeviceToHost));
    const MeshDev& hm = s.host.meshes[mesh];
    // (the copies below are sized by the device record: it has to agree with the host's on everything that sizes an array)
    require(md.nTris == hm.nTris && md.nVerts == hm.nVerts && md.nNodes == hm.nNodes && md.nNodes <= 2u * md.nTris && md.nodeOffset == hm.nodeOffset &&
            md.leafOffset == hm.leafOffset && md.triOffset == hm.triOffset && md.vertOffset == hm.vertOffset,
            "probe_mesh: the device's MeshDev record disagrees with the host's");
    if (mesh_dev_out) std::memcpy(mesh_dev_out, &md, sizeof(md));
    if (nodes_out) HIP_CHECK(hipMemcpy(nodes_out, s.bvhNodes.p + md.nodeOffset, size_t(md.nNodes) * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (leaf_out) HIP_CHECK(hipMemcpy(leaf_out, s.leafTris.p + md.leafOffset, size_t(md.nTris) * sizeof(LeafTri), hipMemcpyDeviceToHost));
    if (shade_out) HIP_CHECK(hipMemcpy(shade_out, s.shadeTris.p + md.triOffset, size_t(md.nTris) * sizeof(ShadeTri), hipMemcpyDeviceToHost));
    if (vpos_out) HIP_CHECK(hipMemcpy(vpos_out, s.vPos.p + md.vertOffset, size_t(md.nVerts) * sizeof(f4), hipMemcpyDeviceToHost));
    if (vnormal_out) HIP_CHECK(hipMemcpy(vnormal_out, s.vNormal.p + md.vertOffset, size_t(md.nVerts) * sizeof(f4), hipMemcpyDeviceToHost));
    if (vtangent_out) HIP_CHECK(hipMemcpy(vtangent_out, s.vTangent.p + md.vertOffset, size_t(md.nVerts) * sizeof(f4), hipMemcpyDeviceToHost));
    if (stack_bound_out) *stack_bound_out = s.host.stackBound;
  });
}

}  // extern "C"
