// graph_update_kernels.inc — yart_hip_scene_update_graph: a new node list for a scene that is on the device — nodes added, removed,
// hidden, re-meshed or re-parented (included by yart_hip.hip, unit 0, behind scene_update_kernels.inc: the entry ends in suRun).
// The topology pass is csrc/graph_update.hpp's, on the host: integers only, one sweep over the new list. What runs on the stream:
//
//   the copies       per node its descriptor (136 B, suRun's staging) and its GuTopo record (16 B); the level tables of the new graph
//   k_gu_topology    one lane per node: parent, mesh, skip, depth into NodeDev and the two .w words of the nodeWorld pair — in front
//                    of k_su_scatter, which reads the node's mesh
//   suRun            unchanged: k_su_scatter, k_su_fold per level, k_su_world, then tbBuild over the new leaf list (or the host's
//                    buildTopLevel under YART_UPDATE_REBUILD_TOP), the lights, the closing synchronisation
//
// No NodeDev array is built on the host and uploaded, except for a graph of more than kSceneUpdateMaxLevels levels, which suRun
// re-derives on the host as it always has (guApplyHost gives it the topology).
namespace {

struct GuTopoArgs { const GuTopo* topo; NodeDev* nodes; f4* nodeWorld; uint32_t nNodes; };
__global__ void __launch_bounds__(kBlock) k_gu_topology(GuTopoArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nNodes) return;
  guApplyNode(a.topo[i], i, a.nNodes, a.nodes[i], a.nodeWorld[size_t(i) * 2u], a.nodeWorld[size_t(i) * 2u + 1u]);
}

constexpr UpdateCheck guCheck{"scene_update_graph: "};

// Everything that can refuse the update, before anything is written: what the list says about itself, then what compares it with
// the scene
void guValidateArguments(const YartSceneGraphUpdate& u) {
  guCheck(u.nodes != nullptr, "nodes pointer is null");
  checkUpdateFlags(guCheck, u.flags);
  guCheck(u.n_nodes >= 1u && u.n_nodes < kGuMaxNodes, "n_nodes is " + std::to_string(u.n_nodes) + ": a scene has 1 .. 2^20 - 1 nodes");
  guCheck(u.nodes[0].parent == -1, "node 0: the root's parent is not -1");
  for (uint32_t i = 1; i < u.n_nodes; i++)
    guCheck(u.nodes[i].parent >= 0 && uint32_t(u.nodes[i].parent) < i,
            "node " + std::to_string(i) + ": its parent is negative or not below the node's index (the list is in pre-order)");
}
void guValidateAgainstScene(const YartScene& scene, const YartSceneGraphUpdate& u) {
  const HostImage& h = scene.host;
  checkLightCount(guCheck, h, u.n_lights, u.lights);
  uint32_t meshNodes = 0;
  for (uint32_t i = 0; i < u.n_nodes; i++) {
    guCheck(u.nodes[i].mesh < int32_t(h.meshes.size()),
            "node " + std::to_string(i) + ": mesh index " + std::to_string(u.nodes[i].mesh) + " of " + std::to_string(h.meshes.size()) + " meshes");
    guCheck(finiteWords(u.nodes[i].fwd, 16) && finiteWords(u.nodes[i].inv, 16), "node " + std::to_string(i) + ": a matrix word is not finite");
    if (u.nodes[i].mesh >= 0) meshNodes++;
  }
  checkLightTransforms(guCheck, h, u.n_lights, u.lights);
  checkMeshBoxes(guCheck, h, nullptr);
  // the new hierarchy's height depends on the number of mesh nodes only (a median split): known here, as scene creation's
  // checkStackBound knows a mesh's
  const uint32_t height = u.n_nodes >= kTlasMinNodes ? guTlasHeight(meshNodes) : 0u;
  guCheck(height <= kMaxStackBound, "the top-level hierarchy would be " + std::to_string(height) + " levels high, the traversal stack holds at most " +
                                        std::to_string(kMaxStackBound));
}

template <class T>
void guReserve(DevBuf<T>& b, size_t count) { if (count > b.n) b.ensure(guCapacity(count)); }
// a table of the pass to the device, on the stream (the vector is the scene's: it outlives the copy)
void guUpload(DevBuf<uint32_t>& b, const std::vector<uint32_t>& v, hipStream_t stream) {
  guReserve(b, v.size());
  HIP_CHECK(hipMemcpyAsync(b.p, v.data(), v.size() * 4u, hipMemcpyHostToDevice, stream));
}

void guUpdate(YartScene& s, const YartSceneGraphUpdate& u, hipStream_t stream, YartSceneUpdateStats* stats) {
  const auto wall0 = WallClock::now();
  HostImage& h = s.host;
  SceneUpdateTables& t = s.su;
  GuDerived& g = s.graphUp.derived;                          // (the scene's: the stream's copies read its arrays)
  const uint32_t nn = u.n_nodes;
  const bool hostTop = (u.flags & YART_UPDATE_REBUILD_TOP) != 0u;
  guDerive(u.nodes, nn, kSuFanOut, g);
  UpdateCall call(wall0, s.device, stream);
  // the arrays a longer list outgrows, and what points into them
  guReserve(s.nodes, nn); guReserve(s.nodeWorld, size_t(nn) * 2u); guReserve(s.tlas, std::max(g.tlasRecords, 1u));
  guReserve(t.stageDesc, size_t(nn) * 34u); guReserve(t.stageFlags, nn);
  s.dev.nodes = s.nodes.p; s.dev.nodeWorld = s.nodeWorld.p; s.dev.tlas = s.tlas.p;
  s.dev.nNodes = nn; s.dev.nTlas = g.tlasRecords;
  // the host image's side of the node count and of the tree's shape (the records themselves come back from the device in suRun)
  h.nodes.resize(nn); h.nodeWorld.resize(size_t(nn) * 2u);
  h.tlas.assign(std::max(g.tlasRecords, 1u), TlasNode{});
  h.tlasHeight = g.tlasHeight; h.maxNodeDepth = g.maxNodeDepth;
  h.stackBound = g.tlasHeight;
  for (uint32_t need : h.meshStackNeed) h.stackBound = std::max(h.stackBound, need);
  s.havePrevious = false;                                    // the kept node array is another list's
  // SceneUpdateTables of the new graph
  t.levels = g.levels; t.levelFirst = g.levelFirst; t.levelBig = g.levelBig; t.levelSmall = g.levelSmall;
  if (!t.ready) t.meshBox.upload(h.meshBox);
  if (g.levels <= kSceneUpdateMaxLevels) {
    guUpload(t.childOff, g.childOff, stream); guUpload(t.childIdx, g.childIdx, stream); guUpload(t.parents, g.parents, stream);
    DevBuf<uint32_t>& stage = s.graphUp.stageTopo;
    guReserve(stage, size_t(nn) * 4u);
    HIP_CHECK(hipMemcpyAsync(stage.p, g.topo.data(), size_t(nn) * sizeof(GuTopo), hipMemcpyHostToDevice, stream));
    GuTopoArgs ta{reinterpret_cast<const GuTopo*>(stage.p), s.nodes.p, s.nodeWorld.p, nn};
    hipLaunchKernelGGL(k_gu_topology, dim3((nn + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, ta);
    call.launched();
  } else {
    guApplyHost(g, h.nodes.data(), h.nodeWorld.data());
  }
  t.ready = true;
  t.tlasReady = false;                                       // the tree changes: a later refit lists its levels again
  // the tables of the new leaf list (blocking copies, and none when the list is the one the scene had); under the host's rebuild a
  // later device rebuild prepares them
  if (hostTop) {
    t.tlasBuild.ready = false;
  } else {
    TlasBuildState& b = t.tlasBuild;
    const size_t leaves = g.leafIds.size();
    if (leaves) {
      guReserve(b.dLeafIds, leaves); guReserve(b.ids, leaves); guReserve(b.dRecA, g.tlasRecords); guReserve(b.dOrder, g.tlasRecords);
      guReserve(b.dRoots, 2u * (leaves / (kTlasLocalLeaves / 2u) + 2u));       // (a subtree root holds more than half of kTlasLocalLeaves leaves)
    }
    tbPrepare(b, g.leafIds);
  }
  // transforms, boxes, world boxes, the hierarchy and the lights: the transform update's chain over the new tables
  YartSceneUpdate su{};
  su.struct_size = sizeof(su); su.n_nodes = nn; su.nodes = u.nodes; su.n_lights = u.n_lights; su.lights = u.lights;
  su.flags = hostTop ? YART_UPDATE_REBUILD_TOP : YART_UPDATE_REBUILD_TOP_DEVICE;
  suRun(s, su, g.flags, g.allIdentity, call);
  call.finish(stats);
}

}  // namespace

extern "C" {

int yart_hip_scene_update_graph(YartScene* scene, const YartSceneGraphUpdate* update, void* stream, YartSceneUpdateStats* stats) {
  return updateEntry(guCheck, "YartSceneGraphUpdate", scene, update, stream, stats,
                     [&](const YartSceneGraphUpdate& u) {
                       guValidateArguments(u);               // (flags 0 builds on the device too: the handle is checked as for the flag)
                       checkDeviceRebuildHandle(guCheck, (u.flags & YART_UPDATE_REBUILD_TOP) ? u.flags : YART_UPDATE_REBUILD_TOP_DEVICE, scene);
                     },
                     guValidateAgainstScene, guUpdate);
}

}  // extern "C"
