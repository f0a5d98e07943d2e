// scene_update_kernels.inc — yart_hip_scene_update: new node and light transforms for a scene that is on the device, and the
// kernels that re-derive what depends on the nodes' (included by yart_hip.hip, unit 0: the entry uses YartScene and guarded).
// The arithmetic is csrc/scene_update.hpp's; what each launch does:
//
//   k_su_scatter     transforms and identity flags into NodeDev, every box reset to the node's own mesh box
//   k_su_fold        one launch per level of the scene graph, deepest first: every node of the level that has children folds their
//                    contributions into its box. The children's boxes are final: they were written by the previous launch, and the
//                    launch boundary is the only hand-off (no in-launch counters, no float atomics)
//   k_su_world       the padded world boxes (nodeWorld x, y, z; the .w words belong to the topology and stay)
//   k_su_tlas_refit  one launch per level of the top-level hierarchy, leaves first: a leaf takes its node's world box, an inner node
//                    the min / max of its two children. The tree itself (a, b) stays
//   (YART_UPDATE_REBUILD_TOP_DEVICE: tlas_build_kernels.inc's launches in the refit's place — a new tree on the same stream)
//
// The tables the launches walk depend on the topology only; they are built at the scene's first update (SceneUpdateTables).
namespace {

// A parent of kSuFanOut children and more is folded by a workgroup — every lane folds a stride of the child range, then the
// workgroup reduces the kBlock partial folds in LDS with the (value, index) rule; a parent of fewer children by one lane, kBlock
// parents per workgroup. 32: below it one lane's serial loop is shorter than the eight reduction steps of the workgroup form.
constexpr uint32_t kSuFanOut = 32;

struct SuScatterArgs { const uint32_t* desc; const uint32_t* flags; const SuBox* meshBox; NodeDev* nodes; uint32_t nNodes; };
__global__ void __launch_bounds__(kBlock) k_su_scatter(SuScatterArgs a) {
  // one lane per (node, word of the transform pair): YartNodeDesc is parent, mesh, fwd[16], inv[16]; NodeDev starts with fwd, inv
  const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint32_t i = uint32_t(t >> 5), w = uint32_t(t & 31u);
  if (i >= a.nNodes) return;
  uint32_t* nd = reinterpret_cast<uint32_t*>(a.nodes + i);
  nd[w] = a.desc[size_t(i) * 34u + 2u + w];
  if (w < 6u) {
    const int32_t mesh = a.nodes[i].mesh;
    const float own = mesh >= 0 ? (w < 3u ? a.meshBox[mesh].mn[w] : a.meshBox[mesh].mx[w - 3u]) : (w < 3u ? kInf : -kInf);
    if (w < 3u) a.nodes[i].bmin[w] = own; else a.nodes[i].bmax[w - 3u] = own;
  } else if (w == 6u) {
    a.nodes[i].pad[0] = a.flags[i];
  }
}

struct SuFoldArgs {
  NodeDev* nodes; const uint32_t* parents; const uint32_t* childOff; const uint32_t* childIdx;
  uint32_t first, nBig, nSmall;      // the level's range of `parents`: nBig parents of kSuFanOut children and more, then nSmall others
};
__device__ __forceinline__ SuFold suFoldChildren(const SuFoldArgs& a, uint32_t p, uint32_t lane, uint32_t lanes) {
  SuFold f = suFoldIdentity();
  for (uint32_t k = a.childOff[p] + lane; k < a.childOff[p + 1u]; k += lanes) {
    const uint32_t c = a.childIdx[k];
    const NodeDev& cn = a.nodes[c];
    suFoldJoin(f, suFoldOf(suChildContribution(cn.xf.fwd, cn.bmin, cn.bmax), c));
  }
  return f;
}
__device__ __forceinline__ void suStoreBox(NodeDev& nd, SuFold f) {
  SuBox own;
  for (int c = 0; c < 3; c++) { own.mn[c] = nd.bmin[c]; own.mx[c] = nd.bmax[c]; }       // (k_su_scatter reset it to the mesh box)
  suFoldJoin(f, suFoldOf(own, kSuOwnBox));
  for (int c = 0; c < 3; c++) { nd.bmin[c] = f.mn[c]; nd.bmax[c] = f.mx[c]; }
}
__global__ void __launch_bounds__(kBlock) k_su_fold(SuFoldArgs a) {
  __shared__ SuFold part[kBlock];
  if (blockIdx.x < a.nBig) {                                    // (uniform per workgroup)
    const uint32_t p = a.parents[a.first + blockIdx.x];
    part[threadIdx.x] = suFoldChildren(a, p, threadIdx.x, kBlock);
    __syncthreads();
    for (uint32_t s = kBlock / 2u; s > 0u; s >>= 1) {
      if (threadIdx.x < s) { SuFold f = part[threadIdx.x]; suFoldJoin(f, part[threadIdx.x + s]); part[threadIdx.x] = f; }
      __syncthreads();
    }
    if (threadIdx.x == 0u) suStoreBox(a.nodes[p], part[0]);
    return;
  }
  const uint32_t k = (blockIdx.x - a.nBig) * kBlock + threadIdx.x;
  if (k >= a.nSmall) return;
  const uint32_t p = a.parents[a.first + a.nBig + k];
  suStoreBox(a.nodes[p], suFoldChildren(a, p, 0u, 1u));
}

struct SuWorldArgs { const NodeDev* nodes; f4* nodeWorld; uint32_t nNodes; };
__global__ void __launch_bounds__(kBlock) k_su_world(SuWorldArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nNodes) return;
  float lo[3], hi[3];
  suWorldBox(a.nodes, i, lo, hi);
  f4* o = a.nodeWorld + size_t(i) * 2u;
  o[0].x = lo[0]; o[0].y = lo[1]; o[0].z = lo[2];
  o[1].x = hi[0]; o[1].y = hi[1]; o[1].z = hi[2];
}

struct SuTlasArgs { TlasNode* tlas; const f4* nodeWorld; const uint32_t* order; uint32_t first, n; };   // `order`: tlas nodes by level
__global__ void __launch_bounds__(kBlock) k_su_tlas_refit(SuTlasArgs a) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.n) return;
  TlasNode& t = a.tlas[a.order[a.first + k]];
  if (t.b) {
    const f4 lo = a.nodeWorld[size_t(t.a) * 2u], hi = a.nodeWorld[size_t(t.a) * 2u + 1u];
    t.lo[0] = lo.x; t.lo[1] = lo.y; t.lo[2] = lo.z; t.hi[0] = hi.x; t.hi[1] = hi.y; t.hi[2] = hi.z;
  } else {
    const TlasNode& l = a.tlas[t.a]; const TlasNode& r = a.tlas[t.a + 1u];
    for (int c = 0; c < 3; c++) { t.lo[c] = stdmin(l.lo[c], r.lo[c]); t.hi[c] = stdmax(l.hi[c], r.hi[c]); }
  }
}

// The tables of SceneUpdateTables from the scene's topology (parent links, top-level tree), uploaded once.
void suBuildTables(YartScene& s) {
  SceneUpdateTables& u = s.su;
  const HostImage& h = s.host;
  const uint32_t nn = uint32_t(h.nodes.size());
  u.levels = h.maxNodeDepth + 1u;
  if (u.levels <= kSceneUpdateMaxLevels) {
    std::vector<uint32_t> off(size_t(nn) + 1u, 0u), idx(nn > 0u ? nn - 1u : 0u);
    for (uint32_t i = 1; i < nn; i++) off[size_t(h.nodes[i].parent) + 1u]++;
    for (uint32_t i = 0; i < nn; i++) off[i + 1u] += off[i];
    {
      std::vector<uint32_t> at(off.begin(), off.end() - 1);
      for (uint32_t i = 1; i < nn; i++) idx[at[h.nodes[i].parent]++] = i;              // ascending within a parent
    }
    // parents by level, the big ones of a level first
    std::vector<std::vector<uint32_t>> big(u.levels), small(u.levels);
    for (uint32_t i = 0; i < nn; i++) {
      const uint32_t nc = off[i + 1u] - off[i];
      if (nc) (nc >= kSuFanOut ? big : small)[h.nodes[i].depth].push_back(i);
    }
    std::vector<uint32_t> parents;
    u.levelFirst.clear(); u.levelBig.clear(); u.levelSmall.clear();
    for (uint32_t l = 0; l < u.levels; l++) {
      u.levelFirst.push_back(uint32_t(parents.size())); u.levelBig.push_back(uint32_t(big[l].size())); u.levelSmall.push_back(uint32_t(small[l].size()));
      parents.insert(parents.end(), big[l].begin(), big[l].end()); parents.insert(parents.end(), small[l].begin(), small[l].end());
    }
    if (idx.empty()) idx.push_back(0u);
    if (parents.empty()) parents.push_back(0u);
    u.childOff.upload(off); u.childIdx.upload(idx); u.parents.upload(parents);
  }
  u.meshBox.upload(h.meshBox);
  u.ready = true;
}

// ... and of the top-level tree (again after YART_UPDATE_REBUILD_TOP replaced it)
void suBuildTlasOrder(YartScene& s) {
  SceneUpdateTables& u = s.su;
  const HostImage& h = s.host;
  // the top-level tree's nodes by level (a child lies one level below its parent)
  u.tlasFirst.clear();
  if (s.dev.nTlas) {
    std::vector<uint32_t> level(h.tlas.size(), 0u), order;
    std::vector<std::vector<uint32_t>> byLevel;
    for (uint32_t k = 0; k < uint32_t(h.tlas.size()); k++) {           // children are allocated after their parent
      if (byLevel.size() <= level[k]) byLevel.resize(level[k] + 1u);
      byLevel[level[k]].push_back(k);
      if (!h.tlas[k].b) { level[h.tlas[k].a] = level[k] + 1u; level[h.tlas[k].a + 1u] = level[k] + 1u; }
    }
    for (const auto& l : byLevel) { u.tlasFirst.push_back(uint32_t(order.size())); order.insert(order.end(), l.begin(), l.end()); }
    u.tlasFirst.push_back(uint32_t(order.size()));
    u.tlasOrder.upload(order);
  }
  u.tlasReady = true;
}

constexpr UpdateCheck suCheck{"scene_update: "};

// Everything that can refuse an update, before anything is written: behind updateHead's checks what needs no look at the scene —
// before its lock is taken —, then what compares the update with the scene
void suValidateArguments(const YartSceneUpdate& u) {
  suCheck(u.nodes != nullptr, "nodes pointer is null");
  checkUpdateFlags(suCheck, u.flags);
}
void suValidateAgainstScene(const YartScene& scene, const YartSceneUpdate& u) {
  const HostImage& h = scene.host;
  suCheck(u.n_nodes == h.nodes.size(), "n_nodes is " + std::to_string(u.n_nodes) + ", the scene has " + std::to_string(h.nodes.size()) + " nodes");
  checkLightCount(suCheck, h, u.n_lights, u.lights);
  for (uint32_t i = 0; i < u.n_nodes; i++) {
    suCheck(u.nodes[i].parent == h.nodes[i].parent && u.nodes[i].mesh == h.nodes[i].mesh,
            "node " + std::to_string(i) + ": parent / mesh differ from the scene's (the topology cannot change)");
    suCheck(finiteWords(u.nodes[i].fwd, 16) && finiteWords(u.nodes[i].inv, 16), "node " + std::to_string(i) + ": a matrix word is not finite");
  }
  checkLightTransforms(suCheck, h, u.n_lights, u.lights);
  checkMeshBoxes(suCheck, h, nullptr);
}

// The chain in the caller's frame (the mesh update ends in it); returns with the frame closed: the stream synchronised.
// flags: suIdentityFlags' of u.nodes (a copy reads them: declared before the caller's frame)
void suRun(YartScene& s, const YartSceneUpdate& u, const std::vector<uint32_t>& flags, bool allIdentity, UpdateCall& call) {
  const hipStream_t stream = call.stream;
  HostImage& h = s.host;
  SceneUpdateTables& t = s.su;
  const uint32_t nn = u.n_nodes;
  if (!t.ready) suBuildTables(s);
  const bool deviceTop = s.dev.nTlas && (u.flags & YART_UPDATE_REBUILD_TOP_DEVICE);
  if (deviceTop && !t.tlasBuild.ready) {                       // (first use: the tables of the scene's leaf list, blocking uploads)
    std::vector<int32_t> mesh(nn);
    for (uint32_t i = 0; i < nn; i++) mesh[i] = h.nodes[i].mesh;
    tbPrepare(t.tlasBuild, tlasLeafIds(mesh.data(), nn));
    require(t.tlasBuild.shape.records() == s.dev.nTlas && t.tlasBuild.shape.height == h.tlasHeight, "scene_update: the top-level hierarchy's shape does not fit the scene's");
  }
  const uint32_t nodeBlocks = (nn + kBlock - 1u) / kBlock;
  if (t.levels <= kSceneUpdateMaxLevels) {
    t.stageDesc.ensure(size_t(nn) * 34u); t.stageFlags.ensure(nn);
    HIP_CHECK(hipMemcpyAsync(t.stageDesc.p, u.nodes, size_t(nn) * sizeof(YartNodeDesc), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(t.stageFlags.p, flags.data(), size_t(nn) * 4u, hipMemcpyHostToDevice, stream));
    SuScatterArgs sa{t.stageDesc.p, t.stageFlags.p, t.meshBox.p, s.nodes.p, nn};
    hipLaunchKernelGGL(k_su_scatter, dim3(uint32_t((uint64_t(nn) * 32u + kBlock - 1u) / kBlock)), dim3(kBlock), 0, stream, sa);
    call.launched();
    for (uint32_t l = t.levels; l-- > 0u;) {
      if (t.levelBig[l] + t.levelSmall[l] == 0u) continue;
      SuFoldArgs fa{s.nodes.p, t.parents.p, t.childOff.p, t.childIdx.p, t.levelFirst[l], t.levelBig[l], t.levelSmall[l]};
      hipLaunchKernelGGL(k_su_fold, dim3(t.levelBig[l] + (t.levelSmall[l] + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, fa);
      call.launched();
    }
    SuWorldArgs wa{s.nodes.p, s.nodeWorld.p, nn};
    hipLaunchKernelGGL(k_su_world, dim3(nodeBlocks), dim3(kBlock), 0, stream, wa);
    call.launched();
    HIP_CHECK(hipMemcpyAsync(h.nodes.data(), s.nodes.p, size_t(nn) * sizeof(NodeDev), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(h.nodeWorld.data(), s.nodeWorld.p, size_t(nn) * 2u * sizeof(f4), hipMemcpyDeviceToHost, stream));
  } else {
    std::vector<SuFold> scratch(nn);
    suRederiveHost(h.nodes.data(), h.nodeWorld.data(), nn, u.nodes, flags.data(), h.meshBox.data(), scratch.data());
    HIP_CHECK(hipMemcpyAsync(s.nodes.p, h.nodes.data(), size_t(nn) * sizeof(NodeDev), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(s.nodeWorld.p, h.nodeWorld.data(), size_t(nn) * 2u * sizeof(f4), hipMemcpyHostToDevice, stream));
  }
  if (deviceTop) {
    // the tree of a fresh scene, built on the stream behind k_su_world (or the upload of the host's nodeWorld): same shape, same
    // height — both depend on the number of mesh nodes only —, so the level lists of a later refit stay as they are
    call.launchedBy(tbBuild(t.tlasBuild, s.nodeWorld.p, s.tlas.p, stream));
    HIP_CHECK(hipMemcpyAsync(h.tlas.data(), s.tlas.p, h.tlas.size() * sizeof(TlasNode), hipMemcpyDeviceToHost, stream));
  } else if (s.dev.nTlas) {
    if (u.flags & YART_UPDATE_REBUILD_TOP) {
      HIP_CHECK(hipStreamSynchronize(stream));                 // (the new nodeWorld is in h.nodeWorld on both paths)
      std::vector<TlasNode> rebuilt;                           // (swapped in only once it is known to fit)
      const uint32_t height = buildTopLevel(h.nodes, h.nodeWorld, rebuilt);
      require(height <= h.stackBound && rebuilt.size() == s.dev.nTlas, "scene_update: the rebuilt top-level hierarchy does not fit the scene's");
      h.tlas.swap(rebuilt);
      h.tlasHeight = height;
      HIP_CHECK(hipMemcpyAsync(s.tlas.p, h.tlas.data(), h.tlas.size() * sizeof(TlasNode), hipMemcpyHostToDevice, stream));
      t.tlasReady = false;                                     // the tree changed: its level lists are rebuilt when a refit needs them
    } else {
      if (!t.tlasReady) suBuildTlasOrder(s);
      for (size_t l = t.tlasFirst.size() - 1u; l-- > 0u;) {
        SuTlasArgs ta{s.tlas.p, s.nodeWorld.p, t.tlasOrder.p, t.tlasFirst[l], t.tlasFirst[l + 1u] - t.tlasFirst[l]};
        hipLaunchKernelGGL(k_su_tlas_refit, dim3((ta.n + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, ta);
        call.launched();
      }
      HIP_CHECK(hipMemcpyAsync(h.tlas.data(), s.tlas.p, h.tlas.size() * sizeof(TlasNode), hipMemcpyDeviceToHost, stream));
    }
  }
  if (u.n_lights) {                                            // the lights, on the host, by the code scene creation uses
    rederiveLights(h, u.lights, u.n_lights);
    uploadLights(s, stream);
  }
  call.close();
  h.allIdentity = allIdentity;                                 // (the render plan reads it: only once the device holds the new transforms)
}

void suUpdate(YartScene& s, const YartSceneUpdate& u, hipStream_t stream, YartSceneUpdateStats* stats) {
  const auto wall0 = WallClock::now();
  std::vector<uint32_t> flags(u.n_nodes);
  const bool allIdentity = suIdentityFlags(u.nodes, u.n_nodes, flags.data());
  UpdateCall call(wall0, s.device, stream);
  suRun(s, u, flags, allIdentity, call);
  call.finish(stats);
}

}  // namespace

extern "C" {

int yart_hip_scene_update(YartScene* scene, const YartSceneUpdate* update, void* stream, YartSceneUpdateStats* stats) {
  return updateEntry(suCheck, "YartSceneUpdate", scene, update, stream, stats,
                     [&](const YartSceneUpdate& u) { suValidateArguments(u); checkDeviceRebuildHandle(suCheck, u.flags, scene); },
                     suValidateAgainstScene, suUpdate);
}

}  // extern "C"
