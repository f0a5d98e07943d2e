// tlas_build_kernels.inc — the top-level hierarchy built on the device with host_scene.hpp::buildTopLevel's bytes (included by
// yart_hip.hip, unit 0, in front of scene_update_kernels.inc: YART_UPDATE_REBUILD_TOP_DEVICE ends the update chain in tbBuild; the
// stand-alone entries yart_hip_tlas_build_device / _host are at the end). The method and the facts it rests on are
// csrc/tlas_build.hpp's, whose tlasBuildLevelwise these launches restate:
//
//   per top level (a range of more than kTlasLocalLeaves leaves exists), over the whole leaf array:
//     k_tb_extent       per range of the level the smallest and largest centre key per axis: a min over each wave, one LDS
//                       integer min per wave and word, then one global
//                       integer min per workgroup and word (the largest as the min of the complement: one fill value for all)
//     k_tb_keys_sort    the keys (range number, centre key on the range's axis, node) and a bitonic sort of every tile of
//                       kTlasLocalLeaves keys in LDS
//     k_tb_global_step  one compare-exchange step of the bitonic network at a distance of a tile and more
//     k_tb_local_merge  the steps below a tile's size of one merge stage, in LDS; the last one writes the leaves' new order
//   k_tb_subtree        one workgroup per subtree root (a range of at most kTlasLocalLeaves leaves below a larger one, or the whole
//                       array): all of its remaining levels in LDS — extents by LDS integer min / max, the axis, one bitonic sort
//   k_tb_boxes          one launch per level of the tree, leaves first: links from the shape table, a leaf's box from nodeWorld,
//                       an inner node's from its two children (k_su_tlas_refit's arithmetic)
//
// The launch boundary is the only hand-off between workgroups; nothing waits inside a launch. tbLaunchBound says how many launches
// a leaf count takes.
namespace {

constexpr uint32_t kTbTile = kTlasLocalLeaves;            // keys a workgroup sorts in LDS
constexpr uint32_t kTbThreads = kTbTile / 2u;             // one lane per compare-exchange: 16 waves
static_assert((kTbTile & (kTbTile - 1u)) == 0u && kTbTile >= 2u * kBlock, "a power of two, and a k_tb_extent workgroup meets at most two ranges");

struct TbArgs {
  const f4* nodeWorld; uint32_t* ids; unsigned long long* keys; uint32_t* ext;
  uint32_t leaves, level, extFirst;               // extFirst: the level's first range in `ext` (6 words per range)
};

__global__ void __launch_bounds__(kBlock) k_tb_extent(TbArgs a) {
  __shared__ uint32_t sExt[2][6];
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  // (a top level's ranges hold at least kTlasLocalLeaves leaves: the workgroup's positions lie in this range or the next)
  const uint32_t firstOrd = tlasSegmentOf(0u, a.leaves, a.level, blockIdx.x * kBlock).ord;
  if (threadIdx.x < 12u) sExt[threadIdx.x / 6u][threadIdx.x % 6u] = 0xffffffffu;
  __syncthreads();
  // per lane the six words for its own range, the fill value for the other; a min over the wave (64 lanes), then one LDS min per
  // wave and word
  uint32_t v[2][6];
  for (int w = 0; w < 6; w++) v[0][w] = v[1][w] = 0xffffffffu;
  if (p < a.leaves) {
    const uint32_t slot = tlasSegmentOf(0u, a.leaves, a.level, p).ord != firstOrd ? 1u : 0u;
    const uint32_t node = a.ids[p];
    for (int c = 0; c < 3; c++) {
      const uint32_t k = tlasOrdKey(tlasCentre(a.nodeWorld, node, c));
      v[0][c] = slot ? 0xffffffffu : k; v[0][3 + c] = slot ? 0xffffffffu : ~k;
      v[1][c] = slot ? k : 0xffffffffu; v[1][3 + c] = slot ? ~k : 0xffffffffu;
    }
  }
  for (int s = 0; s < 2; s++)
    for (int w = 0; w < 6; w++) {
      uint32_t m = v[s][w];
      for (int o = 32; o > 0; o >>= 1) { const uint32_t other = uint32_t(__shfl_xor(int(m), o)); m = other < m ? other : m; }
      if ((threadIdx.x & 63u) == 0u && m != 0xffffffffu) atomicMin(&sExt[s][w], m);
    }
  __syncthreads();
  if (threadIdx.x < 12u) {                                // (`ext` has a spare range behind the last level's)
    const uint32_t word = sExt[threadIdx.x / 6u][threadIdx.x % 6u];
    if (word != 0xffffffffu) atomicMin(&a.ext[size_t(a.extFirst + firstOrd + threadIdx.x / 6u) * 6u + threadIdx.x % 6u], word);
  }
}

// the steps j = jFirst, jFirst / 2, .. 1 of the merge stage k on the tile s, whose first key has the global index `base`
__device__ __forceinline__ void tbMergeSteps(unsigned long long* s, uint32_t base, uint32_t k, uint32_t jFirst, uint32_t pairs) {
  for (uint32_t j = jFirst; j > 0u; j >>= 1) {
    if (threadIdx.x < pairs) {
      const uint32_t t = threadIdx.x;
      const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
      const bool up = ((base + i) & k) == 0u;
      const unsigned long long x = s[i], y = s[i + j];
      if ((x > y) == up) { s[i] = y; s[i + j] = x; }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kTbThreads) k_tb_keys_sort(TbArgs a) {
  __shared__ unsigned long long sKey[kTbTile];
  const uint32_t base = blockIdx.x * kTbTile;
  for (uint32_t e = threadIdx.x; e < kTbTile; e += kTbThreads) {
    const uint32_t p = base + e;
    unsigned long long key = ~0ull;                        // (the padding sorts behind every key)
    if (p < a.leaves) {
      const TlasSegment sg = tlasSegmentOf(0u, a.leaves, a.level, p);
      const uint32_t* x = a.ext + size_t(a.extFirst + sg.ord) * 6u;
      const uint32_t kmin[3] = {x[0], x[1], x[2]}, kmax[3] = {~x[3], ~x[4], ~x[5]};
      const uint32_t node = a.ids[p];
      key = tlasKey(sg.ord, tlasOrdKey(tlasCentre(a.nodeWorld, node, tlasAxis(kmin, kmax))), node);
    }
    sKey[e] = key;
  }
  __syncthreads();
  for (uint32_t k = 2u; k <= kTbTile; k <<= 1) tbMergeSteps(sKey, base, k, k >> 1, kTbThreads);
  for (uint32_t e = threadIdx.x; e < kTbTile; e += kTbThreads) a.keys[base + e] = sKey[e];
}

__global__ void __launch_bounds__(kBlock) k_tb_global_step(unsigned long long* keys, uint32_t padded, uint32_t k, uint32_t j) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= padded / 2u) return;
  const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
  const bool up = (i & k) == 0u;
  const unsigned long long x = keys[i], y = keys[i + j];
  if ((x > y) == up) { keys[i] = y; keys[i + j] = x; }
}

__global__ void __launch_bounds__(kTbThreads) k_tb_local_merge(TbArgs a, uint32_t k, uint32_t last) {
  __shared__ unsigned long long sKey[kTbTile];
  const uint32_t base = blockIdx.x * kTbTile;
  for (uint32_t e = threadIdx.x; e < kTbTile; e += kTbThreads) sKey[e] = a.keys[base + e];
  __syncthreads();
  tbMergeSteps(sKey, base, k, kTbTile >> 1, kTbThreads);
  for (uint32_t e = threadIdx.x; e < kTbTile; e += kTbThreads) {
    a.keys[base + e] = sKey[e];
    if (last && base + e < a.leaves) a.ids[base + e] = uint32_t(sKey[e]) & kTlasKeyNodeMask;
  }
}

struct TbSubArgs { const f4* nodeWorld; uint32_t* ids; const uint32_t* roots; };       // roots: lo, hi per subtree root
__global__ void __launch_bounds__(kTbThreads) k_tb_subtree(TbSubArgs a) {
  __shared__ unsigned long long sKey[kTbTile];
  __shared__ uint32_t sId[kTbTile];
  __shared__ uint32_t sExt[kTbTile / 2u][6];               // (a range of two leaves and more, d levels down, has a number below 2^d <= n / 2)
  const uint32_t lo = a.roots[2u * blockIdx.x], n = a.roots[2u * blockIdx.x + 1u] - lo;     // 1 <= n <= kTbTile
  uint32_t padded = 2u;
  while (padded < n) padded <<= 1;
  for (uint32_t e = threadIdx.x; e < n; e += kTbThreads) sId[e] = a.ids[lo + e];
  __syncthreads();
  for (uint32_t depth = 0; tlasLargestRange(n, depth) > 1u; depth++) {       // (at most 11 levels; uniform)
    const uint32_t nRanges = 1u << depth;
    for (uint32_t w = threadIdx.x; w < nRanges * 6u && w < (kTbTile / 2u) * 6u; w += kTbThreads) sExt[w / 6u][w % 6u] = w % 6u < 3u ? 0xffffffffu : 0u;
    __syncthreads();
    TlasSegment sg[2];
    uint32_t ck[2][3];
    for (uint32_t q = 0; q < 2u; q++) {
      const uint32_t e = threadIdx.x + q * kTbThreads;
      if (e >= n) continue;
      sg[q] = tlasSegmentOf(0u, n, depth, e);
      if (sg[q].hi - sg[q].lo < 2u) continue;
      for (int c = 0; c < 3; c++) {
        ck[q][c] = tlasOrdKey(tlasCentre(a.nodeWorld, sId[e], c));
        atomicMin(&sExt[sg[q].ord][c], ck[q][c]); atomicMax(&sExt[sg[q].ord][3 + c], ck[q][c]);
      }
    }
    __syncthreads();
    for (uint32_t q = 0; q < 2u; q++) {
      const uint32_t e = threadIdx.x + q * kTbThreads;
      if (e >= padded) continue;
      unsigned long long key = ~0ull;
      if (e < n) {
        uint32_t centreKey = 0u;                           // (a range of one leaf: its number keeps it in place)
        if (sg[q].hi - sg[q].lo >= 2u) {
          const uint32_t* x = sExt[sg[q].ord];
          const uint32_t kmin[3] = {x[0], x[1], x[2]}, kmax[3] = {x[3], x[4], x[5]};
          const int axis = tlasAxis(kmin, kmax);
          centreKey = axis == 0 ? ck[q][0] : axis == 1 ? ck[q][1] : ck[q][2];
        }
        key = tlasKey(sg[q].ord, centreKey, sId[e]);
      }
      sKey[e] = key;
    }
    __syncthreads();
    for (uint32_t k = 2u; k <= padded; k <<= 1) tbMergeSteps(sKey, 0u, k, k >> 1, padded >> 1);
    for (uint32_t e = threadIdx.x; e < n; e += kTbThreads) sId[e] = uint32_t(sKey[e]) & kTlasKeyNodeMask;
    __syncthreads();
  }
  for (uint32_t e = threadIdx.x; e < n; e += kTbThreads) a.ids[lo + e] = sId[e];
}

struct TbBoxArgs { TlasNode* tlas; const f4* nodeWorld; const uint32_t* ids; const uint32_t* recA; const uint32_t* order; uint32_t first, n; };
__global__ void __launch_bounds__(kBlock) k_tb_boxes(TbBoxArgs a) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.n) return;
  const uint32_t r = a.order[a.first + k], link = a.recA[r];
  TlasNode t;
  if (link & kTlasLeafMark) {
    t.a = a.ids[link & ~kTlasLeafMark]; t.b = 1u;
    const f4 lo = a.nodeWorld[size_t(t.a) * 2u], hi = a.nodeWorld[size_t(t.a) * 2u + 1u];
    t.lo[0] = lo.x; t.lo[1] = lo.y; t.lo[2] = lo.z; t.hi[0] = hi.x; t.hi[1] = hi.y; t.hi[2] = hi.z;
  } else {
    t.a = link; t.b = 0u;
    const TlasNode& l = a.tlas[link]; const TlasNode& rr = a.tlas[link + 1u];
    for (int c = 0; c < 3; c++) { t.lo[c] = stdmin(l.lo[c], rr.lo[c]); t.hi[c] = stdmax(l.hi[c], rr.hi[c]); }
  }
  a.tlas[r] = t;
}

uint32_t tbPadded(uint32_t leaves) {
  uint32_t p = kTbTile;
  while (p < leaves) p <<= 1;
  return p;
}

// The launches tbBuild makes for a tree of `leaves` leaves: per top level 2 and the merge stages above a tile — stage 2^q takes
// q - log2(tile) global steps and one local merge —, the subtrees' one, and one per level of the tree
uint32_t tbLaunchBound(uint32_t leaves) {
  if (!leaves) return 0u;
  uint32_t top = 0, height = 0, perLevel = 2u;
  while (tlasLargestRange(leaves, top) > kTlasLocalLeaves) top++;
  while (tlasLargestRange(leaves, height) > 1u) height++;
  for (uint32_t k = 2u * kTbTile, steps = 1u; k <= tbPadded(leaves); k <<= 1, steps++) perLevel += steps + 1u;
  return top * perLevel + 1u + height + 1u;
}

// The tables of a leaf list (its shape, the leaves' first order), uploaded with blocking copies, and the working arrays
void tbPrepare(TlasBuildState& b, const std::vector<uint32_t>& leafIds) {
  const uint32_t leaves = uint32_t(leafIds.size());
  if (b.ready && b.leafIds == leafIds) return;
  b.ready = false;
  b.shape = tlasShape(leaves);
  b.leafIds = leafIds;
  if (leaves) {
    std::vector<uint32_t> roots;
    for (size_t r = 0; r < b.shape.rootLo.size(); r++) { roots.push_back(b.shape.rootLo[r]); roots.push_back(b.shape.rootHi[r]); }
    b.dLeafIds.upload(leafIds); b.dRecA.upload(b.shape.recA); b.dOrder.upload(b.shape.order); b.dRoots.upload(roots);
    b.ids.ensure(leaves);
    if (b.shape.topLevels) {
      b.keys.ensure(tbPadded(leaves));
      b.ext.ensure(((size_t(1) << b.shape.topLevels) + 1u) * 6u);
    }
  }
  b.ready = true;
}

// The build on `stream` from the device's nodeWorld into `tlas` (shape.records() records); returns the launches made. No host work
// but the launches themselves: the tables are tbPrepare's.
uint32_t tbBuild(TlasBuildState& b, const f4* nodeWorld, TlasNode* tlas, hipStream_t stream) {
  const TlasShape& s = b.shape;
  if (!s.leaves) return 0u;
  uint32_t launches = 0;
  auto launched = [&] { HIP_CHECK(hipGetLastError()); launches++; };
  HIP_CHECK(hipMemcpyAsync(b.ids.p, b.dLeafIds.p, size_t(s.leaves) * 4u, hipMemcpyDeviceToDevice, stream));
  if (s.topLevels) {
    const uint32_t padded = tbPadded(s.leaves);
    HIP_CHECK(hipMemsetAsync(b.ext.p, 0xff, ((size_t(1) << s.topLevels) + 1u) * 6u * 4u, stream));
    for (uint32_t d = 0; d < s.topLevels; d++) {
      TbArgs a{nodeWorld, b.ids.p, b.keys.p, b.ext.p, s.leaves, d, (1u << d) - 1u};
      hipLaunchKernelGGL(k_tb_extent, dim3((s.leaves + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, a);
      launched();
      hipLaunchKernelGGL(k_tb_keys_sort, dim3(padded / kTbTile), dim3(kTbThreads), 0, stream, a);
      launched();
      for (uint32_t k = 2u * kTbTile; k <= padded; k <<= 1) {
        for (uint32_t j = k >> 1; j >= kTbTile; j >>= 1) {
          hipLaunchKernelGGL(k_tb_global_step, dim3((padded / 2u + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, b.keys.p, padded, k, j);
          launched();
        }
        hipLaunchKernelGGL(k_tb_local_merge, dim3(padded / kTbTile), dim3(kTbThreads), 0, stream, a, k, k == padded ? 1u : 0u);
        launched();
      }
    }
  }
  TbSubArgs sa{nodeWorld, b.ids.p, b.dRoots.p};
  hipLaunchKernelGGL(k_tb_subtree, dim3(uint32_t(s.rootLo.size())), dim3(kTbThreads), 0, stream, sa);
  launched();
  for (uint32_t l = s.height + 1u; l-- > 0u;) {
    TbBoxArgs ba{tlas, nodeWorld, b.ids.p, b.dRecA.p, b.dOrder.p, s.first[l], s.first[l + 1u] - s.first[l]};
    hipLaunchKernelGGL(k_tb_boxes, dim3((ba.n + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, ba);
    launched();
  }
  return launches;
}

void checkTlasBuildArgs(const float* node_world, const int32_t* mesh, uint32_t n_nodes, const void* tlas_out, const uint32_t* n_tlas_out,
                        const uint32_t* height_out) {
  require(node_world && mesh && tlas_out && n_tlas_out && height_out, "tlas build: null pointer");
  require(n_nodes < kTlasMaxNodes, "tlas build: n_nodes is 2^20 or more");
}

}  // namespace

extern "C" {

int yart_hip_tlas_build_device(int device, const float* node_world, const int32_t* mesh, uint32_t n_nodes, void* tlas_out, uint32_t* n_tlas_out,
                               uint32_t* height_out) {
  return guarded([&] {
    checkTlasBuildArgs(node_world, mesh, n_nodes, tlas_out, n_tlas_out, height_out);
    *n_tlas_out = 0u; *height_out = 0u;
    const std::vector<uint32_t> leafIds = tlasLeafIds(mesh, n_nodes);
    if (leafIds.empty()) return;
    const int dev = resolveDevice(device);
    if (dev < 0) throw HipError("no usable HIP device (libyart_hip has no CPU fallback)");
    HIP_CHECK(hipSetDevice(dev));
    TlasBuildState b;
    tbPrepare(b, leafIds);
    DevBuf<f4> world; DevBuf<TlasNode> tlas;
    world.ensure(size_t(n_nodes) * 2u); tlas.ensure(b.shape.records());
    HIP_CHECK(hipMemcpy(world.p, node_world, size_t(n_nodes) * 2u * sizeof(f4), hipMemcpyHostToDevice));
    const uint32_t launches = tbBuild(b, world.p, tlas.p, nullptr);
    HIP_CHECK(hipStreamSynchronize(nullptr));
    require(launches == tbLaunchBound(b.shape.leaves), "tlas build: the launch count differs from its formula");
    HIP_CHECK(hipMemcpy(tlas_out, tlas.p, size_t(b.shape.records()) * sizeof(TlasNode), hipMemcpyDeviceToHost));
    *n_tlas_out = b.shape.records(); *height_out = b.shape.height;
  });
}

int yart_hip_tlas_build_host(const float* node_world, const int32_t* mesh, uint32_t n_nodes, void* tlas_out, uint32_t* n_tlas_out, uint32_t* height_out) {
  return guarded([&] {
    checkTlasBuildArgs(node_world, mesh, n_nodes, tlas_out, n_tlas_out, height_out);
    std::vector<NodeDev> nodes(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) nodes[i].mesh = mesh[i];
    std::vector<f4> world(size_t(n_nodes) * 2u);
    if (n_nodes) std::memcpy(world.data(), node_world, world.size() * sizeof(f4));
    std::vector<TlasNode> tlas;
    *height_out = buildTopLevel(nodes, world, tlas);
    *n_tlas_out = uint32_t(tlas.size());
    if (!tlas.empty()) std::memcpy(tlas_out, tlas.data(), tlas.size() * sizeof(TlasNode));
  });
}

int yart_hip_tlas_build_launches(uint32_t n_leaves) { return int(tbLaunchBound(n_leaves)); }

}  // extern "C"
