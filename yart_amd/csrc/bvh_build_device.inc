// bvh_build_device.inc — the reference's binned-SAH BVH build (core/bvh.hpp:41-184, 273-347) on the device, with the
// node array and the index permutation of bvh_build.hpp byte for byte (included by yart_hip.hip, unit 0; SURVEY §8(f) rank 3).
//
// Why an exact device build is possible at all: every quantity the reference's recursion decides on is either an
// order-free fold (bounds are min / max folds, bin counts are integer sums) or a function of one node's index range, and
// the ranges of the nodes of one tree level are disjoint. So the top of the tree is built level by level, one workgroup per
// node, and every subtree of at most kLocalSpan triangles is then finished by one wave in a single launch (splitNode is the
// same code for both):
//
//   * centroid bounds, the 3 x 20 bins and their SAH sweep: the same float operations in the same order (the sweep
//     itself is 19 + 19 sequential steps per axis, done by one thread); bins accumulate through LDS atomics;
//   * the partition: the reference's loop `while (i <= j) if (c[idx[i]] < split) i++; else swap(idx[i], idx[j--]);` is
//     sequential, but its result has a closed form (below, partitionCode / partitionDest; checked against the loop on
//     200 000 random sequences before it was written down here): with m = number of "left" elements, the first m
//     positions keep their left elements and take the left elements of the back part, last first, into their holes; every
//     right element of the front part lands just below the back part's left element that was pulled for the hole before
//     it (the first one at the very end); right elements of the back part slide down by one while holes are still open;
//   * node bounds: a fold with `m < n ? m : n`, i.e. of equal values the LATER one survives — this only matters for the
//     sign of a zero, and is reproduced by reducing (value, position) pairs;
//   * node numbering: the reference allocates the children pair when the parent is split and finishes the left subtree
//     before the right one (bvh.hpp:163-183), so pair index = 1 + 2 x (rank of the parent among the inner nodes in
//     pre-order). For the top of the tree: subtree inner-node counts bottom-up, ranks top-down, over the levels; a wave
//     that finishes a small subtree splits its nodes in pre-order, so a node's rank is the subtree root's plus the number
//     of splits the wave had done before it.
//
// Input with NaN or infinite coordinates (or a non-finite centroid) is refused (the folds above are order-free only without
// NaNs, and inf + -inf makes them): the caller builds on the host.

namespace devbvh {

constexpr uint32_t kNoChild = 0xffffffffu;
constexpr uint32_t kBins = 20, kSplits = kBins - 1;
constexpr uint32_t kBigSpan = 2048;        // nodes of at least this many triangles get a 1024-thread workgroup, smaller ones a wave
#ifndef YART_DEVBVH_LOCAL_SPAN
#define YART_DEVBVH_LOCAL_SPAN 256
#endif
constexpr uint32_t kLocalSpan = YART_DEVBVH_LOCAL_SPAN;   // subtrees of at most this many triangles are finished by one wave (k_subtree)
constexpr uint32_t kLocalStack = 256;      // pending right children of such a wave (a subtree of s triangles is at most s - 1 deep)
constexpr int kMaxLevels = 192;
enum : uint32_t { NODE_RIGHT = 1u, NODE_LOCAL = 2u, NODE_LOCAL_ROOT = 4u };

struct BNode {                             // build node; ids: [0, n2) created by the level kernels, [n2, 2 n2) by k_subtree (n2 = 2 n)
  float bmin[3], bmax[3];
  uint32_t first, span;
  uint32_t left;                           // id of the left child (right = left + 1), kNoChild = leaf
  uint32_t parent;
  uint32_t info;                           // NODE_*
  uint32_t inner;                          // inner nodes in this subtree (level nodes and subtree roots)
  uint32_t rank;                           // pre-order rank among the inner nodes: of the whole tree (level nodes, subtree roots) ...
  uint32_t lrank;                          // ... within the subtree (nodes k_subtree created; 0 for its root)
  uint32_t root;                           // the subtree root (nodes k_subtree created)
};

struct Args {
  const float* pos; const uint32_t* tris; uint32_t stride, n;
  float* cent;                             // n x 3
  float* tb;                               // n x 6: triangle bounds (fromPoints + 0.001 padding)
  uint32_t *idx, *idxTmp, *code, *tmpR, *tmpL;
  BNode* nodes; uint32_t* counter;
  uint32_t* localRoots;                    // ids of the subtree roots (counter[4] of them)
  BvhNode* out;
};
// counter words: [0] level nodes created, [1] error (1 NaN seen, 2 internal), [2] nodes of at least kBigSpan triangles created by
// the current level, [3] nodes k_subtree created, [4] subtree roots

__device__ __forceinline__ uint32_t ordKey(float v) {          // order-preserving map float -> uint32, both zeros alike
  uint32_t b = __builtin_bit_cast(uint32_t, v == 0.0f ? 0.0f : v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordVal(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __builtin_bit_cast(float, b);
}
__device__ __forceinline__ uint32_t f2uX86(float x) {          // uint32_t(float) as x86-64 performs it (bvh_build.hpp::f2u_x86)
  if (x != x) return 0u;
  if (x >= 9.2e18f || x <= -9.2e18f) return 0u;
  return uint32_t(int64_t(x));
}

// primitives.hpp:41-46 (centroid) and bounds.hpp:89-104 (fromPoints) per triangle
__global__ void k_prepare(Args a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const float* v[3];
  for (int k = 0; k < 3; k++) v[k] = a.pos + size_t(a.tris[size_t(i) * a.stride + k]) * 3;
  bool nan = false;
  for (int c = 0; c < 3; c++) {
    a.cent[size_t(i) * 3 + c] = ((v[0][c] + v[1][c]) + v[2][c]) / 3.0f;
    float mn = kInf, mx = -kInf;
    for (int k = 0; k < 3; k++) {
      if (v[k][c] < mn) mn = v[k][c];
      if (v[k][c] > mx) mx = v[k][c];
      nan |= !(fabsf(v[k][c]) <= 3.4028234664e38f);        // NaN or infinite: inf + -inf centroids / bin bounds would be NaN
    }
    nan |= !(fabsf(a.cent[size_t(i) * 3 + c]) <= 3.4028234664e38f);
    a.tb[size_t(i) * 6 + c] = mn - 0.001f;
    a.tb[size_t(i) * 6 + 3 + c] = mx + 0.001f;
  }
  a.idx[i] = i;
  if (nan) a.counter[1] = 1u;
}

template <uint32_t BLOCK>
struct Lds {
  unsigned long long key[12];              // (value, position) keys: 6 per child, or 6 of one node
  uint32_t binCount[3][kBins];
  uint32_t binLo[3][kBins][3], binHi[3][kBins][3];
  uint32_t cbLo[3], cbHi[3];
  uint32_t waveSum[BLOCK / 64 + 1];
  uint32_t scalar[8];                      // [1] split?, [2] axis, [3] splitPos bits, [4] children, [5] result of splitNode
  unsigned long long sweepKey;             // sweepAndChoose: the minimum of (cost, lane)
  float sweepCost[64];
};

// exclusive count of `flag` over the workgroup in thread order, and the total
template <uint32_t BLOCK>
__device__ __forceinline__ uint32_t blockCount(Lds<BLOCK>& s, bool flag, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const uint32_t inWave = uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
  if (BLOCK == 64) { total = uint32_t(__popcll(m)); return inWave; }
  __syncthreads();
  if (lane == 0) s.waveSum[wave] = uint32_t(__popcll(m));
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < BLOCK / 64; w++) { const uint32_t c = s.waveSum[w]; if (w < wave) before += c; all += c; }
  total = all;
  return before + inWave;
}
template <uint32_t BLOCK>
__device__ __forceinline__ void blockSync() { __syncthreads(); }

// fold of the triangle bounds of positions [lo, hi) of `order` into key slots base .. base + 5 (reset by the caller):
// min components keep the smallest value and of equal values the LAST position, max components likewise
__device__ __forceinline__ unsigned long long waveMin64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ unsigned long long waveMax64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o); v = w > v ? w : v; }
  return v;
}
// (every thread folds its own elements, every wave its threads, and only the waves' results meet in LDS: one atomic per
// wave and component instead of one per triangle on the same six words)
template <uint32_t BLOCK>
__device__ __forceinline__ void foldBounds(Lds<BLOCK>& s, const Args& a, const uint32_t* order, uint32_t lo, uint32_t hi, uint32_t base) {
  unsigned long long kmin[3] = {~0ull, ~0ull, ~0ull}, kmax[3] = {0ull, 0ull, 0ull};
  for (uint32_t p = lo + threadIdx.x; p < hi; p += BLOCK) {
    const float* b = a.tb + size_t(order[p]) * 6;
    for (int c = 0; c < 3; c++) {
      const unsigned long long lo64 = ((unsigned long long) ordKey(b[c]) << 32) | (unsigned long long) (0xffffffffu - p);
      const unsigned long long hi64 = ((unsigned long long) ordKey(b[3 + c]) << 32) | (unsigned long long) p;
      kmin[c] = lo64 < kmin[c] ? lo64 : kmin[c];
      kmax[c] = hi64 > kmax[c] ? hi64 : kmax[c];
    }
  }
  for (int c = 0; c < 3; c++) {
    const unsigned long long mn = waveMin64(kmin[c]), mx = waveMax64(kmax[c]);
    if ((threadIdx.x & 63u) == 0u) { atomicMin(&s.key[base + c], mn); atomicMax(&s.key[base + 3 + c], mx); }
  }
}
// ... and the folded bounds: the winners' own values (a zero keeps its sign)
template <uint32_t BLOCK>
__device__ __forceinline__ void readBounds(const Lds<BLOCK>& s, const Args& a, const uint32_t* order, uint32_t base, BNode& nd) {
  for (int c = 0; c < 3; c++) {
    const uint32_t pl = 0xffffffffu - uint32_t(s.key[base + c]), ph = uint32_t(s.key[base + 3 + c]);
    nd.bmin[c] = a.tb[size_t(order[pl]) * 6 + c];
    nd.bmax[c] = a.tb[size_t(order[ph]) * 6 + 3 + c];
  }
}
__device__ __forceinline__ void resetKeys(unsigned long long* key) {
  for (int c = 0; c < 3; c++) { key[c] = ~0ull; key[3 + c] = 0ull; }
}

// bounds.hpp:38-41 on decoded bin bounds, and the join of bounds.hpp:48-59
struct B3 { float mn[3], mx[3]; };
__device__ __forceinline__ float areaOf(const B3& b) {
  const float sx = b.mx[0] - b.mn[0], sy = b.mx[1] - b.mn[1], sz = b.mx[2] - b.mn[2];
  return sx * sy + sy * sz + sz * sx;
}
__device__ __forceinline__ void joinInto(B3& t, const B3& b) {
  B3 u;
  for (int i = 0; i < 3; i++) { u.mn[i] = kInf; u.mx[i] = -kInf; }
  for (int i = 0; i < 3; i++) { u.mn[i] = ymin(u.mn[i], t.mn[i]); u.mx[i] = ymax(u.mx[i], t.mx[i]); }
  for (int i = 0; i < 3; i++) { u.mn[i] = ymin(u.mn[i], b.mn[i]); u.mx[i] = ymax(u.mx[i], b.mx[i]); }
  t = u;
}

// the root: bounds of all triangles (BVH::init -> updateBounds, bvh.hpp:41-67, 101-115)
__global__ void __launch_bounds__(1024) k_root(Args a) {
  __shared__ Lds<1024> s;
  if (threadIdx.x == 0) resetKeys(s.key);
  __syncthreads();
  foldBounds<1024>(s, a, a.idx, 0, a.n, 0);
  __syncthreads();
  if (threadIdx.x == 0) {
    BNode nd{};
    readBounds<1024>(s, a, a.idx, 0, nd);
    nd.first = 0; nd.span = a.n; nd.left = kNoChild; nd.parent = kNoChild;
    if (a.n <= kLocalSpan) { nd.info = NODE_LOCAL_ROOT; a.localRoots[0] = 0u; a.counter[4] = 1u; }
    a.nodes[0] = nd;
    a.counter[0] = 1;
  }
}

// one tree level: the nodes created by the previous one, one workgroup each (subdivide, bvh.hpp:140-184)
enum : uint32_t { CODE_FRONT_L = 0u << 30, CODE_FRONT_R = 1u << 30, CODE_BACK_L = 2u << 30, CODE_BACK_R = 3u << 30, CODE_MASK = 3u << 30 };
// The SAH sweep over the bins in LDS and the choice of the split (bvh.hpp:305-346), by the first wave of the workgroup:
// lane 19 a + i evaluates split i of axis a — the joins of the bins below and above it in the reference's order, then
// (0 + count_below * area_below) + count_above * area_above as the reference's two loops add them up. The reference's
// scan `if (costs[i] < minCost)` over axes and splits keeps the FIRST of equal minima and never a NaN or an infinite cost:
// the wave takes the minimum of (cost, lane) over the lanes whose cost is below infinity.
// s.scalar[1] = split?, [2] = axis, [3] = split position
template <uint32_t BLOCK>
__device__ __forceinline__ void sweepAndChoose(Lds<BLOCK>& s, const BNode& nd, const float* bmin, const float* bsize) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ax = lane < 3u * kSplits ? lane / kSplits : 0u, i = lane % kSplits;
  // (flat views of the bin arrays: bins of axis ax start at ax * kBins)
  const uint32_t* cnt = &s.binCount[0][0] + ax * kBins;
  const uint32_t* lo = &s.binLo[0][0][0] + ax * kBins * 3u;
  const uint32_t* hi = &s.binHi[0][0][0] + ax * kBins * 3u;
  uint32_t countBelow = 0, countAbove = 0;
  B3 below, above;
  for (int k = 0; k < 3; k++) { below.mn[k] = above.mn[k] = kInf; below.mx[k] = above.mx[k] = -kInf; }
  for (uint32_t j = 0; j < kBins; j++) {                // bins 0 .. i below the split, in rising order
    if (j <= i) {
      B3 b; for (int k = 0; k < 3; k++) { b.mn[k] = ordVal(lo[j * 3u + k]); b.mx[k] = ordVal(hi[j * 3u + k]); }
      joinInto(below, b); countBelow += cnt[j];
    }
  }
  for (uint32_t jj = 0; jj < kBins; jj++) {             // bins kSplits .. i + 1 above it, in falling order
    const uint32_t j = kSplits - jj;
    if (j > i) {
      B3 b; for (int k = 0; k < 3; k++) { b.mn[k] = ordVal(lo[j * 3u + k]); b.mx[k] = ordVal(hi[j * 3u + k]); }
      joinInto(above, b); countAbove += cnt[j];
    }
  }
  float cost = 0.0f;
  cost += float(countBelow) * areaOf(below);
  cost += float(countAbove) * areaOf(above);
  if (lane >= 3u * kSplits) cost = kInf;
  s.sweepCost[lane] = cost;
  atomicMin(&s.sweepKey, cost < kInf ? (((unsigned long long) ordKey(cost) << 32) | lane) : ~0ull);
}
// ... its second half, by one thread after a barrier
template <uint32_t BLOCK>
__device__ __forceinline__ void sweepDecide(Lds<BLOCK>& s, const BNode& nd, const float* bmin, const float* bsize) {
  const unsigned long long key = s.sweepKey;
  float minCost = kInf, splitPos = 0.0f;
  uint32_t axis = 0;
  if (key != ~0ull) {
    const uint32_t w = uint32_t(key);
    minCost = s.sweepCost[w];
    axis = w / kSplits;
    splitPos = bmin[axis] + bsize[axis] * (float(w % kSplits + 1u) / float(kBins));
  }
  B3 nb; for (int k = 0; k < 3; k++) { nb.mn[k] = nd.bmin[k]; nb.mx[k] = nd.bmax[k]; }
  const float leafCost = (float(nd.span) - 0.5f) * areaOf(nb);
  s.scalar[1] = (nd.span <= 20u && leafCost < minCost) ? 0u : 1u;     // MAX_LEAF_SIZE, bvh.hpp:14
  s.scalar[2] = axis;
  s.scalar[3] = __builtin_bit_cast(uint32_t, splitPos);
}

// One step of bvh.hpp:140-184 for node `id`, by the whole workgroup: choose the split, partition the index range, create and
// bound the two children. LOCAL: the children are k_subtree's (ids from counter[3], behind a.n * 2). Returns the left
// child's id, or kNoChild if the node stays a leaf. (Every thread returns the same value.)
template <uint32_t BLOCK, bool LOCAL>
__device__ __forceinline__ uint32_t splitNode(Lds<BLOCK>& s, const Args& a, uint32_t id, uint32_t rootId) {
  blockSync<BLOCK>();                                                  // (the previous node's LDS values have been read, its children written)
  const BNode nd = a.nodes[id];
  const uint32_t first = nd.first, span = nd.span, tid = threadIdx.x;

  // ---- getCentroidBounds (bvh.hpp:123-134)
  if (tid < 3) { s.cbLo[tid] = 0xffffffffu; s.cbHi[tid] = 0u; }
  if (tid == 3) s.sweepKey = ~0ull;
  for (uint32_t k = tid; k < 3 * kBins; k += BLOCK) {
    const uint32_t ax = k / kBins, b = k % kBins;
    s.binCount[ax][b] = 0;
    for (int c = 0; c < 3; c++) { s.binLo[ax][b][c] = ordKey(kInf); s.binHi[ax][b][c] = ordKey(-kInf); }
  }
  blockSync<BLOCK>();
  {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (uint32_t p = tid; p < span; p += BLOCK) {
      const float* c = a.cent + size_t(a.idx[first + p]) * 3;
      for (int ax = 0; ax < 3; ax++) { const uint32_t k = ordKey(c[ax]); lo[ax] = k < lo[ax] ? k : lo[ax]; hi[ax] = k > hi[ax] ? k : hi[ax]; }
    }
    for (int ax = 0; ax < 3; ax++) {
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t l2 = __shfl_xor(lo[ax], o), h2 = __shfl_xor(hi[ax], o);
        lo[ax] = l2 < lo[ax] ? l2 : lo[ax]; hi[ax] = h2 > hi[ax] ? h2 : hi[ax];
      }
      if ((tid & 63u) == 0u) { atomicMin(&s.cbLo[ax], lo[ax]); atomicMax(&s.cbHi[ax], hi[ax]); }
    }
  }
  blockSync<BLOCK>();
  // ---- the bins of the three axes (bvh.hpp:287-303)
  float bmin[3], bsize[3], scale[3];
  for (int ax = 0; ax < 3; ax++) {
    bmin[ax] = ordVal(s.cbLo[ax]);
    bsize[ax] = ordVal(s.cbHi[ax]) - bmin[ax];
    scale[ax] = float(kBins) / bsize[ax];
  }
  for (uint32_t p = tid; p < span; p += BLOCK) {
    const uint32_t t = a.idx[first + p];
    const float* c = a.cent + size_t(t) * 3;
    const float* tb = a.tb + size_t(t) * 6;
    for (int ax = 0; ax < 3; ax++) {
      uint32_t b = f2uX86(scale[ax] * (c[ax] - bmin[ax]));
      if (kBins - 1 < b) b = kBins - 1;
      atomicAdd(&s.binCount[ax][b], 1u);
      for (int k = 0; k < 3; k++) { atomicMin(&s.binLo[ax][b][k], ordKey(tb[k])); atomicMax(&s.binHi[ax][b][k], ordKey(tb[3 + k])); }
    }
  }
  blockSync<BLOCK>();
  // ---- the sweep and the choice (bvh.hpp:305-346), the first wave
  if (tid < 64u) sweepAndChoose<BLOCK>(s, nd, bmin, bsize);
  blockSync<BLOCK>();
  if (tid == 0) sweepDecide<BLOCK>(s, nd, bmin, bsize);
  blockSync<BLOCK>();
  if (s.scalar[1] == 0u) return kNoChild;                              // a leaf: its index range stays as it is
  const uint32_t axis = s.scalar[2];
  const float splitPos = __builtin_bit_cast(float, s.scalar[3]);

  // ---- the partition (bvh.hpp:150-160) in closed form; L = centroid < splitPos
  auto isLeft = [&](uint32_t p) { return a.cent[size_t(a.idx[first + p]) * 3 + axis] < splitPos; };
  uint32_t m = 0;
  for (uint32_t base = 0; base < span; base += BLOCK) {
    uint32_t tot;
    (void)blockCount<BLOCK>(s, base + tid < span && isLeft(base + tid), tot);
    m += tot;
  }
  // front part: positions [0, m), and position m too if it holds a right element (the loop examines it in place)
  const uint32_t frontEnd = (m < span && !isLeft(m)) ? m + 1 : m;
  uint32_t rFront = 0;
  for (uint32_t base = 0; base < frontEnd; base += BLOCK) {
    const uint32_t p = base + tid;
    const bool valid = p < frontEnd, right = valid && !isLeft(p);
    uint32_t tot;
    const uint32_t before = blockCount<BLOCK>(s, right, tot);
    if (valid) {
      if (right) { const uint32_t k = rFront + before + 1; a.tmpR[first + k - 1] = p; a.code[first + p] = CODE_FRONT_R | k; }
      else a.code[first + p] = CODE_FRONT_L;
    }
    rFront += tot;
  }
  // back part, from the end: rank of a left element among the back part's left elements, count of them above a right one
  uint32_t lBack = 0;
  for (uint32_t base = 0; base < span - frontEnd; base += BLOCK) {
    const uint32_t off = base + tid;
    const bool valid = off < span - frontEnd;
    const uint32_t q = valid ? span - 1 - off : 0u;
    const bool left = valid && isLeft(q);
    uint32_t tot;
    const uint32_t before = blockCount<BLOCK>(s, left, tot);
    if (valid) {
      if (left) { const uint32_t k = lBack + before + 1; a.tmpL[first + k - 1] = q; a.code[first + q] = CODE_BACK_L | k; }
      else a.code[first + q] = CODE_BACK_R | (lBack + before);
    }
    lBack += tot;
  }
  __threadfence_block();
  blockSync<BLOCK>();
  for (uint32_t p = tid; p < span; p += BLOCK) {
    const uint32_t c = a.code[first + p], kind = c & CODE_MASK, k = c & ~CODE_MASK;
    uint32_t dest = p;
    if (kind == CODE_FRONT_R) dest = k == 1u ? span - 1u : a.tmpL[first + k - 2] - 1u;
    else if (kind == CODE_BACK_L) dest = a.tmpR[first + k - 1];
    else if (kind == CODE_BACK_R) dest = k < rFront ? p - 1u : p;
    if (dest >= span) { a.counter[1] = 2u; dest = p; }                 // (cannot happen: the build is then refused, not trusted)
    a.idxTmp[first + dest] = a.idx[first + p];
  }
  __threadfence_block();
  blockSync<BLOCK>();
  for (uint32_t p = tid; p < span; p += BLOCK) a.idx[first + p] = a.idxTmp[first + p];
  if (m == 0u || m == span) return kNoChild;                           // bvh.hpp:162: stays a leaf (with the permuted range)
  __threadfence_block();
  blockSync<BLOCK>();

  // ---- the two children and their bounds (bvh.hpp:163-181)
  if (tid == 0) {
    resetKeys(s.key); resetKeys(s.key + 6);
    s.scalar[4] = LOCAL ? a.n * 2u + atomicAdd(a.counter + 3, 2u) : atomicAdd(a.counter, 2u);
  }
  blockSync<BLOCK>();
  foldBounds<BLOCK>(s, a, a.idx, first, first + m, 0);
  foldBounds<BLOCK>(s, a, a.idx, first + m, first + span, 6);
  blockSync<BLOCK>();
  const uint32_t c = s.scalar[4];
  if (tid == 0) {
    BNode l{}, r{};
    readBounds<BLOCK>(s, a, a.idx, 0, l);
    readBounds<BLOCK>(s, a, a.idx, 6, r);
    l.first = first; l.span = m; l.left = kNoChild; l.parent = id;
    r.first = first + m; r.span = span - m; r.left = kNoChild; r.parent = id; r.info = NODE_RIGHT;
    if (LOCAL) { l.info |= NODE_LOCAL; r.info |= NODE_LOCAL; l.root = r.root = rootId; }
    else {
      // small subtrees leave the level-by-level build here
      if (l.span <= kLocalSpan) { l.info |= NODE_LOCAL_ROOT; a.localRoots[atomicAdd(a.counter + 4, 1u)] = c; }
      if (r.span <= kLocalSpan) { r.info |= NODE_LOCAL_ROOT; a.localRoots[atomicAdd(a.counter + 4, 1u)] = c + 1u; }
      const uint32_t big = (l.span >= kBigSpan ? 1u : 0u) + (r.span >= kBigSpan ? 1u : 0u);
      if (big) atomicAdd(a.counter + 2, big);
    }
    a.nodes[c] = l; a.nodes[c + 1] = r;
    a.nodes[id].left = c;
  }
  return c;
}


// splitNode for nodes of at most kLocalSpan triangles, by one wave: every lane keeps its (up to kSmallPerLane) triangles'
// centroids and bounds in registers from one read, so that the passes below cost LDS traffic instead of dependent global
// gathers (a node of the generic form costs ~25 of them, ~140 us by a lone wave). Same decisions, same bytes.
constexpr uint32_t kSmallPerLane = (kLocalSpan + 63u) / 64u;
struct SmallLds {
  uint32_t tmpR[kLocalSpan], tmpL[kLocalSpan];
  float win[12];
};
template <bool LOCAL>
__device__ __forceinline__ uint32_t splitNodeSmall(Lds<64>& s, SmallLds& t, const Args& a, uint32_t id, uint32_t rootId) {
  __syncthreads();
  const BNode nd = a.nodes[id];
  const uint32_t first = nd.first, span = nd.span, lane = threadIdx.x;
  const unsigned long long laneLt = (1ull << lane) - 1ull, laneGt = ~laneLt & ~(1ull << lane);
  uint32_t tri[kSmallPerLane];
  float c[kSmallPerLane][3], b[kSmallPerLane][6];
  bool valid[kSmallPerLane];
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++) {
    const uint32_t p = lane + 64u * e;
    valid[e] = p < span;
    tri[e] = valid[e] ? a.idx[first + p] : 0u;
    for (int k = 0; k < 3; k++) c[e][k] = valid[e] ? a.cent[size_t(tri[e]) * 3 + k] : 0.0f;
    for (int k = 0; k < 6; k++) b[e][k] = valid[e] ? a.tb[size_t(tri[e]) * 6 + k] : 0.0f;
  }
  if (lane < 3) { s.cbLo[lane] = 0xffffffffu; s.cbHi[lane] = 0u; }
  if (lane == 3) s.sweepKey = ~0ull;
  for (uint32_t k = lane; k < 3 * kBins; k += 64u) {
    const uint32_t ax = k / kBins, bi = k % kBins;
    s.binCount[ax][bi] = 0;
    for (int q = 0; q < 3; q++) { s.binLo[ax][bi][q] = ordKey(kInf); s.binHi[ax][bi][q] = ordKey(-kInf); }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++)
    if (valid[e]) for (int ax = 0; ax < 3; ax++) { atomicMin(&s.cbLo[ax], ordKey(c[e][ax])); atomicMax(&s.cbHi[ax], ordKey(c[e][ax])); }
  __syncthreads();
  float bmin[3], bsize[3], scale[3];
  for (int ax = 0; ax < 3; ax++) {
    bmin[ax] = ordVal(s.cbLo[ax]);
    bsize[ax] = ordVal(s.cbHi[ax]) - bmin[ax];
    scale[ax] = float(kBins) / bsize[ax];
  }
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++)
    if (valid[e]) for (int ax = 0; ax < 3; ax++) {
      uint32_t bi = f2uX86(scale[ax] * (c[e][ax] - bmin[ax]));
      if (kBins - 1 < bi) bi = kBins - 1;
      atomicAdd(&s.binCount[ax][bi], 1u);
      for (int k = 0; k < 3; k++) { atomicMin(&s.binLo[ax][bi][k], ordKey(b[e][k])); atomicMax(&s.binHi[ax][bi][k], ordKey(b[e][3 + k])); }
    }
  __syncthreads();
  sweepAndChoose<64>(s, nd, bmin, bsize);
  __syncthreads();
  if (lane == 0) sweepDecide<64>(s, nd, bmin, bsize);
  __syncthreads();
  if (s.scalar[1] == 0u) return kNoChild;
  const uint32_t axis = s.scalar[2];
  const float splitPos = __builtin_bit_cast(float, s.scalar[3]);

  // the partition in closed form (see splitNode); positions run lane-fastest, chunk e = positions [64 e, 64 e + 64)
  bool left[kSmallPerLane];
  unsigned long long leftMask[kSmallPerLane];
  uint32_t m = 0;
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++) {
    const float cv = axis == 0u ? c[e][0] : (axis == 1u ? c[e][1] : c[e][2]);
    left[e] = valid[e] && cv < splitPos;
    leftMask[e] = __ballot(left[e]);
    m += uint32_t(__popcll(leftMask[e]));
  }
  // is position m a right element? (then the loop examines it in place: it belongs to the front part)
  bool mRight = false;
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++)
    if (m < span && (m >> 6) == e) mRight = !((leftMask[e] >> (m & 63u)) & 1ull);
  const uint32_t frontEnd = mRight ? m + 1u : m;
  uint32_t code[kSmallPerLane];
  uint32_t rFront = 0;
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++) {
    const uint32_t p = lane + 64u * e;
    const bool inFront = valid[e] && p < frontEnd, right = inFront && !left[e];
    const unsigned long long mask = __ballot(right);
    code[e] = CODE_FRONT_L;
    if (right) { const uint32_t k = rFront + uint32_t(__popcll(mask & laneLt)) + 1u; t.tmpR[k - 1u] = p; code[e] = CODE_FRONT_R | k; }
    rFront += uint32_t(__popcll(mask));
  }
  uint32_t lAbove = 0;                                  // left elements of the back part in the chunks above the current one
#pragma unroll
  for (uint32_t ee = 0; ee < kSmallPerLane; ee++) {
    const uint32_t e = kSmallPerLane - 1u - ee;
    const uint32_t p = lane + 64u * e;
    const bool inBack = valid[e] && p >= frontEnd, leftB = inBack && left[e];
    const unsigned long long mask = __ballot(leftB);
    const uint32_t above = lAbove + uint32_t(__popcll(mask & laneGt));
    if (inBack) {
      if (leftB) { t.tmpL[above] = p; code[e] = CODE_BACK_L | (above + 1u); }
      else code[e] = CODE_BACK_R | above;
    }
    lAbove += uint32_t(__popcll(mask));
  }
  __syncthreads();
  uint32_t dest[kSmallPerLane];
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++) {
    const uint32_t p = lane + 64u * e, kind = code[e] & CODE_MASK, k = code[e] & ~CODE_MASK;
    uint32_t d = p;
    if (kind == CODE_FRONT_R) d = k == 1u ? span - 1u : t.tmpL[k - 2u] - 1u;
    else if (kind == CODE_BACK_L) d = t.tmpR[k - 1u];
    else if (kind == CODE_BACK_R) d = k < rFront ? p - 1u : p;
    if (valid[e] && d >= span) { a.counter[1] = 2u; d = p; }
    dest[e] = d;
    if (valid[e]) a.idx[first + d] = tri[e];              // (every lane read its old entries above)
  }
  if (m == 0u || m == span) return kNoChild;
  if (lane == 0) {
    resetKeys(s.key); resetKeys(s.key + 6);
    s.scalar[4] = LOCAL ? a.n * 2u + atomicAdd(a.counter + 3, 2u) : atomicAdd(a.counter, 2u);
  }
  __syncthreads();
  // children bounds: (value, new position) keys, then every winner publishes its own value
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++)
    if (valid[e]) {
      const uint32_t base = dest[e] < m ? 0u : 6u;
      for (int k = 0; k < 3; k++) {
        atomicMin(&s.key[base + k], ((unsigned long long) ordKey(b[e][k]) << 32) | (unsigned long long) (0xffffffffu - dest[e]));
        atomicMax(&s.key[base + 3 + k], ((unsigned long long) ordKey(b[e][3 + k]) << 32) | (unsigned long long) dest[e]);
      }
    }
  __syncthreads();
#pragma unroll
  for (uint32_t e = 0; e < kSmallPerLane; e++)
    if (valid[e]) {
      const uint32_t base = dest[e] < m ? 0u : 6u;
      for (int k = 0; k < 3; k++) {
        if (uint32_t(s.key[base + k]) == 0xffffffffu - dest[e]) t.win[base + k] = b[e][k];
        if (uint32_t(s.key[base + 3 + k]) == dest[e]) t.win[base + 3 + k] = b[e][3 + k];
      }
    }
  __syncthreads();
  const uint32_t cid = s.scalar[4];
  if (lane == 0) {
    BNode l{}, r{};
    for (int k = 0; k < 3; k++) { l.bmin[k] = t.win[k]; l.bmax[k] = t.win[3 + k]; r.bmin[k] = t.win[6 + k]; r.bmax[k] = t.win[9 + k]; }
    l.first = first; l.span = m; l.left = kNoChild; l.parent = id;
    r.first = first + m; r.span = span - m; r.left = kNoChild; r.parent = id; r.info = NODE_RIGHT;
    if (LOCAL) { l.info |= NODE_LOCAL; r.info |= NODE_LOCAL; l.root = r.root = rootId; }
    else {
      l.info |= NODE_LOCAL_ROOT; a.localRoots[atomicAdd(a.counter + 4, 1u)] = cid;          // (both at most kLocalSpan triangles)
      r.info |= NODE_LOCAL_ROOT; a.localRoots[atomicAdd(a.counter + 4, 1u)] = cid + 1u;
    }
    a.nodes[cid] = l; a.nodes[cid + 1] = r;
    a.nodes[id].left = cid;
  }
  return cid;
}

// one tree level: the nodes created by the previous one, one workgroup each; nodes of at most kLocalSpan triangles wait for k_subtree
template <uint32_t BLOCK>
__global__ void __launch_bounds__(BLOCK) k_level(Args a, uint32_t levelStart) {
  __shared__ Lds<BLOCK> s;
  const uint32_t id = levelStart + blockIdx.x;
  const uint32_t span = a.nodes[id].span;
  if ((span >= kBigSpan) != (BLOCK != 64) || (a.nodes[id].info & NODE_LOCAL_ROOT)) return;
  (void)splitNode<BLOCK, false>(s, a, id, 0u);
}

// a subtree of at most kLocalSpan triangles, finished by one wave: the reference's recursion with an explicit stack —
// split, go on with the left child, come back for the right one — so the wave splits its nodes in pre-order
#if defined(YART_EXP_SLP)
__attribute__((optnone, noinline))        // (experiment builds with the SLP vectoriser on: it crashes this compiler's instruction selection here)
#endif
__global__ void __launch_bounds__(64) k_subtree(Args a) {
  __shared__ Lds<64> s;
  __shared__ SmallLds t;
  __shared__ uint32_t stack[kLocalStack];
  const uint32_t rootId = a.localRoots[blockIdx.x];
  uint32_t cur = rootId, sp = 0, splits = 0;
  for (;;) {
    const uint32_t left = splitNodeSmall<true>(s, t, a, cur, rootId);
    if (left != kNoChild) {
      if (threadIdx.x == 0) { a.nodes[cur].lrank = splits; if (sp < kLocalStack) stack[sp] = left + 1u; else a.counter[1] = 2u; }
      splits++;
      sp = sp < kLocalStack ? sp + 1u : sp;
      cur = left;
      __threadfence_block();
    } else {
      if (sp == 0u) break;
      __syncthreads();
      cur = stack[--sp];
    }
  }
  if (threadIdx.x == 0) a.nodes[rootId].inner = splits;
}

// numbering of the level nodes, bottom-up: inner nodes per subtree (the subtree roots bring theirs from k_subtree)
__global__ void k_count_inner(Args a, uint32_t levelStart, uint32_t levelCount) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= levelCount) return;
  BNode& nd = a.nodes[levelStart + i];
  if (nd.info & NODE_LOCAL_ROOT) return;
  nd.inner = nd.left == kNoChild ? 0u : 1u + a.nodes[nd.left].inner + a.nodes[nd.left + 1].inner;
}
// ... top-down: pre-order rank among the inner nodes
__global__ void k_number(Args a, uint32_t levelStart, uint32_t levelCount) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= levelCount) return;
  const uint32_t id = levelStart + i;
  BNode& nd = a.nodes[id];
  if (id == 0) nd.rank = 0;
  if (nd.left == kNoChild || (nd.info & NODE_LOCAL_ROOT)) return;
  BNode& l = a.nodes[nd.left];
  BNode& r = a.nodes[nd.left + 1];
  l.rank = nd.rank + 1u;
  r.rank = nd.rank + 1u + l.inner;
}
// the reference's node array: the children pair of an inner node of rank k stands at 1 + 2 k
__device__ __forceinline__ uint32_t globalRank(const Args& a, const BNode& nd) {
  return (nd.info & NODE_LOCAL) ? a.nodes[nd.root].rank + nd.lrank : nd.rank + ((nd.info & NODE_LOCAL_ROOT) ? nd.lrank : 0u);
}
__global__ void k_emit(Args a, uint32_t base, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const BNode nd = a.nodes[base + i];
  BvhNode o;
  for (int c = 0; c < 3; c++) { o.bmin[c] = nd.bmin[c]; o.bmax[c] = nd.bmax[c]; }
  if (nd.left == kNoChild) { o.leftFirst = nd.first; o.span = nd.span; }
  else { o.leftFirst = 1u + 2u * globalRank(a, nd); o.span = 0; }
  const uint32_t at = nd.parent == kNoChild ? 0u : 1u + 2u * globalRank(a, a.nodes[nd.parent]) + (nd.info & NODE_RIGHT ? 1u : 0u);
  a.out[at] = o;
}

// The build's working arrays, sized by the triangle count and grown on demand: a caller that builds again and again (a scene
// whose meshes deform, mesh_update_kernels.inc) keeps one of these and allocates nothing per build.
struct Scratch {
  DevBuf<float> cent, tb;
  DevBuf<uint32_t> idxTmp, code, tmpR, tmpL, counter, localRoots;
  DevBuf<BNode> nodes;
  void ensure(uint32_t nTris) {
    cent.ensure(size_t(nTris) * 3); tb.ensure(size_t(nTris) * 6);
    idxTmp.ensure(nTris); code.ensure(nTris); tmpR.ensure(nTris); tmpL.ensure(nTris); counter.ensure(8);
    nodes.ensure(size_t(nTris) * 4); localRoots.ensure(size_t(nTris) + 1);
  }
};
// What a build leaves on the device besides the node array and the permutation: the build nodes (ids [0, created) from the level
// kernels, [2 nTris, 2 nTris + createdLocal) from k_subtree) with their index ranges and parent links, for passes over the tree.
struct Built {
  Args args{};
  uint32_t created = 0, createdLocal = 0;
  uint32_t launches = 0;
  uint32_t nNodes() const { return created + createdLocal; }
};

// The build proper, on device arrays and a stream: `positions` (3 floats per vertex) and `tris` (`stride` words per triangle, the
// first three its vertices) are read; `out` (room for 2 nTris nodes) takes the reference's node array, `idx` (nTris) the index
// permutation. Returns false (`out` / `idx` hold nothing of use) if the input has NaN coordinates or the tree is deeper than
// kMaxLevels. The counters of every level are read back: `stream` is synchronised that often. ms: device time, if asked for.
inline bool buildCore(Scratch& sc, const float* positions, const uint32_t* tris, uint32_t stride, uint32_t nTris, BvhNode* out, uint32_t* idx,
                      hipStream_t stream, Built& built, double* ms) {
  require(nTris >= 1 && stride >= 3, "bvh build: empty mesh");
  sc.ensure(nTris);
  HIP_CHECK(hipMemsetAsync(sc.counter.p, 0, 32, stream));
  Args a{};
  a.pos = positions; a.tris = tris; a.stride = stride; a.n = nTris; a.cent = sc.cent.p; a.tb = sc.tb.p;
  a.idx = idx; a.idxTmp = sc.idxTmp.p; a.code = sc.code.p; a.tmpR = sc.tmpR.p; a.tmpL = sc.tmpL.p;
  a.nodes = sc.nodes.p; a.counter = sc.counter.p; a.out = out; a.localRoots = sc.localRoots.p;
  built = Built{};
  built.args = a;
  struct Events {                           // (destroyed on every way out)
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  } ev;
  if (ms) { HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); HIP_CHECK(hipEventRecord(ev.a, stream)); }
  auto readCounters = [&](uint32_t* c, uint32_t words) {
    HIP_CHECK(hipMemcpyAsync(c, sc.counter.p, size_t(words) * 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  };
  hipLaunchKernelGGL(k_prepare, dim3((nTris + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_root, dim3(1), dim3(1024), 0, stream, a);
  HIP_CHECK(hipGetLastError());
  built.launches += 2;
  const bool trace = std::getenv("YART_DEVBVH_TRACE") != nullptr;     // phase times on stderr (hipDeviceSynchronize between phases)
  auto lap = [&, last = std::chrono::steady_clock::now()](const char* what) mutable {
    if (!trace) return;
    (void)hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "devbvh %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  };
  lap("prepare + root");
  std::vector<uint32_t> levelStart(1, 0u);
  uint32_t created = 1;
  bool ok = true, anyBig = nTris >= kBigSpan;
  for (uint32_t start = 0; start < created;) {
    if (int(levelStart.size()) > kMaxLevels) { ok = false; break; }
    const uint32_t count = created - start;
    HIP_CHECK(hipMemsetAsync(sc.counter.p + 2, 0, 4, stream));
    if (anyBig) { hipLaunchKernelGGL(k_level<1024>, dim3(count), dim3(1024), 0, stream, a, start); built.launches++; }
    hipLaunchKernelGGL(k_level<64>, dim3(count), dim3(64), 0, stream, a, start);
    HIP_CHECK(hipGetLastError());
    built.launches++;
    uint32_t c[3];
    readCounters(c, 3);
    if (c[1]) { ok = false; break; }
    anyBig = c[2] != 0;
    if (trace) std::fprintf(stderr, "devbvh level %2zu: %u nodes (big: %d) ", levelStart.size() - 1, count, int(anyBig));
    lap("");
    start = created; created = c[0];
    if (created > start) levelStart.push_back(start);
  }
  uint32_t createdLocal = 0;
  if (ok) {
    uint32_t c[5];
    readCounters(c, 5);
    if (c[4]) { hipLaunchKernelGGL(k_subtree, dim3(c[4]), dim3(64), 0, stream, a); built.launches++; }
    if (trace) std::fprintf(stderr, "devbvh %u subtrees ", c[4]);
    lap("subtrees");
    for (size_t l = levelStart.size(); l-- > 0;) {
      const uint32_t s0 = levelStart[l], cnt = (l + 1 < levelStart.size() ? levelStart[l + 1] : created) - s0;
      hipLaunchKernelGGL(k_count_inner, dim3((cnt + 255) / 256), dim3(256), 0, stream, a, s0, cnt);
    }
    for (size_t l = 0; l < levelStart.size(); l++) {
      const uint32_t s0 = levelStart[l], cnt = (l + 1 < levelStart.size() ? levelStart[l + 1] : created) - s0;
      hipLaunchKernelGGL(k_number, dim3((cnt + 255) / 256), dim3(256), 0, stream, a, s0, cnt);
    }
    HIP_CHECK(hipGetLastError());
    built.launches += 2u * uint32_t(levelStart.size());
    readCounters(c, 5);
    if (c[1]) ok = false;
    createdLocal = c[3];
    if (ok) {
      hipLaunchKernelGGL(k_emit, dim3((created + 255) / 256), dim3(256), 0, stream, a, 0u, created);
      if (createdLocal) hipLaunchKernelGGL(k_emit, dim3((createdLocal + 255) / 256), dim3(256), 0, stream, a, nTris * 2u, createdLocal);
      HIP_CHECK(hipGetLastError());
      built.launches += createdLocal ? 2u : 1u;
    }
  }
  lap("numbering + emit");
  if (ms) {
    HIP_CHECK(hipEventRecord(ev.b, stream));
    HIP_CHECK(hipEventSynchronize(ev.b));
    float t = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
    *ms = t;
  }
  built.created = created; built.createdLocal = createdLocal;
  return ok;
}

// Builds the BVH of one mesh on `device`. Returns false (nothing written) if the input has NaN coordinates or the tree is
// deeper than kMaxLevels: the caller then builds on the host. ms: device time of the build, upload and download excluded.
inline bool build(int device, const float* positions, uint32_t nVerts, const uint32_t* tris, uint32_t stride, uint32_t nTris,
                  std::vector<BvhNode>& nodesOut, std::vector<uint32_t>& indicesOut, double* ms) {
  require(nTris >= 1 && nVerts >= 1 && stride >= 3, "bvh build: empty mesh");
  HIP_CHECK(hipSetDevice(device));
  DevBuf<float> pos;
  DevBuf<uint32_t> tri, idx;
  DevBuf<BvhNode> out;
  Scratch sc;
  pos.ensure(size_t(nVerts) * 3); tri.ensure(size_t(nTris) * stride);
  HIP_CHECK(hipMemcpy(pos.p, positions, size_t(nVerts) * 12, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(tri.p, tris, size_t(nTris) * stride * 4, hipMemcpyHostToDevice));
  idx.ensure(nTris); out.ensure(size_t(nTris) * 2);
  Built b;
  double t = 0.0;
  const bool ok = buildCore(sc, pos.p, tri.p, stride, nTris, out.p, idx.p, nullptr, b, &t);   // (the event pair also waits for the last launch)
  if (ms) *ms = t;
  if (!ok) return false;
  nodesOut.resize(b.nNodes()); indicesOut.resize(nTris);
  HIP_CHECK(hipMemcpy(nodesOut.data(), out.p, nodesOut.size() * sizeof(BvhNode), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(indicesOut.data(), idx.p, size_t(nTris) * 4, hipMemcpyDeviceToHost));
  return true;
}

}  // namespace devbvh
