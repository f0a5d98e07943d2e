// wavefront_kernels.inc — persistent-thread wavefront pipeline: what its kernels share, and the path kernels.
// Included inside the anonymous namespace by every unit: by wavefront_units.hip (units 1-4), which instantiates the kernel
// templates below, and by yart_hip.hip (unit 0), which needs WfArgs, WfDyn, WfCounter, the constants and the queue helpers for
// the host side and for stream_kernels.inc and aov_kernels.inc, and instantiates none of the templates. Nothing here is a
// non-template kernel: one would be emitted in all five units.
//
// One batch = up to kWfMaxPaths (pixel, sample) paths whose state lives in HBM
// (wavefront.hpp::WfState). Per bounce:
//
//   k_wf_extend_lean   closest-hit traversal of the `active` queue, lean variant (the roofline
//                      kernel): no alpha / transparency code, identity-only if the scene allows;
//                      paths that meet such a triangle go to the `retry` queue
//   k_wf_extend_retry_lean  general closest-hit traversal of the `retry` queue
//   k_wf_shade         miss / BSDF / NEE set-up / roulette — tentative for a path with a shadow ray (wavefront.hpp:
//                      WF_RR_PENDING) —; survivors -> `next`, shadow rays -> `shadow`
//   k_wf_shadow_lean   any-hit traversal of the `shadow` queue, lean variant; the NEE contribution is added to the
//                      path's radiance where the result is committed (wfShadowCommit)
//   k_wf_shadow_retry_lean  general any-hit traversal of the shadow `retry` queue; draws a pending roulette again at the
//                      walk's final sampler dimension and repairs a decision that flipped (wfShadowCommitGeneral)
// (k_wf_extend_fast / k_wf_extend / k_wf_shadow_fast / k_wf_shadow: the one-ray-per-lane forms of the same stages.)
// and, between these, the streaming passes of stream_kernels.inc (unit 0): k_wf_generate before the first bounce,
// k_wf_reset_retry after a retry pass, k_wf_advance and k_wf_compact / k_wf_compact_commit after the shadow stage;
// k_wf_refill, k_wf_roulette, k_wf_pool_init and k_wf_pool_advance in the path pool; k_sampler_tables once per render.
//
// Round 2 had a pass (k_wf_post) between the shadow traversal and the next bounce for the NEE contribution and the
// roulette: 46 ms and 205 GB per C3 frame. The contribution is now added by the lanes of the shadow kernels — VALU-bound
// kernels that leave the memory system idle — when they commit a ray's result, together for all lanes that finished since
// the last refill. What was left for a pass, the roulette from depth 2 on (k_wf_roulette: 22.7 ms of a 795 ms step in 12 launches),
// is decided in k_wf_shade since; only the path pool still runs the pass.
//
// The traversal kernels are persistent grids: a wave takes its first 64 queue entries by wave
// index and further ones from an atomic cursor, and exits when the cursor passes the queue
// length (a condition every wave reaches). Queue appends are staged per wave in LDS.

constexpr int kWfLdsStack = 16;                      // traversal stack entries per lane in LDS (general kernels)
#ifndef YART_LEAN_LDS_STACK
#define YART_LEAN_LDS_STACK 8     // 8 entries: 16 KB of stack + 2 KB of retry stage + 4 KB of scene records per block, 7 blocks per CU (10 / 9 / 8 entries measure the same)
#endif
// 7 waves / SIMD (72 VGPRs): with the SLP vectoriser off the lean kernels fit them without spilling into their loops —
// 1080p x 64 spp: extend 96.9 -> 95.8 ms, shadow 83.4 -> 80.7 ms against 6 waves (80 VGPRs, 12 stack entries); 8 waves (64 VGPRs,
// 8 entries): 99.1 / 81.2. (With the vectoriser on, 7 waves had lost: 98.8 -> 102.8 / 83.9 -> 86.0.)
#ifndef YART_LEAN_WAVES
#define YART_LEAN_WAVES 7
#endif
constexpr int leanWaves(int) { return YART_LEAN_WAVES; }
constexpr int kWfLdsStackFast = YART_LEAN_LDS_STACK;  // lean kernels: 16 KB / block, 7 blocks per CU
constexpr int kWfSpillDepth = int(kRefStackDepth) - kWfLdsStack;
#ifndef YART_WF_MAX_PATHS_LOG2
#define YART_WF_MAX_PATHS_LOG2 30
#endif
constexpr uint32_t kWfMaxPaths = 1u << YART_WF_MAX_PATHS_LOG2;   // at most 1 Gi paths per batch; the batch is sized by free memory (renderToDevice)

// Path-state compaction (k_wf_compact): from the third bounce on few paths are alive (C3: 26 %, 11 %, 5 % ...
// of the batch) and every 16-B field of a survivor drags a 64-B sector through the memory system. Between two
// bounces the survivors' live fields are copied, in queue order, into a smaller "tail" state whose slots are then
// 0..count-1, so that the kernels of the following bounces read and write dense arrays again. Which state is
// current is decided on the device (the host never reads the queue length): the kernels take it from WfDyn.
struct WfDyn {
  WfState st;              // current path state
  uint32_t* slotMap;       // slot of the current state -> slot of the batch (index of L), nullptr = identity
  uint32_t extent;         // number of slots of the current state that may hold a live path
  uint32_t inTail;         // 0: the batch-sized state, 1 / 2: tail buffer 0 / 1
};
struct WfArgs {
  SceneDev sc;
  CameraDev cam;
  RenderConst rc;
  WfDyn* dyn;              // nullptr: st below is used as is (no compaction)
  uint32_t* slotMap;       // set from dyn at kernel entry (WF_DYN)
  WfState tail[2];         // destination states of k_wf_compact
  uint32_t* tailMap[2];
  uint32_t tailCap[2];
  WfState st;
  uint32_t* qA;            // active
  uint32_t* qB;            // next
  uint32_t* qS;            // shadow
  uint32_t* qR;            // retry (paths the lean traversal kernels handed to the general ones)
  uint32_t* counters;      // WfCounter
  const uint32_t* pixels;
  uint32_t nPaths, spp, sampleOffset, pixBase;   // pixBase: index of pixels[0] in the rank's pixel list
  uint32_t bounce;                                // bounces the paths of this launch have behind them (uniform: their depth)
  f4* L;                       // per (pixel, sample) of the batch: radiance.xyz, ray count
  unsigned long long* stats;   // [0] rays
  uint64_t* spill;
  f4* resumeRec;               // resume records of the rays the lean kernels hand over (traverse.hpp), nullptr: restarts only
  uint32_t resumeCap, padR;
  const uint8_t* matClass;     // lobe class per material (host_scene.hpp::lobeClass): the bucket key of k_wf_shade<true>
  // Path pool (poolSlots != 0): the state arrays hold poolSlots paths, not the batch; slotMap[slot] is the path (index of L) a
  // slot carries, kWfFreeSlot when its path has ended; every round k_wf_refill starts the batch's next paths in the free slots.
  uint32_t poolSlots, padP;
};

enum WfCounter : uint32_t {   // words of WfArgs::counters
  WC_ACTIVE = 0, WC_NEXT = 1, WC_SHADOW = 2, WC_CUR_EXTEND = 3, WC_CUR_SHADE = 4, WC_CUR_SHADOW = 5,
  WC_RETRY = 6, WC_CUR_RETRY = 7,
  WC_RESUME = 8,               // resume records handed out (in ranges of 64)
  WC_STARTED = 9,              // path pool: paths of the batch started so far (may overshoot WfArgs::nPaths; kept across rounds)
  WC_DUMMY = 10,               // entries of `next` whose path a general shadow kernel has written out since (WF_DEAD): not paths of the next bounce
  WC_COUNT = 11
};

// A workgroup whose waves would find nothing in their first round of the queue — entries are dealt by wave index first, `per` per
// workgroup, and a wave that gets none of those never takes any — returns before it copies tables into LDS: the launches of the
// late bounces (and of small batches, and of one rank of eight) hold a few thousand entries for a grid of a few thousand
// workgroups, and were paying every workgroup's start-up (profiles/r3_shard_trace.txt: launches of 0.03 ms of work took 0.2 ms).
#define WF_EMPTY_BLOCK(count, per) do { if (uint64_t(blockIdx.x) * uint64_t(per) >= uint64_t(count)) return; } while (0)
// every path-state kernel starts with this: the current state and slot map (uniform scalar loads)
#define WF_DYN(a) do { if ((a).dyn) { (a).st = (a).dyn->st; (a).slotMap = (a).dyn->slotMap; } } while (0)

// wave-compacted append of `slot` to queue q (counter word c) for lanes with pred == true
__device__ __forceinline__ void wfPush(uint32_t* q, uint32_t* counter, bool pred, uint32_t slot) {
  const unsigned long long m = __ballot(pred);
  if (m == 0) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int leader = __ffsll((long long) m) - 1;
  uint32_t base = 0;
  if (int(lane) == leader) base = atomicAdd(counter, uint32_t(__popcll(m)));
  base = __shfl(base, leader);
  if (pred) q[base + __popcll(m & ((1ull << lane) - 1ull))] = slot;
}

// Per-wave staging of queue appends in LDS: one atomicAdd on the queue counter per ~7 wave
// iterations instead of one per iteration (a single L2 word takes only ~90 atomics/us, which
// otherwise bounds the light kernels). `n` is wave-uniform.
constexpr uint32_t kStageCap = 512;
template <uint32_t CAP>
struct WaveStageT {
  uint32_t* buf;           // CAP words of LDS owned by this wave
  uint32_t n;
  __device__ __forceinline__ void flush(uint32_t* q, uint32_t* counter) {
    if (n == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, n);
    base = __shfl(base, 0);
    for (uint32_t i = lane; i < n; i += 64u) q[base + i] = buf[i];
    n = 0;
  }
  __device__ __forceinline__ void push(uint32_t* q, uint32_t* counter, bool pred, uint32_t slot) {
    const unsigned long long m = __ballot(pred);
    if (m == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    if (pred) buf[n + __popcll(m & ((1ull << lane) - 1ull))] = slot;
    n += uint32_t(__popcll(m));
    if (n > CAP - 64u) flush(q, counter);
  }
};
typedef WaveStageT<kStageCap> WaveStage;
// copy `words` 32-bit words into LDS with the whole workgroup (no barrier)
__device__ __forceinline__ void ldsCopyWords(uint32_t* dst, const void* src, uint32_t words) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) dst[k] = s[k];
}
// The lean kernels' scene walk reads three small tables per step (scene node, its padded world box, its mesh record): with at most
// kLeanSceneNodes nodes and meshes they come from a copy in LDS (generic pointers: larger scenes keep them in memory).
// (1080p x 64 spp: extend lean 67.5 -> 65.4 ms, shadow lean 70.3 -> 66.8: profiles/r3_ab_shade_lds.txt)
// the sampler's small tables (hashDim values; with `sobol` the byte-wise XOR tables of the Sobol' matrix too) from a copy in LDS
struct SamplerLds { uint64_t hash[264]; uint32_t sobol1[8 * 256]; };
__device__ __forceinline__ void samplerToLds(SamplerConfig& c, SamplerLds& l, bool sobol) {
  if (c.tab.hash == nullptr || c.tab.dims + 3u > 264u) return;              // (uniform)
  for (uint32_t k = threadIdx.x; k < c.tab.dims + 3u; k += blockDim.x) l.hash[k] = c.tab.hash[k];
  if (sobol) for (uint32_t k = threadIdx.x; k < 8u * 256u; k += blockDim.x) l.sobol1[k] = c.tab.sobol1[k];
  __syncthreads();
  c.tab.hash = l.hash;
  if (sobol) c.tab.sobol1 = l.sobol1;
}
constexpr uint32_t kLeanSceneNodes = 16;
struct LeanSceneLds { uint32_t node[kLeanSceneNodes * sizeof(NodeDev) / 4], world[kLeanSceneNodes * 8], mesh[kLeanSceneNodes * sizeof(MeshDev) / 4]; };
// (NODES == kNodesMaskLds: the host has checked that the scene fits — the copies' being in LDS is then known at compile time: ds_read with constant
// addresses instead of flat loads through pointers that might be either; extend lean 65.7 -> 62.0 ms, shadow lean 67.0 -> 63.7)
__device__ __forceinline__ void leanSceneToLds(SceneDev& sc, LeanSceneLds& l, uint32_t nMeshes) {
  ldsCopyWords(l.node, sc.nodes, sc.nNodes * uint32_t(sizeof(NodeDev) / 4));
  ldsCopyWords(l.world, sc.nodeWorld, sc.nNodes * 8u);
  ldsCopyWords(l.mesh, sc.meshes, nMeshes * uint32_t(sizeof(MeshDev) / 4));
  __syncthreads();
  sc.nodes = reinterpret_cast<const NodeDev*>(l.node); sc.nodeWorld = reinterpret_cast<const f4*>(l.world);
  sc.meshes = reinterpret_cast<const MeshDev*>(l.mesh);
}
// What the general shadow kernels do when they reverse a roulette decision of k_wf_shade (wavefront.hpp: wfShadowCommitGeneral):
// rare — a few per thousand shadow rays —, and from divergent code, one lane at a time, so neither a queue append per event (a word
// takes ~90 atomics per microsecond; a 1080p x 256 spp frame has about a million events) nor WaveStageT's ballots fit. A wave
// collects the paths it revives in LDS (count: an LDS atomic) and appends them to `next` when it is done; what does not fit goes
// to the queue directly; the paths it retires are counted per lane and added up once.
constexpr uint32_t kRepairCap = 32;       // (528 B per workgroup: the general kernels keep their 4 workgroups per CU)
struct WfRepairLds { uint32_t slots[kBlock / 64][kRepairCap]; uint32_t n[kBlock / 64]; };
struct WfRepair {
  uint32_t* slots; uint32_t* n;       // this wave's row and count in LDS
  uint32_t* qNext; uint32_t* counters;
  uint32_t dummies;
  __device__ __forceinline__ WfRepair(WfRepairLds& l, uint32_t* q, uint32_t* c) : slots(l.slots[threadIdx.x >> 6]), n(&l.n[threadIdx.x >> 6]), qNext(q), counters(c), dummies(0) {
    if ((threadIdx.x & 63u) == 0) *n = 0;                  // (same wave, program order: no barrier needed before the first use)
  }
  __device__ __forceinline__ void revived(uint32_t slot) {
    const uint32_t i = atomicAdd(n, 1u);
    if (i < kRepairCap) slots[i] = slot;
    else qNext[atomicAdd(&counters[WC_NEXT], 1u)] = slot;
  }
  __device__ __forceinline__ void died() { dummies++; }
  __device__ __forceinline__ void flush() {                // (convergent: at the end of the kernel)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = *n < kRepairCap ? *n : kRepairCap;
    if (count != 0u) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&counters[WC_NEXT], count);
      base = __shfl(base, 0);
      for (uint32_t i = lane; i < count; i += 64u) qNext[base + i] = slots[i];
    }
    uint32_t d = dummies;
    for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o);
    if (lane == 0 && d) atomicAdd(&counters[WC_DUMMY], d);
  }
};
constexpr uint32_t kRetryStageCap = 128;     // retries are rare: a small stage keeps the lean kernels at 6 blocks / CU

// a finished path's radiance and its ray count (path segments + unoccluded NEE rays): one 16-byte record per (pixel, sample)
__device__ __forceinline__ void wfWriteL(f4* L, uint32_t slot, f3 v, uint32_t rays) { wfSt(L + slot, mk4(v.x, v.y, v.z, asF(rays))); }

__device__ __forceinline__ void wfAddStat(unsigned long long* p, uint32_t v) {
  unsigned long long r = v;
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o);
  if ((threadIdx.x & 63u) == 0 && r) atomicAdd(p, r);
}

__device__ __forceinline__ void wfFlushTally(unsigned long long* stats, const WfTally& t) {
#if defined(YART_COUNT_TRAVERSAL)
  wfAddStat(stats + 1, t.trav); wfAddStat(stats + 2, t.box); wfAddStat(stats + 3, t.tri); wfAddStat(stats + 4, t.shade);
#else
  (void)stats; (void)t;
#endif
#if defined(YART_TRACE_STATS)
  for (int k = 0; k < 16; k++) wfAddStat(stats + 8 + k, t.ph[k]);
#endif
}

// Persistent traversal loop of the one-ray-per-lane kernels: trace(stk, slot, tally) returns true when
// the path must be retried by the general variant.
template <int LDS_DEPTH, bool RETRY_INPUT, bool LEAN_EXTEND, class Trace>
__device__ __forceinline__ void wfTraverseQueue(const WfArgs& a, const uint32_t* q, uint32_t count, uint32_t* cursor,
                                                uint64_t* ldsStack, Trace trace) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = LDS_DEPTH;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  __shared__ uint32_t stageRetry[kBlock / 64][RETRY_INPUT ? 1 : kRetryStageCap];
  WaveStageT<kRetryStageCap> sRetry{stageRetry[threadIdx.x >> 6], 0};
  WfTally tally;
  const uint32_t nWaves = (gridDim.x * blockDim.x) >> 6;
  // 64 entries at a time from a private range of the queue, topped up `chunk` entries per atomic (leanChunk: one atomic per 64
  // entries runs into the rate a single L2 word takes)
  const uint32_t chunk = leanChunk(count, nWaves);
  uint32_t next = 0, end = 0;
  for (uint32_t base = (gtid >> 6) * 64u; base < count;) {
    const uint32_t k = base + lane;
    bool retry = false;
    uint32_t slot = 0;
    if (k < count) { slot = q[k]; if (slot != kWfFreeSlot) retry = trace(stk, slot, tally); }
    if (!RETRY_INPUT) sRetry.push(a.qR, &a.counters[WC_RETRY], retry, slot);
    if (next == end) {
      uint32_t c = 0;
      if (lane == 0) c = atomicAdd(cursor, chunk);
      next = nWaves * 64u + __shfl(c, 0);
      end = next + chunk;
    }
    base = next;
    next += 64u;
  }
  if (!RETRY_INPUT) sRetry.flush(a.qR, &a.counters[WC_RETRY]);
  wfFlushTally(a.stats, tally);
#if defined(YART_COUNT_TRAVERSAL)
  // the roofline kernel's own share of the exact counters (bench.py): stats[5..7]
  if (LEAN_EXTEND) { wfAddStat(a.stats + 5, tally.trav); wfAddStat(a.stats + 6, tally.box); wfAddStat(a.stats + 7, tally.tri); }
  wfAddStat(a.stats + 10, tally.flipAlive); wfAddStat(a.stats + 11, tally.flipDead);     // (k_wf_shadow: roulette decisions of shade reversed)
#endif
}

// lean closest-hit kernel, one ray per lane; MODE = TRAV_FAST or TRAV_FAST | TRAV_IDENTITY (scene property)
template <int MODE>
__global__ void __launch_bounds__(kBlock, 6) k_wf_extend_fast(WfArgs a) {
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStackFast * kBlock];
  wfTraverseQueue<kWfLdsStackFast, false, true>(a, a.qA, a.counters[WC_ACTIVE], &a.counters[WC_CUR_EXTEND], ldsStack,
      [&](const TravStack& stk, uint32_t slot, WfTally& tally) { return !wfExtendFast<MODE>(a.sc, stk, a.st, slot, tally); });
}
// general closest-hit kernel; RETRY: over the retry queue of k_wf_extend_fast, else over the active queue
template <bool RETRY>
__global__ void __launch_bounds__(kBlock, 4) k_wf_extend(WfArgs a) {
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStack * kBlock];
  wfTraverseQueue<kWfLdsStack, true, false>(a, RETRY ? a.qR : a.qA, a.counters[RETRY ? WC_RETRY : WC_ACTIVE],
      &a.counters[RETRY ? WC_CUR_RETRY : WC_CUR_EXTEND], ldsStack,
      [&](const TravStack& stk, uint32_t slot, WfTally& tally) { wfExtend(a.sc, a.rc, stk, a.st, slot, tally); return false; });
}
template <int MODE>
__global__ void __launch_bounds__(kBlock, 6) k_wf_shadow_fast(WfArgs a) {
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStackFast * kBlock];
  uint32_t rays = 0;
  wfTraverseQueue<kWfLdsStackFast, false, false>(a, a.qS, a.counters[WC_SHADOW], &a.counters[WC_CUR_SHADOW], ldsStack,
      [&](const TravStack& stk, uint32_t slot, WfTally& tally) { WfNoRepair none; return !wfShadow<MODE>(a.sc, a.rc, stk, a.st, slot, tally, a.L, a.slotMap, a.poolSlots != 0u, rays, none); });
  wfAddStat(a.stats, rays);
}
template <bool RETRY>
__global__ void __launch_bounds__(kBlock, 4) k_wf_shadow(WfArgs a) {
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStack * kBlock];
  uint32_t rays = 0;
  __shared__ WfRepairLds repairLds;
  WfRepair repair(repairLds, a.qB, a.counters);
  wfTraverseQueue<kWfLdsStack, true, false>(a, RETRY ? a.qR : a.qS, a.counters[RETRY ? WC_RETRY : WC_SHADOW],
      &a.counters[RETRY ? WC_CUR_RETRY : WC_CUR_SHADOW], ldsStack,
      [&](const TravStack& stk, uint32_t slot, WfTally& tally) {
        wfShadow<TRAV_GENERAL>(a.sc, a.rc, stk, a.st, slot, tally, a.L, a.slotMap, a.poolSlots != 0u, rays, repair);
        return false;
      });
  repair.flush();
  wfAddStat(a.stats, rays);
}
// Lean kernels with in-wave ray replacement (trace_lean.hpp); same queues, counters and results as
// k_wf_extend_fast / k_wf_shadow_fast.
template <int MODE, int NODES>
__global__ void __launch_bounds__(kBlock, leanWaves(MODE)) k_wf_extend_lean(WfArgs a) {
  WF_EMPTY_BLOCK(a.counters[WC_ACTIVE], kBlock);
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStackFast * kBlock];
  __shared__ uint32_t stageRetry[kBlock / 64][kRetryStageCap];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = kWfLdsStackFast;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  WaveStageT<kRetryStageCap> sRetry{stageRetry[threadIdx.x >> 6], 0};
  WfTally tally;
  const WfState st = a.st;
  stk.rec = a.resumeRec; stk.recCursor = &a.counters[WC_RESUME]; stk.recCap = a.resumeCap;
  __shared__ __attribute__((aligned(16))) LeanSceneLds sceneLds;        // (used by the kNodesMaskLds form only)
  if (NODES == kNodesMaskLds) leanSceneToLds(a.sc, sceneLds, a.sc.nMeshes);
  traceLeanAny<false, MODE, NODES>(a.sc, a.rc.sampler, stk, a.qA, a.counters[WC_ACTIVE], &a.counters[WC_CUR_EXTEND],
      [&](uint32_t slot) {
        const f4 r0 = wfLd(st.ray0 + slot), r1 = wfLd(st.ray1 + slot);
        LeanRay r; r.o = mk3(r0.x, r0.y, r0.z); r.d = mk3(r0.w, r1.x, r1.y); r.tMax = kInf;
        return r;
      },
      [&](uint32_t slot, const HitRec& h, bool didHit, f3, uint32_t) {
        wfSt(st.hit0 + slot, mk4(didHit ? h.t : -1.0f, h.u, h.v, asF(h.tri)));
        wfSt1(&st.hit1[slot].x, asF(wfHitWord(h, didHit)));
      },
      [&](bool pred, uint32_t slot) { sRetry.push(a.qR, &a.counters[WC_RETRY], pred, slot); }, tally);
  sRetry.flush(a.qR, &a.counters[WC_RETRY]);
  wfFlushTally(a.stats, tally);
#if defined(YART_COUNT_TRAVERSAL)
  wfAddStat(a.stats + 5, tally.trav); wfAddStat(a.stats + 6, tally.box); wfAddStat(a.stats + 7, tally.tri);
  wfAddStat(a.stats + 27, tally.waste);
#endif
}
template <int MODE, int NODES>
__global__ void __launch_bounds__(kBlock, leanWaves(MODE)) k_wf_shadow_lean(WfArgs a) {
  WF_EMPTY_BLOCK(a.counters[WC_SHADOW], kBlock);
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStackFast * kBlock];
  __shared__ uint32_t stageRetry[kBlock / 64][kRetryStageCap];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = kWfLdsStackFast;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  WaveStageT<kRetryStageCap> sRetry{stageRetry[threadIdx.x >> 6], 0};
  WfTally tally;
  const WfState st = a.st;
  uint32_t nRays = 0;
  stk.rec = a.resumeRec; stk.recCursor = &a.counters[WC_RESUME]; stk.recCap = a.resumeCap;
  __shared__ __attribute__((aligned(16))) LeanSceneLds sceneLds;        // (used by the kNodesMaskLds form only)
  if (NODES == kNodesMaskLds) leanSceneToLds(a.sc, sceneLds, a.sc.nMeshes);
  traceLeanAny<true, MODE, NODES>(a.sc, a.rc.sampler, stk, a.qS, a.counters[WC_SHADOW], &a.counters[WC_CUR_SHADOW],
      [&](uint32_t slot) {
        const f4 r0 = wfLd(st.ray0 + slot), s0 = wfLd(st.sh0 + slot);
        const f3 from = mk3(r0.x, r0.y, r0.z), to = mk3(s0.x, s0.y, s0.z);
        LeanRay r; r.o = from; r.d = normalized(to - from);     // mis-integrator.cpp:140
        r.tMax = length(to - from) - 0.001f;                     // :144
        return r;
      },
      [&](uint32_t slot, const HitRec&, bool occluded, f3, uint32_t) {
        nRays += wfShadowCommit(st, slot, occluded, mk3(1.0f), a.L, a.slotMap, a.poolSlots != 0u);      // (the lean walk never attenuates)
      },
      [&](bool pred, uint32_t slot) { sRetry.push(a.qR, &a.counters[WC_RETRY], pred, slot); }, tally);
  sRetry.flush(a.qR, &a.counters[WC_RETRY]);
  wfAddStat(a.stats, nRays);
  wfFlushTally(a.stats, tally);
#if defined(YART_COUNT_TRAVERSAL)
  wfAddStat(a.stats + 24, tally.trav); wfAddStat(a.stats + 25, tally.box); wfAddStat(a.stats + 26, tally.tri);
  wfAddStat(a.stats + 31, tally.waste);
#endif
}

// General closest-hit / shadow traversal of the retry queue in the same in-wave-replacement form
// (alpha tests and NEE attenuation inline; sampler state per lane).
#ifndef YART_RETRY_WAVES
#define YART_RETRY_WAVES 4
#endif
template <int NODES>
__global__ void __launch_bounds__(kBlock, YART_RETRY_WAVES) k_wf_extend_retry_lean(WfArgs a) {
  WF_EMPTY_BLOCK(a.counters[WC_RETRY], kBlock);
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStack * kBlock];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = kWfLdsStack;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  WfTally tally;
  const WfState st = a.st;
  stk.rec = a.resumeRec; stk.recCursor = &a.counters[WC_RESUME]; stk.recCap = a.resumeCap;
  __shared__ __attribute__((aligned(16))) LeanSceneLds sceneLds;        // (used by the kNodesMaskLds form only)
  if (NODES == kNodesMaskLds) leanSceneToLds(a.sc, sceneLds, a.sc.nMeshes);
  __shared__ uint64_t sHash[264];                          // the alpha tests' draws read one hashDim value each
  if (a.rc.sampler.tab.hash != nullptr && a.rc.sampler.tab.dims + 3u <= 264u) {
    for (uint32_t k = threadIdx.x; k < a.rc.sampler.tab.dims + 3u; k += blockDim.x) sHash[k] = a.rc.sampler.tab.hash[k];
    __syncthreads();
    a.rc.sampler.tab.hash = sHash;
  }
  traceLeanAny<false, TRAV_GENERAL, NODES>(a.sc, a.rc.sampler, stk, a.qR, a.counters[WC_RETRY], &a.counters[WC_CUR_RETRY],
      [&](uint32_t slot) {
        const f4 r0 = wfLd(st.ray0 + slot), r1 = wfLd(st.ray1 + slot), h1 = wfLd(st.hit1 + slot);
        LeanRay r; r.o = mk3(r0.x, r0.y, r0.z); r.d = mk3(r0.w, r1.x, r1.y); r.tMax = kInf;
        r.smp.dim = asU(wfLd1(&st.thr[slot].w)); r.smp.morton = uint64_t(asU(h1.y)) | (uint64_t(asU(h1.z)) << 32); r.smp.pix = asU(h1.w);
        return r;
      },
      [&](uint32_t slot, const HitRec& h, bool didHit, f3, uint32_t dim) {
        wfSt(st.hit0 + slot, mk4(didHit ? h.t : -1.0f, h.u, h.v, asF(h.tri)));
        wfSt1(&st.hit1[slot].x, asF(wfHitWord(h, didHit)));
        wfSt1(&st.thr[slot].w, asF(dim));
      },
      [&](bool, uint32_t) {}, tally);
  wfFlushTally(a.stats, tally);
#if defined(YART_COUNT_TRAVERSAL)
  wfAddStat(a.stats + 29, tally.trav);       // closest-hit rays the lean kernel handed over
  wfAddStat(a.stats + 8, tally.resumed);     // ... of which resumed
#endif
}
template <int NODES>
__global__ void __launch_bounds__(kBlock, YART_RETRY_WAVES) k_wf_shadow_retry_lean(WfArgs a) {
  WF_EMPTY_BLOCK(a.counters[WC_RETRY], kBlock);
  WF_DYN(a);
  __shared__ uint64_t ldsStack[kWfLdsStack * kBlock];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = kWfLdsStack;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  WfTally tally;
  const WfState st = a.st;
  uint32_t nRays = 0;
  stk.rec = a.resumeRec; stk.recCursor = &a.counters[WC_RESUME]; stk.recCap = a.resumeCap;
  __shared__ __attribute__((aligned(16))) LeanSceneLds sceneLds;        // (used by the kNodesMaskLds form only)
  if (NODES == kNodesMaskLds) leanSceneToLds(a.sc, sceneLds, a.sc.nMeshes);
  __shared__ uint64_t sHash[264];                          // the alpha tests' draws read one hashDim value each
  if (a.rc.sampler.tab.hash != nullptr && a.rc.sampler.tab.dims + 3u <= 264u) {
    for (uint32_t k = threadIdx.x; k < a.rc.sampler.tab.dims + 3u; k += blockDim.x) sHash[k] = a.rc.sampler.tab.hash[k];
    __syncthreads();
    a.rc.sampler.tab.hash = sHash;
  }
  __shared__ WfRepairLds repairLds;
  WfRepair repair(repairLds, a.qB, a.counters);
  traceLeanAny<true, TRAV_GENERAL, NODES>(a.sc, a.rc.sampler, stk, a.qR, a.counters[WC_RETRY], &a.counters[WC_CUR_RETRY],
      [&](uint32_t slot) {
        const f4 r0 = wfLd(st.ray0 + slot), s0 = wfLd(st.sh0 + slot), h1 = wfLd(st.hit1 + slot);
        const f3 from = mk3(r0.x, r0.y, r0.z), to = mk3(s0.x, s0.y, s0.z);
        LeanRay r; r.o = from; r.d = normalized(to - from); r.tMax = length(to - from) - 0.001f;
        r.smp.dim = asU(s0.w); r.smp.morton = uint64_t(asU(h1.y)) | (uint64_t(asU(h1.z)) << 32); r.smp.pix = asU(h1.w);   // (thr.w may stand past a pending roulette draw)
        return r;
      },
      [&](uint32_t slot, const HitRec&, bool occluded, f3 att, uint32_t dim) {
        // (alpha tests of the shadow walk draw before the roulette does: the dimension is stored, a pending roulette drawn again)
        nRays += wfShadowCommitGeneral(a.rc.sampler, st, slot, occluded, att, asU(wfLd1(&st.sh0[slot].w)), dim, a.L, a.slotMap, a.poolSlots != 0u,
                                       repair, tally);
      },
      [&](bool, uint32_t) {}, tally);
  repair.flush();
  wfAddStat(a.stats, nRays);
  wfFlushTally(a.stats, tally);
#if defined(YART_COUNT_TRAVERSAL)
  wfAddStat(a.stats + 30, tally.trav);       // shadow rays the lean kernel handed over
  wfAddStat(a.stats + 9, tally.resumed);
  wfAddStat(a.stats + 10, tally.flipAlive); wfAddStat(a.stats + 11, tally.flipDead);     // roulette decisions of shade reversed
#endif
}

#ifndef YART_SHADE_WAVES
#define YART_SHADE_WAVES 3      // 168 VGPRs + ~300 B of scratch per lane: measured 4 % faster than 2 waves without spills, 4 waves lose 9 %
#endif
// A wave takes 256 queue entries at a time and, with SORT (YART_FLAG_SHADE_SORT), buckets them by lobe class
// (plain / transmissive / clearcoat / metallic combinations of the hit's material — the branches
// parametric.cpp:226-251 chooses between —, or "miss"; the material index is bits 20..30 of the hit word the
// traversal kernels wrote) before shading them 64 at a time: wave ballots partition the 4 x 64 entries class by
// class into an LDS array (a stable partition: entries of one class keep their queue order, so a scene of one
// class keeps its coalesced state access), so that the lanes of a sub-batch run the same lobes.
// Paths are independent: the order in which they are shaded does not change any result.
// Round 1 bucketed by material index: +5 % shade time on the C3 scene (22 materials of one class, scattered
// state access for nothing), -9.5 % on the McLaren-class scene (clearcoat paint / glass / chrome / diffuse).
// Read-only tables the shade kernel keeps in LDS (one copy per CU: its workgroup is the CU's 12 waves). What the kernel waits on is a
// chain of some seventy DEPENDENT reads per batch of hits, most of them L2 hits of ~500 cycles; a read from LDS is a fifth of that.
// 1080p x 64 spp, shade kernel: 72.4 ms -> 68.2 (sampler tables + GGX tables, 256-thread workgroups) -> 64.8 (one 768-thread
// workgroup per CU) -> 53.8 (the scene's small records): profiles/r3_ab_shade_lds.txt.
// Workgroup of the shade kernel: YART_SHADE_WAVES waves per SIMD in ONE workgroup per CU (768 threads), so that the read-only
// tables it keeps in LDS exist once per CU.
constexpr int kShadeBlock = YART_SHADE_WAVES * 256;
constexpr uint32_t kShadeStageCap = 512;   // LDS staging of the kernel's two queue appends (one atomic per CAP - 64 entries; 256: kernel +4 %)
constexpr int kShadeBlocksPerCU = 1;
// slots of the kernel's LDS copies of the scene's small tables (yart_hip.hip decides FIT against them)
constexpr uint32_t kShadeHashSlots = 264, kShadeMatSlots = 64, kShadeTexSlots = 128, kShadeLightSlots = 8, kShadeEnvSlots = 4, kShadeNodeSlots = 32;
// FIT: the host has checked that the sampler tables are in use and that every scene table fits its slot below; the copies' being in LDS is
// then known at compile time (ds_read with constant addresses; kernel 54.7 -> 52.0 ms). Otherwise each table is repointed only if it fits.
// ENV1: the scene's only light is one infinite light (the reference's own set-up: an environment map, no emissive mesh) — the host has checked;
// the light-selection and area-light code then folds away (scratch 52 -> 36 B, kernel 51.6 -> 49.7 ms).
template <bool SORT, bool FIT, bool ENV1>
__global__ void __launch_bounds__(kShadeBlock, kShadeBlocksPerCU) k_wf_shade(WfArgs a) {
  WF_EMPTY_BLOCK(a.counters[0], kShadeBlock * 4);           // (a wave takes 256 entries at a time)
  WF_DYN(a);
  if (ENV1) { __builtin_assume(a.sc.nArea == 0u); __builtin_assume(a.sc.nInfinite == 1u); __builtin_assume(a.sc.nLights == 1u); }
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long laneLt = (1ull << lane) - 1ull;
  const uint32_t* sobol = reinterpret_cast<const uint32_t*>(a.sc.lut + LutDev::sobol);
  const uint32_t count = a.counters[0];
  uint32_t rays = 0;
  WfTally tally;
  __shared__ uint32_t stageNext[kShadeBlock / 64][kShadeStageCap], stageShadow[kShadeBlock / 64][kShadeStageCap];
  __shared__ uint32_t sorted[kShadeBlock / 64][SORT ? 256 : 1];
  WaveStageT<kShadeStageCap> sNext{stageNext[threadIdx.x >> 6], 0}, sShadow{stageShadow[threadIdx.x >> 6], 0};
  uint32_t* mySorted = sorted[threadIdx.x >> 6];
  const uint32_t waveId = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nWaves = (gridDim.x * blockDim.x) >> 6;
  uint32_t nSorted = 0;
  // The sampler's small tables — hashDim values (one read per draw) and the byte-wise XOR tables of the Sobol' matrix (four reads
  // per 2D draw) — from a copy in LDS: every one of them is a hop in the chain of dependent reads this kernel waits on, and an
  // LDS hop is a fifth of an L2 hop.
  __shared__ uint64_t sHash[kShadeHashSlots];
  __shared__ uint32_t sSobol1[8 * 256];
  if (FIT || (a.rc.sampler.tab.hash != nullptr && a.rc.sampler.tab.dims + 3u <= kShadeHashSlots)) {
    for (uint32_t k = threadIdx.x; k < a.rc.sampler.tab.dims + 3u; k += blockDim.x) sHash[k] = a.rc.sampler.tab.hash[k];
    for (uint32_t k = threadIdx.x; k < 8u * 256u; k += blockDim.x) sSobol1[k] = a.rc.sampler.tab.sobol1[k];
    __syncthreads();
    a.rc.sampler.tab.hash = sHash; a.rc.sampler.tab.sobol1 = sSobol1;
  }
  // ... and the GGX energy tables of the glossy lobes (bsdf.hpp::lutInLds): E, Eavg, baseE, baseEavg, 21.6 KB
  __shared__ float sLut[LutDev::glassE + 2];
  {
    const float* g = a.sc.lut;
    for (uint32_t k = threadIdx.x; k < LutDev::glassE; k += blockDim.x) sLut[k] = g[k];
    if (threadIdx.x == 0) {
      const uint64_t p = reinterpret_cast<uint64_t>(g);
      reinterpret_cast<uint32_t*>(sLut)[LutDev::glassE] = uint32_t(p); reinterpret_cast<uint32_t*>(sLut)[LutDev::glassE + 1] = uint32_t(p >> 32);
    }
    __syncthreads();
    a.sc.lut = sLut;
  }
  // ... and the scene's small records — materials, texture and light and environment descriptors, scene nodes, the lobe classes —
  // where they fit (a table that does not stays where it is: the pointers are generic)
  {
    constexpr uint32_t kMatCap = kShadeMatSlots, kTexCap = kShadeTexSlots, kLightCap = kShadeLightSlots, kEnvCap = kShadeEnvSlots, kNodeCap = kShadeNodeSlots, kInfCap = kShadeLightSlots;
    __shared__ __attribute__((aligned(16))) uint32_t sMat[kMatCap * sizeof(MaterialDev) / 4], sTex[kTexCap * sizeof(TexDev) / 4],
        sLight[kLightCap * sizeof(LightDev) / 4], sEnv[kEnvCap * sizeof(EnvDev) / 4], sNode[kNodeCap * sizeof(NodeDev) / 4], sInf[kInfCap],
        sClass[kMatCap / 4];
    const bool mOk = FIT || a.sc.nMaterials <= kMatCap, tOk = FIT || a.sc.nTextures <= kTexCap, lOk = FIT || (a.sc.nLights <= kLightCap && a.sc.nLights > 0u),
               eOk = FIT || a.sc.nEnvs <= kEnvCap, nOk = FIT || a.sc.nNodes <= kNodeCap, iOk = FIT || (a.sc.nInfinite <= kInfCap && a.sc.nInfinite > 0u);
    if (mOk) { ldsCopyWords(sMat, a.sc.materials, a.sc.nMaterials * uint32_t(sizeof(MaterialDev) / 4)); ldsCopyWords(sClass, a.matClass, (a.sc.nMaterials + 3u) / 4u); }
    if (tOk) ldsCopyWords(sTex, a.sc.textures, a.sc.nTextures * uint32_t(sizeof(TexDev) / 4));
    if (lOk) ldsCopyWords(sLight, a.sc.lights, a.sc.nLights * uint32_t(sizeof(LightDev) / 4));
    if (eOk) ldsCopyWords(sEnv, a.sc.envs, a.sc.nEnvs * uint32_t(sizeof(EnvDev) / 4));
    if (nOk) ldsCopyWords(sNode, a.sc.nodes, a.sc.nNodes * uint32_t(sizeof(NodeDev) / 4));
    if (iOk) ldsCopyWords(sInf, a.sc.infiniteLights, a.sc.nInfinite);
    __syncthreads();
    if (mOk) { a.sc.materials = reinterpret_cast<const MaterialDev*>(sMat); a.matClass = reinterpret_cast<const uint8_t*>(sClass); }
    if (tOk) a.sc.textures = reinterpret_cast<const TexDev*>(sTex);
    if (lOk) a.sc.lights = reinterpret_cast<const LightDev*>(sLight);
    if (eOk) a.sc.envs = reinterpret_cast<const EnvDev*>(sEnv);
    if (nOk) a.sc.nodes = reinterpret_cast<const NodeDev*>(sNode);
    if (iOk) a.sc.infiniteLights = sInf;
  }
#if defined(YART_SHADE_REGIONS) && defined(__HIP_DEVICE_COMPILE__)
  if (lane == 0) { for (int k = 0; k < 3 * kShadeRegions; k++) srAcc[threadIdx.x >> 6][k] = 0; srLast[threadIdx.x >> 6] = clock64(); }
#endif
  for (uint32_t sub = 0, grab = waveId * 256u, first = 1;; sub = (sub + 1u) & 3u) {
    if (sub == 0) {
      if (!first) {                            // one dequeue atomic per 256 paths (first grab: by wave index)
        if (lane == 0) grab = atomicAdd(&a.counters[4], 256u);
        grab = nWaves * 256u + __shfl(grab, 0);
      }
      if (SORT && grab < count) {
        uint32_t slots[4], keys[4];
        unsigned long long pending[4];
        for (int r = 0; r < 4; r++) {
          const uint32_t k = grab + uint32_t(r) * 64u + lane;
          const uint32_t word = k < count ? a.qA[k] : kWfFreeSlot;     // (path pool: the slots in order, free ones marked)
          const bool valid = word != kWfFreeSlot;
          slots[r] = valid ? word : 0u;
          if (valid) {
            const uint32_t m = (asU(wfLd1(&a.st.hit1[slots[r]].x)) >> kWfNodeBits) & kWfClassMiss;
            keys[r] = m == kWfClassMiss ? 0xffu : uint32_t(a.matClass[m]);
          } else keys[r] = 0xffffffffu;
          pending[r] = __ballot(valid);
        }
        uint32_t out = 0;
        while (pending[0] | pending[1] | pending[2] | pending[3]) {          // one round per class present
          uint32_t key = 0;
          for (int r = 3; r >= 0; r--)
            if (pending[r]) key = __shfl(keys[r], __ffsll((long long) pending[r]) - 1);   // first pending entry's class
          for (int r = 0; r < 4; r++) {
            const unsigned long long m = __ballot(keys[r] == key) & pending[r];
            if ((m >> lane) & 1ull) mySorted[out + uint32_t(__popcll(m & laneLt))] = slots[r];
            out += uint32_t(__popcll(m));
            pending[r] &= ~m;
          }
        }
        nSorted = out;
      }
    }
    first = 0;
    SR_MARK(12);                               // tile grab + bucketing (and the loop overhead of the other sub-batches)
    const uint32_t base = grab + sub * 64u;
    if (base >= count) break;
    const uint32_t k = base + lane;
    bool toNext = false, toShadow = false;
    uint32_t slot = 0;
    const bool valid = SORT ? (sub * 64u + lane < nSorted) : (k < count && a.qA[k] != kWfFreeSlot);
    if (valid) {
      slot = SORT ? mySorted[sub * 64u + lane] : a.qA[k];
      WfPath p;
      WfShadeResult r = wfShade(a.sc, a.rc, sobol, a.st, slot, p, rays, tally);
      if (r == WF_SHADOW) {
        // The roulette of a path with a shadow ray comes after the shadow traversal, which may draw sampler dimensions — but
        // only in the general kernels: the decision is taken here, tentatively, and a general shadow kernel whose walk drew
        // takes it again (wfRouletteTentative, wfShadowCommitGeneral). At depth 1 none applies yet (wfRoulette: depth > 1),
        // the path simply continues; a path whose bounce budget is used up (WF_FINAL, set by wfShade) — or that dies in the
        // tentative draw — is written out by whoever commits its shadow ray. (Path pool: k_wf_roulette decides, after the
        // shadow stage.)
        toShadow = true;
        if (p.flags & WF_FINAL) toNext = false;
        else if ((p.flags & WF_DEPTH_MASK) <= 1u) toNext = true;
        else toNext = !a.poolSlots && wfRouletteTentative(a.rc, p);
        wfStoreThr(a.st, slot, p);              // (wfShade has stored the new ray)
      } else if (r == WF_CONTINUE && wfRoulette(a.rc, p)) {
        wfStoreThr(a.st, slot, p);
        toNext = true;
      } else if (r != WF_SKIPPED) {
        // segments traced: a path that ends inside wfShade (miss / absorbed) still carries the depth it entered with
        const uint32_t segs = (p.flags & WF_DEPTH_MASK) + (r == WF_TERMINATED ? 1u : 0u);
        wfRetire(a.L, a.slotMap, p.slot, mk4(p.L.x, p.L.y, p.L.z, asF(segs + ((p.flags & WF_NEE_MASK) >> WF_NEE_SHIFT))), a.poolSlots != 0u);
      }
    }
    if (!a.poolSlots) sNext.push(a.qB, &a.counters[1], toNext, slot);     // (path pool: a path that goes on simply keeps its slot)
    sShadow.push(a.qS, &a.counters[2], toShadow, slot);
    SR_MARK(11);                               // roulette, throughput / radiance stores, queue appends
  }
  sNext.flush(a.qB, &a.counters[1]);
  sShadow.flush(a.qS, &a.counters[2]);
#if defined(YART_SHADE_REGIONS) && defined(__HIP_DEVICE_COMPILE__)
  if (lane == 0) for (int k = 0; k < 3 * kShadeRegions; k++) if (srAcc[threadIdx.x >> 6][k]) atomicAdd(&g_shadeRegion[k], srAcc[threadIdx.x >> 6][k]);
#endif
  wfAddStat(a.stats, rays);
  wfFlushTally(a.stats, tally);
#if defined(YART_COUNT_TRAVERSAL)
  wfAddStat(a.stats + 28, rays);             // entries shaded by this kernel (hits and misses): one path segment each
#endif
}
