// stream_kernels.inc — the streaming passes of the wavefront pipelines: light, uniform work per path or per slot between the
// traversal and shade stages, and the sampler tables of a render. Ten kernels, none a template, so they are emitted wherever
// this file is compiled: included by yart_hip.hip (unit 0) only, inside the anonymous namespace, after wavefront_kernels.inc
// (WfArgs, WfDyn, WfCounter, WF_DYN, WF_EMPTY_BLOCK, WaveStage, samplerToLds).
//   k_sampler_tables     once per render: the sampler's tables for the rank's pixels
//   k_wf_generate        camera rays of a batch;  k_wf_refill / k_wf_pool_init / k_wf_pool_advance  the path pool's rounds
//   k_wf_reset_retry     after a retry pass;  k_wf_advance  swap queue counters between two bounces
//   k_wf_compact / k_wf_compact_commit   dense copy of the survivors' state (late bounces)
//   k_wf_roulette        path pool only: Russian roulette of the `shadow` paths at depth >= 2 (the batch-synchronous pipeline
//                        decides in k_wf_shade, wavefront.hpp: wfRouletteTentative)

// SamplerTables of one render (sampler.hpp): entries for dims x this rank's pixels, hashDim
// values, byte-wise XOR tables of the Sobol' dimension-1 matrix (LutDev::sobol columns 52..103)
struct SamplerTabArgs {
  SamplerConfig cfg;
  const uint32_t* pixels; uint32_t nPixels, dims;
  uint64_t* entries; uint64_t* hash; uint32_t* sobol1;
  const uint32_t* matrix52;
};
__global__ void __launch_bounds__(kBlock) k_sampler_tables(SamplerTabArgs a) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (uint32_t k = gtid; k < a.dims + 3u; k += stride) a.hash[k] = hashDim(k);
  for (uint32_t k = gtid; k < 8u * 256u; k += stride) {
    const uint32_t b = k >> 8, v = k & 255u;
    uint32_t x = 0;
    for (uint32_t j = 0; j < 8; j++) if (((v >> j) & 1u) && 8u * b + j < 52u) x ^= a.matrix52[8u * b + j];
    a.sobol1[k] = x;
  }
  const uint64_t total = uint64_t(a.dims) * a.nPixels;
  for (uint64_t k = gtid; k < total; k += stride) {               // entries[pixel][dimension]
    const uint32_t pi = uint32_t(k / a.dims), dim = uint32_t(k - uint64_t(pi) * a.dims);
    const uint32_t pk = a.pixels[pi];
    a.entries[k] = samplerTableEntry(a.cfg, encodeMorton2(pk & 0xffffu, pk >> 16), dim);
  }
}

__global__ void __launch_bounds__(kBlock) k_wf_generate(WfArgs a) {
  WF_DYN(a);
  const uint32_t* sobol = reinterpret_cast<const uint32_t*>(a.sc.lut + LutDev::sobol);
  __shared__ SamplerLds smpLds;
  samplerToLds(a.rc.sampler, smpLds, true);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nPaths; i += gridDim.x * blockDim.x) {
    const uint32_t pi = i / a.spp, s = i - pi * a.spp;
    const uint32_t pk = a.pixels[pi];
    wfGenerate(a.rc, sobol, a.cam, pk & 0xffffu, pk >> 16, s + a.sampleOffset, a.pixBase + pi, a.st, i);
    a.qA[i] = i;
  }
}

// Path pool: every wave scans its share of the slots; a free slot (its path has ended, or the pool has just been created) gets the
// batch's next path — camera sample, path state, slotMap[slot] = path index. The round's kernels then take the slots IN ORDER
// (the "queue" this kernel writes is the identity with the free slots marked kWfFreeSlot): while the batch lasts every slot is
// live, so state accesses are as dense as a wave's lanes — paths that go on keep their slots, nothing is appended or compacted.
// Two passes over the wave's slots: count the free ones, claim as many path indices with ONE atomic (a word takes ~90 atomics per
// microsecond: one per 64 slots would cost milliseconds per round), then generate. counters[WC_NEXT] receives the number of
// live slots (what the host watches to see the batch finish).
__global__ void __launch_bounds__(kBlock) k_wf_refill(WfArgs a) {
  const uint32_t* sobol = reinterpret_cast<const uint32_t*>(a.sc.lut + LutDev::sobol);
  __shared__ SamplerLds smpLds;
  samplerToLds(a.rc.sampler, smpLds, true);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waveId = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nWaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t per = (((a.poolSlots + nWaves - 1u) / nWaves) + 63u) & ~63u;
  const uint32_t s0 = waveId * per < a.poolSlots ? waveId * per : a.poolSlots, s1 = s0 + per < a.poolSlots ? s0 + per : a.poolSlots;
  uint32_t nFree = 0;
  for (uint32_t base = s0; base < s1; base += 64u) {
    const uint32_t slot = base + lane;
    nFree += uint32_t(__popcll(__ballot(slot < s1 && a.slotMap[slot] == kWfFreeSlot)));
  }
  uint32_t first = 0, avail = 0;
  if (nFree != 0u && a.counters[WC_STARTED] < a.nPaths) {      // (wave-uniform; the counter only grows: a stale read costs an atomic)
    if (lane == 0) first = atomicAdd(&a.counters[WC_STARTED], nFree);
    first = __shfl(first, 0);
    avail = first < a.nPaths ? (a.nPaths - first < nFree ? a.nPaths - first : nFree) : 0u;
  }
  uint32_t taken = 0;
  for (uint32_t base = s0; base < s1; base += 64u) {
    const uint32_t slot = base + lane;
    const bool isFree = slot < s1 && a.slotMap[slot] == kWfFreeSlot;
    const unsigned long long m = __ballot(isFree);
    const uint32_t k = taken + uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
    const bool take = isFree && k < avail;
    if (take) {
      const uint32_t i = first + k;                            // path index within the batch: pixel i / spp, sample i % spp
      const uint32_t pi = i / a.spp, sm = i - pi * a.spp;
      const uint32_t pk = a.pixels[pi];
      wfGenerate(a.rc, sobol, a.cam, pk & 0xffffu, pk >> 16, sm + a.sampleOffset, a.pixBase + pi, a.st, slot);
      a.slotMap[slot] = i;
    }
    if (slot < s1) a.qA[slot] = (isFree && !take) ? kWfFreeSlot : slot;
    taken += uint32_t(__popcll(m));
  }
  const uint32_t live = (s1 - s0) - nFree + avail;
  if (lane == 0 && live != 0u) atomicAdd(&a.counters[WC_NEXT], live);
}
// end of a round of the path pool: the next round's queue is again all slots; cursors and per-round counters zeroed
__global__ void k_wf_pool_advance(uint32_t* counters, uint32_t poolSlots) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    counters[WC_ACTIVE] = poolSlots;
    for (uint32_t k = 1; k < WC_COUNT; k++) if (k != WC_STARTED) counters[k] = 0;
  }
}
__global__ void k_wf_pool_init(uint32_t* slotMap, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) slotMap[i] = kWfFreeSlot;
}

// between a lean kernel and its retry pass / before the next user of the retry queue
__global__ void k_wf_reset_retry(uint32_t* counters) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { counters[WC_RETRY] = 0; counters[WC_CUR_RETRY] = 0; counters[WC_RESUME] = 0; }
}

// between two bounces (after k_wf_advance: counters[WC_ACTIVE] paths in qA): copy the live fields of the
// survivors — ray0, ray1, thr, acc, hit1 (sampler state) — into the tail state that is not in use, in queue
// order, and make the queue the identity. Done only if the survivors fit and fill at most half of the slots in
// use; the decision depends on device values that neither kernel changes, so k_wf_compact_commit repeats it.
#ifndef YART_COMPACT_NUM
#define YART_COMPACT_NUM 1      // compact when the survivors fill at most NUM / DEN of the slots in use
#define YART_COMPACT_DEN 2
#endif
__device__ __forceinline__ bool wfCompactPlan(const WfArgs& a, const WfDyn& d, uint32_t count, uint32_t& dst) {
  dst = d.inTail == 1u ? 1u : 0u;
  return count > 0u && count <= a.tailCap[dst] && uint64_t(YART_COMPACT_DEN) * count <= uint64_t(YART_COMPACT_NUM) * d.extent;
}
__global__ void __launch_bounds__(kBlock) k_wf_compact(WfArgs a) {
  const WfDyn d = *a.dyn;
  const uint32_t count = a.counters[WC_ACTIVE];
  uint32_t dst;
  if (!wfCompactPlan(a, d, count, dst)) return;
  const WfState from = d.st, to = a.tail[dst];
  uint32_t* map = a.tailMap[dst];
  // two survivors per thread and round: ten gathers in flight behind two queue words (the source is sparse: latency, not bandwidth)
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t k0 = blockIdx.x * blockDim.x + threadIdx.x; k0 < count; k0 += 2u * stride) {
    const uint32_t k1 = k0 + stride;
    const bool v1 = k1 < count;
    const uint32_t s0 = a.qA[k0], s1 = v1 ? a.qA[k1] : s0;
    const f4 a0 = wfLd(from.ray0 + s0), b0 = wfLd(from.ray1 + s0), c0 = wfLd(from.thr + s0), d0 = wfLd(from.acc + s0), e0 = wfLd(from.hit1 + s0);
    const f4 a1 = wfLd(from.ray0 + s1), b1 = wfLd(from.ray1 + s1), c1 = wfLd(from.thr + s1), d1 = wfLd(from.acc + s1), e1 = wfLd(from.hit1 + s1);
    const uint32_t m0 = d.slotMap ? d.slotMap[s0] : s0, m1 = d.slotMap ? d.slotMap[s1] : s1;
    wfSt(to.ray0 + k0, a0); wfSt(to.ray1 + k0, b0); wfSt(to.thr + k0, c0); wfSt(to.acc + k0, d0); wfSt(to.hit1 + k0, e0);
    map[k0] = m0; a.qA[k0] = k0;
    if (v1) {
      wfSt(to.ray0 + k1, a1); wfSt(to.ray1 + k1, b1); wfSt(to.thr + k1, c1); wfSt(to.acc + k1, d1); wfSt(to.hit1 + k1, e1);
      map[k1] = m1; a.qA[k1] = k1;
    }
  }
}
__global__ void k_wf_compact_commit(WfArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const WfDyn d = *a.dyn;
  const uint32_t count = a.counters[WC_ACTIVE];
  uint32_t dst;
  if (!wfCompactPlan(a, d, count, dst)) return;
  WfDyn n;
  n.st = a.tail[dst]; n.slotMap = a.tailMap[dst]; n.extent = count; n.inTail = dst + 1u;
  *a.dyn = n;
}

// (pathsLog: where the number of paths that enter the next bounce is added up, for YartStats::paths_at_bounce; may be null)
__global__ void k_wf_advance(uint32_t* counters, unsigned long long* pathsLog) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    counters[0] = counters[1];
    if (pathsLog) *pathsLog += counters[1] - counters[WC_DUMMY];      // (entries of paths written out since they were queued: WF_DEAD)
    for (uint32_t k = 1; k < WC_COUNT; k++) if (k != WC_STARTED) counters[k] = 0;
  }
}

// ---------------------------------------------------------------------------------------
//   k_wf_roulette       Russian roulette + next-bounce decision of the paths of the `shadow` queue, after their shadow rays
//                       (mis-integrator.cpp:96-102). Launched by the path pool only, whose k_wf_shade leaves the decision
//                       to it (no draw is ever pending there); the batch-synchronous form below the pool's is kept for a
//                       pipeline that cannot decide in shade (a.bounce >= 1: the paths leave the bounce at depth >= 2).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_wf_roulette(WfArgs a) {
  WF_EMPTY_BLOCK(a.counters[WC_SHADOW], kBlock);
  WF_DYN(a);
  // light, uniform work per path: static grid-stride assignment (an atomic cursor would
  // serialise ~90 dequeues/us on one L2 word and dominate this kernel)
  const uint32_t count = a.counters[WC_SHADOW];
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t rounds = (count + stride - 1) / stride;
  __shared__ uint32_t stageNext[kBlock / 64][kStageCap];
  WaveStage sNext{stageNext[threadIdx.x >> 6], 0};
  __shared__ SamplerLds smpLds;
  samplerToLds(a.rc.sampler, smpLds, false);
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t k = r * stride + blockIdx.x * blockDim.x + threadIdx.x;
    bool toNext = false;
    uint32_t slot = 0;
    if (k < count) {
      slot = a.qS[k];
      if (a.poolSlots) {
        // path pool: the queue holds paths of every depth. Depth 1: no roulette applies, k_wf_shade queued the path itself;
        // WF_FINAL: written out by the shadow kernels.
        const uint32_t fl = asU(wfLd1(&a.st.acc[slot].w));
        if ((fl & WF_DEPTH_MASK) >= 2u && !(fl & WF_FINAL)) toNext = wfRouletteAfterShadow(a.rc, a.st, slot, fl & WF_DEPTH_MASK, a.L, a.slotMap, true);
      } else toNext = wfRouletteAfterShadow(a.rc, a.st, slot, a.bounce + 1u, a.L, a.slotMap, false);
    }
    if (!a.poolSlots) sNext.push(a.qB, &a.counters[WC_NEXT], toNext, slot);      // (two paths per thread in flight measured: no gain)
  }
  sNext.flush(a.qB, &a.counters[WC_NEXT]);
}
