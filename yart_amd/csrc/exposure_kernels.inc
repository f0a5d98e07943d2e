// exposure_kernels.inc — auto-exposure (yart_hip_exposure_*), device side (included by postprocess.inc, unit 0, after
// denoise_kernels.inc whose 16-byte load / store it uses). The arithmetic is exposure.hpp; the definition is the header comment
// of include/yart_hip.h.
//
//   k_ex_histogram<V>   grid-stride over the metering window's pixels in row order, one aligned 16-byte load per lane and pixel (a
//                     window as wide as the frame is one contiguous run; a narrower one is contiguous per row), four pixels —
//                     four runs of 256 — per lane and pass, loaded before the first is binned: with at most 512 workgroups (two
//                     per CU) that is 32 wave-loads of 1 KB in flight per CU, and half the global atomics of 1024 workgroups.
//                     Each workgroup counts into a private uint32 histogram in LDS and, after a barrier, adds every non-zero bin
//                     to the handle's 256 words with one global atomicAdd each (and the ignored pixels to word 256). Integer
//                     counts: the result does not depend on the order the adds arrive in. A rendered frame puts most of a wave into a handful of
//                     bins, so one LDS atomic per lane on the lane's own bin serialises on that word; two ways round it are
//                     built (tools/exposure_bench.py times both; profiles/auto_exposure.txt):
//                       V = 0  per-wave counting: the wave takes its first active lane's bin, counts the lanes that have it with
//                              a ballot, and that one lane adds the count; repeated until no lane is left — as many LDS atomics
//                              as the wave has distinct bins (1 for a constant frame, 64 at worst). 1 KB of LDS.
//                       V = 1  eight interleaved replicas: lane l adds 1 to word bin * 8 + (l & 7), so lanes with one bin spread
//                              over 8 words on 8 banks; the replicas are summed at the end. 8 KB of LDS.
//   k_ex_resolve      one workgroup of 256 lanes, launched after k_ex_histogram on the same stream — the launch boundary is the
//                     only hand-off: an inclusive scan of the bins in LDS, every lane its bin's term of S, lane 0 sums the 256
//                     terms in ascending order in double and takes the state step; the histogram is copied to the handle's
//                     "last" words (what yart_hip_exposure_get returns) and cleared for the next call.
//   k_ex_apply<LDR, RGB8>   one lane per pixel: 16 bytes in, gain (read from the handle's record), AgX and the 8-bit encoding in
//                     registers, 16 and / or 3 bytes out — where the pair k_tonemap_agx + k_encode_rgb8 writes the tonemapped
//                     frame and reads it again.
// Handle memory: 257 + 256 words and the record. Vector atomics only; no scratch memory.

constexpr uint32_t kExReplicas = 8u;
constexpr uint32_t kExUnroll = 4u;                // pixels per lane and pass of k_ex_histogram: four 16-byte loads in flight per lane

struct ExHistArgs {
  const f4* rgba;
  uint32_t* hist;                                  // kExBins words, then the ignored pixels' count
  uint32_t stride, x0, y0, ww, n;                  // the frame's width; the window's origin, width and pixel count
  ExConst k;
};

template <int V>
__global__ void __launch_bounds__(kBlock) k_ex_histogram(ExHistArgs a) {
  constexpr uint32_t kWords = V == 0 ? kExBins : kExBins * kExReplicas;
  __shared__ uint32_t s_hist[kWords];
  __shared__ uint32_t s_ignored;
  for (uint32_t i = threadIdx.x; i < kWords; i += kBlock) s_hist[i] = 0u;
  if (threadIdx.x == 0) s_ignored = 0u;
  __syncthreads();
  uint32_t ignored = 0u;
  const uint32_t step = gridDim.x * kBlock * kExUnroll;
  // A pass is kExUnroll runs of kBlock consecutive pixels per workgroup, all of a lane's loads issued before the first is used.
  // Every lane of a wave makes the same number of passes (the ballots below need the whole wave): a lane past the end has no pixel.
  for (uint32_t base = blockIdx.x * (kBlock * kExUnroll); base < a.n; base += step) {
    f4 v[kExUnroll];
#pragma unroll
    for (uint32_t j = 0; j < kExUnroll; j++) {
      const uint32_t i = base + j * kBlock + threadIdx.x;
      v[j].x = 0.0f; v[j].y = 0.0f; v[j].z = 0.0f; v[j].w = 0.0f;
      if (i < a.n) {
        const uint32_t y = i / a.ww, x = i - y * a.ww;
        v[j] = dnLd(a.rgba + (size_t(a.y0 + y) * a.stride + (a.x0 + x)));
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kExUnroll; j++) {
      uint32_t bin = kExBins + 1u;                 // no pixel
      if (base + j * kBlock + threadIdx.x < a.n) {
        bin = exBin(v[j].x, v[j].y, v[j].z, a.k);
        if (bin == kExBins) ignored++;
      }
      if (V == 0) {
        uint64_t left = __ballot(bin < kExBins);
        while (left) {
          const uint32_t leader = uint32_t(__builtin_ctzll(left));
          const uint32_t lb = uint32_t(__shfl(int(bin), int(leader)));
          const uint64_t same = __ballot(bin == lb);
          if ((threadIdx.x & 63u) == leader) atomicAdd(&s_hist[lb], uint32_t(__popcll(same)));
          left &= ~same;
        }
      } else {
        if (bin < kExBins) atomicAdd(&s_hist[bin * kExReplicas + (threadIdx.x & (kExReplicas - 1u))], 1u);
      }
    }
  }
  if (ignored) atomicAdd(&s_ignored, ignored);
  __syncthreads();
  uint32_t count = 0u;                             // kBlock == kExBins: lane t owns bin t
  if (V == 0) {
    count = s_hist[threadIdx.x];
  } else {
    for (uint32_t r = 0; r < kExReplicas; r++) count += s_hist[threadIdx.x * kExReplicas + r];
  }
  if (count) atomicAdd(a.hist + threadIdx.x, count);
  if (threadIdx.x == 0 && s_ignored) atomicAdd(a.hist + kExBins, s_ignored);
}

struct ExResolveArgs {
  uint32_t* hist;                                  // kExBins + 1 words: read, then cleared
  uint32_t* last;                                  // kExBins words: the histogram of this call
  ExRecord* rec;
  ExConst k;
};

__global__ void __launch_bounds__(kBlock) k_ex_resolve(ExResolveArgs a) {
  __shared__ uint32_t s_scan[kExBins];
  __shared__ double s_term[kExBins];
  const uint32_t b = threadIdx.x;                  // kBlock == kExBins
  const uint32_t n = a.hist[b];
  s_scan[b] = n;
  __syncthreads();
  for (uint32_t d = 1; d < kExBins; d <<= 1) {     // inclusive scan (at most 2^28 pixels: no overflow)
    const uint32_t v = b >= d ? s_scan[b - d] : 0u;
    __syncthreads();
    s_scan[b] += v;
    __syncthreads();
  }
  const uint64_t N = s_scan[kExBins - 1u];
  const ExTrim t = exTrim(N, a.k);
  s_term[b] = exTerm(b, uint64_t(s_scan[b] - n), n, t, a.k);
  const uint32_t ignored = a.hist[kExBins];
  __syncthreads();
  a.last[b] = n;
  a.hist[b] = 0u;
  if (b == 0) {
    a.hist[kExBins] = 0u;
    double S = 0.0;
    for (uint32_t j = 0; j < kExBins; j++) S += s_term[j];
    ExRecord r = *a.rec;
    exStep(r, S, N, ignored, t, a.k);
    *a.rec = r;
  }
}

struct ExApplyArgs {
  const f4* rgba;
  const ExRecord* rec;
  f4* ldr;                                         // LDR only
  uint8_t* rgb8;                                   // RGB8 only
  uint32_t n;
  int look;
};

template <bool LDR, bool RGB8>
__global__ void __launch_bounds__(kBlock) k_ex_apply(ExApplyArgs a) {
  const float gain = a.rec->gain;
  const AgxLook lk = agxLook(a.look);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    const f4 o = exApply(dnLd(a.rgba + i), gain, a.look, lk);
    if (LDR) dnSt(a.ldr + i, o);
    if (RGB8) {
      a.rgb8[3 * size_t(i)] = ppmByte(o.x); a.rgb8[3 * size_t(i) + 1] = ppmByte(o.y); a.rgb8[3 * size_t(i) + 2] = ppmByte(o.z);
    }
  }
}
