// moment_kernels.inc — per-pixel sample moments (YART_MOMENT_*), device side (included by yart_hip.hip, unit 0, next to
// aov_kernels.inc). The arithmetic is moments.hpp; the definition is the header comment of include/yart_hip.h.
//
//   k_moments_accumulate  launched next to k_gmon_blend over the same per-(pixel, sample) radiance records L (pixel-major, spp
//                         consecutive 16-byte records per pixel of the batch): adds the wave's samples of every pixel of the batch,
//                         in ASCENDING sample order, onto the pixel's running state (MomentState, 48 bytes per pixel of the rank,
//                         indexed pixBase + pixel like the feature buffers' sums) — so a pixel whose samples span waves or batches
//                         still sums in ascending s. The serial order per pixel is the constraint: 16 lanes per pixel load 16
//                         consecutive records at once (256 contiguous bytes per pixel, 1 KB per wave and load), each lane forms
//                         w, y and the accept bit of its own record, and lane 0 of the group takes them one by one through
//                         cross-lane moves (4 floats + 1 bit per sample) and does the five binary64 additions.
//   k_moments_finish      after the last wave: one lane per pixel of the rank, mean / variance / count scattered into the caller's
//                         buffers through the rank's pixel list.
//
// No LDS, no scratch memory; none of the existing kernels changes: without a moment mask none of these is launched.

struct MomentArgs {
  const f4* L;                 // per (pixel, sample) of the batch: radiance.xyz, ray count (not read)
  MomentState* state;          // per pixel of the rank
  uint32_t nPixels, spp, pixBase, pad;   // the batch: pixels, samples of the wave, index of its first pixel
  float exposureScale;
};

constexpr int kMomentLanes = 16;
constexpr int kMomentPixPerBlock = kBlock / kMomentLanes;
__global__ void __launch_bounds__(kBlock) k_moments_accumulate(MomentArgs a) {
  const uint32_t sub = threadIdx.x & (kMomentLanes - 1);
  const uint32_t pi = blockIdx.x * kMomentPixPerBlock + threadIdx.x / kMomentLanes;
  const bool valid = pi < a.nPixels;     // (the same for the 16 lanes of a group; no lane leaves before the cross-lane moves)
  const f4* p = a.L + size_t(valid ? pi : 0u) * a.spp;
  MomentState st{};
  if (valid && sub == 0u) st = a.state[a.pixBase + pi];
  for (uint32_t s0 = 0; s0 < a.spp; s0 += kMomentLanes) {
    const uint32_t s = s0 + sub;
    const bool have = valid && s < a.spp;
    f4 q; q.x = q.y = q.z = q.w = 0.0f;
    if (have) q = wfLd(p + s);
    const MomentSample m = momentSample(mk3(q.x, q.y, q.z), a.exposureScale);
    const int ok = have && m.ok ? 1 : 0;
    const uint32_t cnt = a.spp - s0 < uint32_t(kMomentLanes) ? a.spp - s0 : uint32_t(kMomentLanes);   // (uniform over the grid)
    for (uint32_t k = 0; k < cnt; k++) {
      const float wr = __shfl(m.w.x, int(k), kMomentLanes), wg = __shfl(m.w.y, int(k), kMomentLanes);
      const float wb = __shfl(m.w.z, int(k), kMomentLanes), y = __shfl(m.y, int(k), kMomentLanes);
      const int okk = __shfl(ok, int(k), kMomentLanes);
      if (sub == 0u && okk) momentAdd(st, wr, wg, wb, y);
    }
  }
  if (valid && sub == 0u) a.state[a.pixBase + pi] = st;
}

struct MomentFinishArgs {
  const MomentState* state;
  const uint32_t* pixels;
  uint32_t nPixels, width, mask, pad;
  float *mean, *variance;      // identity pixel list (pixels == nullptr): index = pixel
  uint32_t* count;
};
__global__ void __launch_bounds__(kBlock) k_moments_finish(MomentFinishArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nPixels) return;
  size_t o = i;
  if (a.pixels) {
    const uint32_t pk = a.pixels[i];
    o = size_t(pk >> 16) * a.width + (pk & 0xffffu);
  }
  float mean[3], variance;
  uint32_t count;
  momentFinish(a.state[i], mean, variance, count);
  if (a.mask & YART_MOMENT_MEAN) { a.mean[3 * o] = mean[0]; a.mean[3 * o + 1] = mean[1]; a.mean[3 * o + 2] = mean[2]; }
  if (a.mask & YART_MOMENT_VARIANCE) a.variance[o] = variance;
  if (a.mask & YART_MOMENT_COUNT) a.count[o] = count;
}
