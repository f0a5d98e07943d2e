// aov_kernels.inc — first-hit feature buffers (YART_AOV_*), device side (included by yart_hip.hip, unit 0).
//
//   k_aov_capture   after bounce 0's closest-hit stage (lean + retry + general kernels done: hit0 / hit1 are final) and before
//                   k_wf_shade consumes them: one streaming pass over the paths that stand at bounce 0 — ray, hit record ->
//                   finalizeHit + matBase (aov.hpp) -> one 48-byte AovRecord per path; the ids of sample 0 go to the pixel.
//                   Batch-synchronous pipeline: slot = path, and the records are written into sh0 / sh1 / sh2 — the shadow-ray
//                   arrays, which nothing reads or writes before bounce 0's shade stage — so the capture holds no memory of its
//                   own. Path pool: every round, over the slots whose path has depth 0 (started by this round's k_wf_refill),
//                   into record arrays of the batch's size (path index = slotMap[slot]).
//                   (The megakernel writes the same record from its loop: k_render_mega<true>.)
//   k_aov_reduce    per pixel of the batch the float32 sums of its records in ASCENDING sample order — the order is the
//                   contract: the result is a pure function of the per-sample values — on top of the running sums of the
//                   earlier waves (per pixel of the rank). Three lanes per pixel, one per record word: each reads spp
//                   consecutive 16-byte words. Runs right after the capture (batch-synchronous) or at the end of the batch.
//   k_aov_add_rays  adds the wave's per-pixel ray counts (k_gmon_blend's pixRays) to the pixel's total
//   k_aov_finish    after the last wave: one division by float(samples) per channel, scattered into the caller's buffers
//
// None of the existing kernels changes: without feature buffers none of these is launched.

struct AovArgs {
  f4 *r0, *r1, *r2;            // records, per path of the batch (index pixel-in-batch * spp + sample-in-wave)
  f4 *acc0, *acc1, *acc2;      // running sums per pixel of the rank: {albedo.xyz, depth} {n.xyz, hits (u32)} {p.xyz, -}
  uint32_t* accRays;           // per pixel of the rank
  int32_t* ids;                // per pixel of the rank: node, mesh, material, triangle of sample 0
  uint32_t nPixels, spp, pixBase, sampleOffset;   // the batch: pixels, samples of the wave, index of its first pixel, first sample
};

__global__ void __launch_bounds__(kBlock) k_aov_capture(WfArgs a, AovArgs v) {
  const uint32_t n = a.poolSlots ? a.poolSlots : a.nPaths;
  for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < n; slot += gridDim.x * blockDim.x) {
    uint32_t path = slot;
    if (a.poolSlots) {
      path = a.slotMap[slot];
      if (path == kWfFreeSlot || (asU(wfLd1(&a.st.acc[slot].w)) & WF_DEPTH_MASK) != 0u) continue;
    }
    const f4 r0 = wfLd(a.st.ray0 + slot), r1 = wfLd(a.st.ray1 + slot), h0 = wfLd(a.st.hit0 + slot);
    const uint32_t word = asU(wfLd1(&a.st.hit1[slot].x));
    HitRec hr;                               // (unpacked as wfShade does)
    hr.t = h0.x; hr.u = h0.y; hr.v = h0.z; hr.tri = asU(h0.w); hr.node = word & ((1u << kWfNodeBits) - 1u);
    hr.backSide = (word >> 31) | (((word >> kWfNodeBits) & kWfClassMiss) << 1);
    AovIds ids;
    const AovRecord rec = aovCapture(a.sc, hr, !(h0.x < 0.0f), mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), ids);
    wfSt(v.r0 + path, rec.r0); wfSt(v.r1 + path, rec.r1); wfSt(v.r2 + path, rec.r2);
    const uint32_t pi = path / a.spp, s = path - pi * a.spp;
    if (s + a.sampleOffset == 0u) {
      int32_t* o = v.ids + size_t(a.pixBase + pi) * 4;
      o[0] = ids.node; o[1] = ids.mesh; o[2] = ids.material; o[3] = ids.tri;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_aov_reduce(AovArgs v) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t pi = t >> 2, j = t & 3u;
  if (pi >= v.nPixels || j == 3u) return;
  const f4* r = (j == 0u ? v.r0 : j == 1u ? v.r1 : v.r2) + size_t(pi) * v.spp;
  f4* accp = (j == 0u ? v.acc0 : j == 1u ? v.acc1 : v.acc2) + (v.pixBase + pi);
  f4 acc = *accp;
  uint32_t hits = asU(acc.w);                // (j == 1)
  auto add = [&](const f4& q) {
    // word 0 carries t (-1: miss), words 1 and 2 the hit flag; a miss contributes nothing
    if (j == 0u ? !(q.w >= 0.0f) : asU(q.w) == 0u) return;
    acc.x += q.x; acc.y += q.y; acc.z += q.z;
    if (j == 0u) acc.w += q.w;
    hits++;
  };
  uint32_t s = 0;
  for (; s + 4u <= v.spp; s += 4u) {         // four loads in flight, added in order
    f4 q[4];
    for (uint32_t k = 0; k < 4u; k++) q[k] = wfLd(r + s + k);
    for (uint32_t k = 0; k < 4u; k++) add(q[k]);
  }
  for (; s < v.spp; s++) add(wfLd(r + s));
  if (j == 1u) acc.w = asF(hits);
  *accp = acc;
}

__global__ void __launch_bounds__(kBlock) k_aov_add_rays(uint32_t* accRays, const uint32_t* pixRays, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) accRays[i] += pixRays[i];
}

struct AovFinishArgs {
  const f4 *acc0, *acc1, *acc2;
  const uint32_t* accRays;
  const int32_t* ids;
  const uint32_t* pixels;
  uint32_t nPixels, width, samples, mask;
  float *albedo, *normal, *position, *depth, *coverage;
  int32_t* outIds;
  uint32_t* outRays;
};
__global__ void __launch_bounds__(kBlock) k_aov_finish(AovFinishArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nPixels) return;
  const uint32_t pk = a.pixels[i];
  const size_t o = size_t(pk >> 16) * a.width + (pk & 0xffffu);
  const float n = float(a.samples);
  const f4 a0 = a.acc0[i], a1 = a.acc1[i], a2 = a.acc2[i];
  if (a.mask & YART_AOV_ALBEDO) { a.albedo[3 * o] = a0.x / n; a.albedo[3 * o + 1] = a0.y / n; a.albedo[3 * o + 2] = a0.z / n; }
  if (a.mask & YART_AOV_NORMAL) { a.normal[3 * o] = a1.x / n; a.normal[3 * o + 1] = a1.y / n; a.normal[3 * o + 2] = a1.z / n; }
  if (a.mask & YART_AOV_POSITION) { a.position[3 * o] = a2.x / n; a.position[3 * o + 1] = a2.y / n; a.position[3 * o + 2] = a2.z / n; }
  if (a.mask & YART_AOV_DEPTH) a.depth[o] = a0.w / n;
  if (a.mask & YART_AOV_COVERAGE) a.coverage[o] = float(asU(a1.w)) / n;
  if (a.mask & YART_AOV_IDS) for (int k = 0; k < 4; k++) a.outIds[4 * o + k] = a.ids[4 * size_t(i) + k];
  if (a.mask & YART_AOV_RAYS) a.outRays[o] = a.accRays[i];
}

// diagnostic (yart_hip_probe_camera_rays): the camera ray of (x, y, sample) as bounce 0 draws it (wfGenerate / samplePixel)
struct ProbeCameraArgs { CameraDev cam; RenderConst rc; const uint32_t* sobol; const uint32_t* xys; uint32_t n, pad; float* out; };
__global__ void __launch_bounds__(kBlock) k_probe_camera_rays(ProbeCameraArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t px = a.xys[3 * i], py = a.xys[3 * i + 1];
  Sampler smp;
  startPixelSample(smp, a.rc.sampler, px, py, a.xys[3 * i + 2]);
  const f2 uvFilm = get2D(smp, a.rc.sampler, a.sobol);
  const f2 uvLens = get2D(smp, a.rc.sampler, a.sobol);
  f3 o, d;
  cameraRay(a.cam, px, py, uvFilm, uvLens, o, d);
  float* q = a.out + size_t(i) * 6;
  q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = d.x; q[4] = d.y; q[5] = d.z;
}
