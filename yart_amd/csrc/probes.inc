// probes.inc — diagnostics for the parity tests: the kernels k_probe_* and the yart_hip_probe_* entries of the C ABI, each of
// which runs one piece of the device code on caller-supplied input (included by yart_hip.hip, unit 0, last: the entries use
// YartScene, guarded, validate and the kernels of stream_kernels.inc, aov_kernels.inc and moment_kernels.inc).
#include "tonemap.hpp"         // (ypowf, for k_probe_math)
#include "probe_record.hpp"
#include "shade_record.hpp"

namespace {

struct ProbeSampleArgs {
  SceneDev sc; CameraDev cam; RenderConst rc;
  const uint32_t* xys; uint32_t n; float* out; unsigned long long* rays; uint64_t* spill;
};
__global__ void __launch_bounds__(kBlock) k_probe_samples(ProbeSampleArgs a) {
  __shared__ uint64_t ldsStack[kLdsStack * kBlock];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  PathCtx cx;
  cx.sc = &a.sc;
  cx.sobol = reinterpret_cast<const uint32_t*>(a.sc.lut + LutDev::sobol);
  cx.stk.lds = (lds_u64*)(ldsStack + threadIdx.x); cx.stk.ldsStride = kBlock; cx.stk.ldsDepth = kLdsStack;
  cx.stk.spill = a.spill + gtid; cx.stk.spillStride = gridDim.x * blockDim.x;
  cx.rc = a.rc;
  if (gtid >= a.n) return;
  uint32_t rays = 0;
  f3 L = samplePixel(cx, a.cam, a.xys[gtid * 3], a.xys[gtid * 3 + 1], a.xys[gtid * 3 + 2], rays);
  a.out[gtid * 3] = L.x; a.out[gtid * 3 + 1] = L.y; a.out[gtid * 3 + 2] = L.z;
  atomicAdd(a.rays, (unsigned long long) rays);
}

// the sampler alone (diagnostic): per case startPixelSample + a pattern of draws (1 = get1D, 2 = get2D); with `tab` set the
// draws go through the per-render sampler tables exactly as the wavefront kernels' do
struct ProbeSamplerArgs { SamplerConfig cfg; const uint32_t* sobol; const uint32_t* cases; uint32_t n, nDraws, nOut, pad; const uint8_t* pattern; float* out; };
__global__ void __launch_bounds__(kBlock) k_probe_sampler(ProbeSamplerArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  Sampler s;
  startPixelSample(s, a.cfg, a.cases[3 * i], a.cases[3 * i + 1], a.cases[3 * i + 2]);
  s.pix = i;                                                 // (sampler tables: one pixel column per case)
  float* o = a.out + size_t(i) * a.nOut;
  for (uint32_t k = 0; k < a.nDraws; k++) {
    if (a.pattern[k] == 2) { const f2 v = get2D(s, a.cfg, a.sobol); *o++ = v.x; *o++ = v.y; }
    else *o++ = get1D(s, a.cfg);
  }
}

struct ProbeHitArgs { SceneDev sc; const float* rays; uint32_t n; float* out; uint64_t* spill; };
__global__ void __launch_bounds__(kBlock) k_probe_hits(ProbeHitArgs a) {
  __shared__ uint64_t ldsStack[kLdsStack * kBlock];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = kLdsStack;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  if (gtid >= a.n) return;
  const float* r = a.rays + size_t(gtid) * 6;
  f3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
  HitRec hr; hr.t = kInf; hr.u = hr.v = 0; hr.tri = 0; hr.node = 0; hr.backSide = 0;
  f3 att = mk3(1.0f);
  Sampler dummy; dummy.dim = 0; dummy.morton = 0;
  AlphaCtx ac; ac.sampler = &dummy; ac.cfg.log2spp = 0; ac.cfg.nBase4Digits = 6;
  bool hit = traverseScene<false>(a.sc, o, d, 0.001f, hr, att, stk, ac);
  float* q = a.out + size_t(gtid) * 16;
  for (int i = 0; i < 16; i++) q[i] = 0.0f;
  q[0] = hit ? 1.0f : 0.0f;
  if (hit) {
    Hit h = finalizeHit(a.sc, hr, o, d);
    q[1] = h.t; q[2] = hr.u; q[3] = hr.v;
    q[4] = h.p.x; q[5] = h.p.y; q[6] = h.p.z; q[7] = h.n.x; q[8] = h.n.y; q[9] = h.n.z;
    q[10] = h.tg.x; q[11] = h.tg.y; q[12] = h.tg.z;
    q[13] = float(localTri(a.sc, hr)); q[14] = float(h.lightIdx); q[15] = h.backSide ? 1.0f : 0.0f;
  }
}

// one walk of traverseScene per caller-supplied ray record (yart_hip_probe_rays, include/yart_hip.h; probe_record.hpp): MODE is
// the instantiation, the ray's kind word picks the <false> / <true> form, the sampler is the render's
struct ProbeRayArgs { SceneDev sc; SamplerConfig cfg; const uint32_t* rays; uint32_t n; uint32_t* out; uint64_t* spill; };
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_probe_rays(ProbeRayArgs a) {
  __shared__ uint64_t ldsStack[kLdsStack * kBlock];
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  TravStack stk;
  stk.lds = (lds_u64*)(ldsStack + threadIdx.x); stk.ldsStride = kBlock; stk.ldsDepth = kLdsStack;
  stk.spill = a.spill + gtid; stk.spillStride = gridDim.x * blockDim.x;
  if (gtid >= a.n) return;
  probeRayRecord<MODE>(a.sc, a.cfg, stk, a.rays + size_t(gtid) * 12, a.out + size_t(gtid) * 20);
}

// one case of the shading code per thread (yart_hip_probe_shading, include/yart_hip.h; shade_record.hpp): bsdf.hpp / lights.hpp as
// the render kernels include them, in the forms only the device runs. The LDS set-up repeats k_wf_shade's (wavefront_kernels.inc):
// form bit 1 hands the functions the LDS copy of the glossy lobes' GGX tables with the tables' address behind it, bit 2 repoints the
// scene's small record tables to LDS copies where they fit the shade kernel's slots (generic pointers, as its non-FIT form does),
// bit 4 sends a BSDF case through matEvaluate and the *ImplE entries.
struct ProbeShadeArgs { SceneDev sc; const uint32_t* cases; uint32_t n, form; uint32_t* out; };
__global__ void __launch_bounds__(kBlock) k_probe_shading(ProbeShadeArgs a) {
  __shared__ float sLut[LutDev::glassE + 2];
  __shared__ __attribute__((aligned(16))) uint32_t sMat[kShadeMatSlots * sizeof(MaterialDev) / 4], sTex[kShadeTexSlots * sizeof(TexDev) / 4],
      sLight[kShadeLightSlots * sizeof(LightDev) / 4], sEnv[kShadeEnvSlots * sizeof(EnvDev) / 4], sInf[kShadeLightSlots];
  if (a.form & SHADE_FORM_LDS_LUT) {
    const float* g = a.sc.lut;
    for (uint32_t k = threadIdx.x; k < LutDev::glassE; k += blockDim.x) sLut[k] = g[k];
    if (threadIdx.x == 0) {
      const uint64_t p = reinterpret_cast<uint64_t>(g);
      reinterpret_cast<uint32_t*>(sLut)[LutDev::glassE] = uint32_t(p); reinterpret_cast<uint32_t*>(sLut)[LutDev::glassE + 1] = uint32_t(p >> 32);
    }
    __syncthreads();
    a.sc.lut = sLut;
  }
  if (a.form & SHADE_FORM_LDS_RECORDS) {
    const bool mOk = a.sc.nMaterials <= kShadeMatSlots, tOk = a.sc.nTextures <= kShadeTexSlots, lOk = a.sc.nLights <= kShadeLightSlots && a.sc.nLights > 0u,
               eOk = a.sc.nEnvs <= kShadeEnvSlots, iOk = a.sc.nInfinite <= kShadeLightSlots && a.sc.nInfinite > 0u;
    if (mOk) ldsCopyWords(sMat, a.sc.materials, a.sc.nMaterials * uint32_t(sizeof(MaterialDev) / 4));
    if (tOk) ldsCopyWords(sTex, a.sc.textures, a.sc.nTextures * uint32_t(sizeof(TexDev) / 4));
    if (lOk) ldsCopyWords(sLight, a.sc.lights, a.sc.nLights * uint32_t(sizeof(LightDev) / 4));
    if (eOk) ldsCopyWords(sEnv, a.sc.envs, a.sc.nEnvs * uint32_t(sizeof(EnvDev) / 4));
    if (iOk) ldsCopyWords(sInf, a.sc.infiniteLights, a.sc.nInfinite);
    __syncthreads();
    if (mOk) a.sc.materials = reinterpret_cast<const MaterialDev*>(sMat);
    if (tOk) a.sc.textures = reinterpret_cast<const TexDev*>(sTex);
    if (lOk) a.sc.lights = reinterpret_cast<const LightDev*>(sLight);
    if (eOk) a.sc.envs = reinterpret_cast<const EnvDev*>(sEnv);
    if (iOk) a.sc.infiniteLights = sInf;
  }
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  shadeCaseRecord(a.sc, a.cases + size_t(i) * 32, (a.form & SHADE_FORM_IMPL_E) != 0u, a.out + size_t(i) * 32);
}

// the math the frames rest on, one function at a time (diagnostic, yart_hip_probe_math[_pairs]): the very inline functions the
// render kernels call (ymath.hpp, libm_pow.hpp via tonemap.hpp) and the fp32 divide / sqrt / bit reversal as this build compiles them
struct ProbeMathArgs { int fn; uint32_t firstBits; uint64_t n; float y; const float* a; const float* b; float* out; };
YART_HD float probeMathEval(int fn, float a, float b) {   // (host + device only so that the host pass resolves the names)
  switch (fn) {
    case YART_MATH_SINF: return ysinf(a);
    case YART_MATH_COSF: return ycosf(a);
    case YART_MATH_SINF_2PI: return ysinf2pi(a);
    case YART_MATH_COSF_2PI: return ycosf2pi(a);
    case YART_MATH_LOGF: return ylogf(a);
    case YART_MATH_EXPF: return yexpf(a);
    case YART_MATH_LOG2F: return ylog2f(a);
    case YART_MATH_POWF: return ypowf(a, b);
    case YART_MATH_DIV: return a / b;
    case YART_MATH_SQRT: return sqrtf(a);
    default: return __builtin_bit_cast(float, reverseBits32(__builtin_bit_cast(uint32_t, a)));   // YART_MATH_BREV
  }
}
__global__ void __launch_bounds__(kBlock) k_probe_math(ProbeMathArgs q) {
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < q.n; i += stride) {
    const float a = q.a ? q.a[i] : __builtin_bit_cast(float, q.firstBits + uint32_t(i));
    const float b = q.b ? q.b[i] : q.y;
    q.out[i] = probeMathEval(q.fn, a, b);
  }
}

}  // namespace

extern "C" {

int yart_hip_probe_samples(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                           uint32_t n, const uint32_t* xys, float* out_rgb, uint64_t* out_rays) {
  return guarded([&] {
    require(scene && xys && out_rgb, "null pointer");
    validate(cam, params);
    if (n == 0) return;
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    HIP_CHECK(hipSetDevice(s.device));
    const int grid = int((n + kBlock - 1) / kBlock);
    s.spill.ensure(size_t(grid) * kBlock * spillDepthFor(s.host, false));
    s.probeIn.ensure(size_t(n) * 3); s.probeOut.ensure(size_t(n) * 3); s.counters.ensure(8);
    HIP_CHECK(hipMemcpy(s.probeIn.p, xys, size_t(n) * 3 * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(s.counters.p, 0, 8 * sizeof(unsigned long long)));
    ProbeSampleArgs a{};
    a.sc = s.dev; a.cam = makeCamera(*cam); a.rc = makeRenderConst(*params);
    a.xys = s.probeIn.p; a.n = n; a.out = s.probeOut.p; a.rays = s.counters.p; a.spill = s.spill.p;
    hipLaunchKernelGGL(k_probe_samples, dim3(grid), dim3(kBlock), 0, nullptr, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_rgb, s.probeOut.p, size_t(n) * 3 * 4, hipMemcpyDeviceToHost));
    if (out_rays) {
      unsigned long long r = 0;
      HIP_CHECK(hipMemcpy(&r, s.counters.p, sizeof(r), hipMemcpyDeviceToHost));
      *out_rays = r;
    }
  });
}

int yart_hip_probe_scene_graph(YartScene* scene, void* nodes_out, float* node_world_out, void* tlas_out, uint32_t* n_tlas_out) {
  return guarded([&] {
    require(scene, "probe_scene_graph: scene pointer is null");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    HIP_CHECK(hipSetDevice(s.device));
    const size_t nn = s.host.nodes.size();
    if (nodes_out) HIP_CHECK(hipMemcpy(nodes_out, s.nodes.p, nn * sizeof(NodeDev), hipMemcpyDeviceToHost));
    if (node_world_out) HIP_CHECK(hipMemcpy(node_world_out, s.nodeWorld.p, nn * 2u * sizeof(f4), hipMemcpyDeviceToHost));
    if (tlas_out && s.dev.nTlas) HIP_CHECK(hipMemcpy(tlas_out, s.tlas.p, size_t(s.dev.nTlas) * sizeof(TlasNode), hipMemcpyDeviceToHost));
    if (n_tlas_out) *n_tlas_out = s.dev.nTlas;
  });
}

int yart_hip_probe_hits(YartScene* scene, uint32_t n, const float* rays, float* out) {
  return guarded([&] {
    require(scene && rays && out, "null pointer");
    if (n == 0) return;
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    HIP_CHECK(hipSetDevice(s.device));
    const int grid = int((n + kBlock - 1) / kBlock);
    s.spill.ensure(size_t(grid) * kBlock * spillDepthFor(s.host, false));
    DevBuf<float> in, res;
    in.ensure(size_t(n) * 6); res.ensure(size_t(n) * 16);
    HIP_CHECK(hipMemcpy(in.p, rays, size_t(n) * 6 * 4, hipMemcpyHostToDevice));
    ProbeHitArgs a{};
    a.sc = s.dev; a.rays = in.p; a.n = n; a.out = res.p; a.spill = s.spill.p;
    hipLaunchKernelGGL(k_probe_hits, dim3(grid), dim3(kBlock), 0, nullptr, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, res.p, size_t(n) * 16 * 4, hipMemcpyDeviceToHost));
  });
}

int yart_hip_probe_rays(YartScene* scene, const YartRenderParams* params, uint32_t n, const uint32_t* rays, int walk, uint32_t* out) {
  return guarded([&] {
    require(scene && params && rays && out, "probe_rays: null pointer");
    require(walk >= 0 && walk <= 2, "probe_rays: walk must be 0 (general), 1 (fast) or 2 (fast, identity)");
    require(params->samples > 0 && params->tile_size > 0 && params->tile_size <= 4096, "probe_rays: samples / tile_size out of range");
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t* q = rays + size_t(i) * 12;
      require(q[7] <= 1u, "probe_rays: kind must be 0 (closest hit) or 1 (occlusion)");
      require(q[8] < 65536u && q[9] < 65536u && q[10] < params->samples, "probe_rays: pixel / sample out of range");
    }
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    require(walk != 2 || s.host.allIdentity, "probe_rays: walk 2 (TRAV_IDENTITY) needs a scene whose node chains are all the identity");
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(s.device));
    const int grid = int((n + kBlock - 1) / kBlock);
    s.spill.ensure(size_t(grid) * kBlock * spillDepthFor(s.host, false));
    DevBuf<uint32_t> in, res;
    in.ensure(size_t(n) * 12); res.ensure(size_t(n) * 20);
    HIP_CHECK(hipMemcpy(in.p, rays, size_t(n) * 12 * 4, hipMemcpyHostToDevice));
    ProbeRayArgs a{};
    a.sc = s.dev; a.cfg = makeRenderConst(*params).sampler; a.rays = in.p; a.n = n; a.out = res.p; a.spill = s.spill.p;
    if (walk == 0) hipLaunchKernelGGL(k_probe_rays<TRAV_GENERAL>, dim3(grid), dim3(kBlock), 0, nullptr, a);
    else if (walk == 1) hipLaunchKernelGGL(k_probe_rays<TRAV_FAST>, dim3(grid), dim3(kBlock), 0, nullptr, a);
    else hipLaunchKernelGGL((k_probe_rays<TRAV_FAST | TRAV_IDENTITY>), dim3(grid), dim3(kBlock), 0, nullptr, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, res.p, size_t(n) * 20 * 4, hipMemcpyDeviceToHost));
  });
}

int yart_hip_probe_shading(YartScene* scene, uint32_t n, const uint32_t* cases, uint32_t form, uint32_t* out) {
  return guarded([&] {
    require(scene && cases && out, "probe_shading: null pointer");
    require((form & ~SHADE_FORM_ALL) == 0u, "probe_shading: unknown form bits (1 LDS tables, 2 LDS records, 4 matEvaluate + *ImplE)");
    require(n <= (1u << 20), "probe_shading: more than 2^20 cases");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    // everything a case names is checked against the scene before a device is touched: no lane reads outside the scene
    std::vector<uint32_t> dims;
    for (const TexDev& t : s.host.textures) { dims.push_back(t.width); dims.push_back(t.height); }
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t* q = cases + size_t(i) * 32;
      if (const char* why = shadeCaseProblem(q, s.host.nMaterials, uint32_t(s.host.textures.size()), s.host.nLights, dims.data()))
        throw std::invalid_argument(std::string("probe_shading: case ") + std::to_string(i) + ": " + why);
      // (a texture that only material bundles sample has no footprint records of its own, host_scene.hpp)
      require(q[0] != SHADE_TEX || s.dev.texQuads == nullptr || s.host.textures[q[1]].quadOffset != kNoTexQuads,
              "probe_shading: a TEX case names a texture without footprint records of its own");
    }
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(s.device));
    DevBuf<uint32_t> in, res;
    in.ensure(size_t(n) * 32); res.ensure(size_t(n) * 32);
    HIP_CHECK(hipMemcpy(in.p, cases, size_t(n) * 32 * 4, hipMemcpyHostToDevice));
    ProbeShadeArgs a{};
    a.sc = s.dev; a.cases = in.p; a.n = n; a.form = form; a.out = res.p;
    hipLaunchKernelGGL(k_probe_shading, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, res.p, size_t(n) * 32 * 4, hipMemcpyDeviceToHost));
  });
}

int yart_hip_probe_camera_rays(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, uint32_t n,
                               const uint32_t* xys, float* out_rays) {
  return guarded([&] {
    require(scene && xys && out_rays && n > 0, "probe_camera_rays: null pointer or n == 0");
    validate(cam, params);
    for (uint32_t i = 0; i < n; i++)
      require(xys[3 * i] < cam->width && xys[3 * i + 1] < cam->height && xys[3 * i + 2] < params->samples, "probe_camera_rays: pixel / sample out of range");
    YartScene& s = *scene;
    std::lock_guard<std::mutex> lk(s.mu);
    HIP_CHECK(hipSetDevice(s.device));
    DevBuf<uint32_t> dIn; DevBuf<float> dOut;
    dIn.upload(std::vector<uint32_t>(xys, xys + size_t(n) * 3));
    dOut.ensure(size_t(n) * 6);
    ProbeCameraArgs a{};
    a.cam = makeCamera(*cam); a.rc = makeRenderConst(*params);
    a.sobol = reinterpret_cast<const uint32_t*>(s.dev.lut + LutDev::sobol);
    a.xys = dIn.p; a.n = n; a.out = dOut.p;
    hipLaunchKernelGGL(k_probe_camera_rays, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_rays, dOut.p, size_t(n) * 6 * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int yart_hip_probe_sampler(YartScene* scene, uint32_t spp, uint32_t tile, uint32_t n, const uint32_t* cases, uint32_t n_draws,
                           const uint8_t* pattern, int use_tables, float* out) {
  return guarded([&] {
    require(scene && cases && pattern && out && n > 0 && n_draws > 0 && n_draws <= 64 && spp > 0 && tile > 0, "probe_sampler: bad argument");
    YartScene& s = *scene;
    std::lock_guard<std::mutex> lk(s.mu);
    HIP_CHECK(hipSetDevice(s.device));
    uint32_t nOut = 0;
    for (uint32_t k = 0; k < n_draws; k++) { require(pattern[k] == 1 || pattern[k] == 2, "probe_sampler: pattern entries are 1 or 2"); nOut += pattern[k]; }
    for (uint32_t i = 0; i < n; i++) require(cases[3 * i] < 65536u && cases[3 * i + 1] < 65536u && cases[3 * i + 2] < spp, "probe_sampler: pixel / sample out of range");
    DevBuf<uint32_t> dCases; DevBuf<uint8_t> dPat; DevBuf<float> dOut;
    dCases.upload(std::vector<uint32_t>(cases, cases + size_t(n) * 3)); dPat.upload(std::vector<uint8_t>(pattern, pattern + n_draws));
    dOut.ensure(size_t(n) * nOut);
    ProbeSamplerArgs a{};
    a.cfg = makeSamplerConfig(spp, tile);
    a.sobol = reinterpret_cast<const uint32_t*>(s.dev.lut + LutDev::sobol);
    a.cases = dCases.p; a.n = n; a.nDraws = n_draws; a.nOut = nOut; a.pattern = dPat.p; a.out = dOut.p;
    DevBuf<uint32_t> dPix; DevBuf<uint64_t> entries, hash; DevBuf<uint32_t> sobol1;
    if (use_tables) {
      // the tables of a render whose pixel list is the cases' pixels (k_sampler_tables, as renderToDevice builds them)
      require(uint64_t(spp) <= (1ull << a.cfg.log2spp), "probe_sampler: the sampler tables need spp <= 2^log2spp");
      std::vector<uint32_t> pix(n);
      for (uint32_t i = 0; i < n; i++) pix[i] = cases[3 * i] | (cases[3 * i + 1] << 16);
      dPix.upload(pix);
      const uint32_t dims = 256u;
      entries.ensure(size_t(dims) * n); hash.ensure(dims + 3); sobol1.ensure(8 * 256);
      SamplerTabArgs ta{};
      ta.cfg = a.cfg; ta.pixels = dPix.p; ta.nPixels = n; ta.dims = dims; ta.entries = entries.p; ta.hash = hash.p; ta.sobol1 = sobol1.p;
      ta.matrix52 = a.sobol;
      hipLaunchKernelGGL(k_sampler_tables, dim3(64), dim3(kBlock), 0, nullptr, ta);
      HIP_CHECK(hipGetLastError());
      a.cfg.tab.entries = entries.p; a.cfg.tab.hash = hash.p; a.cfg.tab.sobol1 = sobol1.p; a.cfg.tab.dims = dims; a.cfg.tab.stride = n;
    }
    hipLaunchKernelGGL(k_probe_sampler, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dOut.p, size_t(n) * nOut * 4, hipMemcpyDeviceToHost));
  });
}

namespace {
constexpr uint64_t kProbeMathMax = 1ull << 28;   // results per call: 1 GiB of device memory
void probeMath(int fn, uint32_t firstBits, uint64_t n, float y, const float* a, const float* b, float* out) {
  HIP_CHECK(hipSetDevice(0));
  DevBuf<float> dA, dB, dOut;
  dOut.ensure(size_t(n));
  if (a) { dA.ensure(size_t(n)); HIP_CHECK(hipMemcpy(dA.p, a, size_t(n) * 4, hipMemcpyHostToDevice)); }
  if (b) { dB.ensure(size_t(n)); HIP_CHECK(hipMemcpy(dB.p, b, size_t(n) * 4, hipMemcpyHostToDevice)); }
  ProbeMathArgs q{};
  q.fn = fn; q.firstBits = firstBits; q.n = n; q.y = y; q.a = dA.p; q.b = dB.p; q.out = dOut.p;
  const uint64_t blocks = std::min<uint64_t>((n + kBlock - 1) / kBlock, 1u << 16);
  hipLaunchKernelGGL(k_probe_math, dim3(uint32_t(blocks)), dim3(kBlock), 0, nullptr, q);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(out, dOut.p, size_t(n) * 4, hipMemcpyDeviceToHost));
}
}  // namespace

int yart_hip_probe_math(int fn, uint32_t first_bits, uint64_t count, float y, float* out_host) {
  return guarded([&] {
    require(fn >= 0 && fn < YART_MATH_COUNT, "probe_math: unknown function");
    require(fn != YART_MATH_DIV, "probe_math: the divide takes explicit operands (yart_hip_probe_math_pairs)");
    require(out_host && count > 0 && count <= kProbeMathMax, "probe_math: null output, count == 0 or count > 2^28");
    require(uint64_t(first_bits) + count <= (1ull << 32), "probe_math: the range runs past the last bit pattern");
    probeMath(fn, first_bits, count, y, nullptr, nullptr, out_host);
  });
}

int yart_hip_probe_math_pairs(int fn, uint64_t n, const float* a, const float* b, float* out_host) {
  return guarded([&] {
    require(fn >= 0 && fn < YART_MATH_COUNT, "probe_math_pairs: unknown function");
    require(a && out_host && n > 0 && n <= kProbeMathMax, "probe_math_pairs: null pointer, n == 0 or n > 2^28");
    require(b || (fn != YART_MATH_DIV && fn != YART_MATH_POWF), "probe_math_pairs: this function takes a second operand");
    probeMath(fn, 0, n, 0.0f, a, b, out_host);
  });
}

// Diagnostic: the moment kernels on caller-supplied per-sample records (no scene), one accumulate launch per chunk
int yart_hip_probe_moments(const float* L_rgba, uint32_t n_pixels, uint32_t spp, const uint32_t* chunks, uint32_t n_chunks,
                           float exposure_scale, float* mean, float* variance, uint32_t* count) {
  return guarded([&] {
    require(L_rgba && chunks && mean && variance && count, "probe_moments: null pointer");
    require(n_pixels > 0 && spp > 0 && n_chunks > 0, "probe_moments: n_pixels, spp or n_chunks is 0");
    require(uint64_t(n_pixels) * spp <= (1ull << 26), "probe_moments: more than 2^26 records");
    uint64_t sum = 0;
    for (uint32_t c = 0; c < n_chunks; c++) { require(chunks[c] > 0, "probe_moments: an empty chunk"); sum += chunks[c]; }
    require(sum == spp, "probe_moments: the chunks do not sum to spp");
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) throw HipError("no HIP device");
    DevBuf<f4> L; DevBuf<MomentState> state; DevBuf<float> dMean, dVar; DevBuf<uint32_t> dCount;
    uint32_t largest = 0;
    for (uint32_t c = 0; c < n_chunks; c++) largest = std::max(largest, chunks[c]);
    L.ensure(size_t(n_pixels) * largest); state.ensure(n_pixels); dMean.ensure(size_t(n_pixels) * 3); dVar.ensure(n_pixels); dCount.ensure(n_pixels);
    HIP_CHECK(hipMemset(state.p, 0, size_t(n_pixels) * sizeof(MomentState)));
    std::vector<f4> wave(size_t(n_pixels) * largest);
    const f4* all = reinterpret_cast<const f4*>(L_rgba);
    uint32_t s0 = 0;
    for (uint32_t c = 0; c < n_chunks; c++) {
      const uint32_t w = chunks[c];           // the records of this "wave", pixel-major, w per pixel: what a batch holds in its L array
      for (uint32_t pi = 0; pi < n_pixels; pi++)
        for (uint32_t k = 0; k < w; k++) wave[size_t(pi) * w + k] = all[size_t(pi) * spp + s0 + k];
      HIP_CHECK(hipMemcpy(L.p, wave.data(), size_t(n_pixels) * w * sizeof(f4), hipMemcpyHostToDevice));
      MomentArgs ma{};
      ma.L = L.p; ma.state = state.p; ma.nPixels = n_pixels; ma.spp = w; ma.pixBase = 0; ma.exposureScale = exposure_scale;
      hipLaunchKernelGGL(k_moments_accumulate, dim3((n_pixels + kMomentPixPerBlock - 1) / kMomentPixPerBlock), dim3(kBlock), 0, nullptr, ma);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
      s0 += w;
    }
    MomentFinishArgs f{};
    f.state = state.p; f.pixels = nullptr; f.nPixels = n_pixels; f.width = n_pixels; f.mask = YART_MOMENT_ALL;
    f.mean = dMean.p; f.variance = dVar.p; f.count = dCount.p;
    hipLaunchKernelGGL(k_moments_finish, dim3((n_pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, f);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(mean, dMean.p, size_t(n_pixels) * 12, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(variance, dVar.p, size_t(n_pixels) * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(count, dCount.p, size_t(n_pixels) * 4, hipMemcpyDeviceToHost));
  });
}

// Diagnostic: k_gmon_blend on caller-supplied per-sample records (no scene), one launch with the render's launch geometry
int yart_hip_probe_estimator(const float* L_rgba, uint32_t n_pixels, uint32_t spp, int kind, float exposure_scale,
                             const uint32_t* pixels, uint32_t width, uint32_t height, float w_current, float w_wave,
                             float* hdr_inout, uint32_t* pix_rays) {
  return guarded([&] {
    require(L_rgba && hdr_inout, "probe_estimator: null pointer");
    require(n_pixels > 0 && spp > 0, "probe_estimator: n_pixels or spp is 0");
    require(width > 0 && height > 0, "probe_estimator: width or height is 0");
    require(width <= 65536u && height <= 65536u, "probe_estimator: width or height above 65536");     // pixels[] packs x | y << 16
    require(kind >= EST_GMON && kind <= EST_GMONB, "probe_estimator: kind must be one of YART_ESTIMATOR_*");
    require(uint64_t(n_pixels) * spp <= (1ull << 26), "probe_estimator: more than 2^26 records");
    require(uint64_t(n_pixels) <= uint64_t(width) * height, "probe_estimator: n_pixels exceeds width * height");
    require(std::isfinite(exposure_scale), "probe_estimator: exposure_scale is not finite");
    require(std::isfinite(w_current) && std::isfinite(w_wave), "probe_estimator: a blend weight is not finite");
    std::vector<uint32_t> px(n_pixels);
    for (uint32_t i = 0; i < n_pixels; i++) {
      px[i] = pixels ? pixels[i] : (i % width) | ((i / width) << 16);
      require((px[i] & 0xffffu) < width && (px[i] >> 16) < height, "probe_estimator: a pixels[] entry is outside the frame");
    }
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) throw HipError("no HIP device");
    const size_t records = size_t(n_pixels) * spp, frame = size_t(width) * height * 4;
    DevBuf<f4> L; DevBuf<uint32_t> dPixels, dRays; DevBuf<float> hdr;
    L.ensure(records); dPixels.ensure(n_pixels); hdr.ensure(frame);
    if (pix_rays) dRays.ensure(n_pixels);
    HIP_CHECK(hipMemcpy(L.p, L_rgba, records * sizeof(f4), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dPixels.p, px.data(), size_t(n_pixels) * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(hdr.p, hdr_inout, frame * sizeof(float), hipMemcpyHostToDevice));
    GmonArgs g{};
    g.L = L.p; g.pixRays = dRays.p; g.pixels = dPixels.p; g.nPixels = n_pixels; g.spp = spp; g.width = width;
    g.kind = kind; g.exposureScale = exposure_scale; g.wCurrent = w_current; g.wWave = w_wave; g.hdr = hdr.p;
    hipLaunchKernelGGL(k_gmon_blend, dim3((n_pixels + kGmonPixPerBlock - 1) / kGmonPixPerBlock), dim3(kBlock), 0, nullptr, g);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(hdr_inout, hdr.p, frame * sizeof(float), hipMemcpyDeviceToHost));
    if (pix_rays) HIP_CHECK(hipMemcpy(pix_rays, dRays.p, size_t(n_pixels) * 4, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
