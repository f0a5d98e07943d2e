// postprocess.inc — what happens to a frame after it has been rendered: the AgX tonemap and the 8-bit encoding, the edge-avoiding
// a-trous denoiser, temporal accumulation and auto-exposure; kernels, host drivers and the entries of the C ABI (included by yart_hip.hip,
// unit 0, after `guarded`; nothing here needs a scene).
#include "tonemap.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "exposure.hpp"

namespace {

// AgX tonemap of an RGBA32F frame (alpha kept as 1, tile-renderer.hpp:234-237) and the 8-bit
// encoding of output/ppm.cpp; one lane per pixel, 16 B in / 16 B (or 3 B) out: HBM-bound.
__global__ void __launch_bounds__(kBlock) k_tonemap_agx(const f4* in, f4* out, uint32_t n, int look) {
  const AgxLook lk = agxLook(look);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const f4 v = in[i];
    const f3 c = agxTonemap(mk3(v.x, v.y, v.z), lk);
    f4 o; o.x = c.x; o.y = c.y; o.z = c.z; o.w = 1.0f;
    out[i] = o;
  }
}
__global__ void __launch_bounds__(kBlock) k_encode_rgb8(const f4* in, uint8_t* out, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const f4 v = in[i];
    out[3 * size_t(i)] = ppmByte(v.x); out[3 * size_t(i) + 1] = ppmByte(v.y); out[3 * size_t(i) + 2] = ppmByte(v.z);
  }
}

#include "denoise_kernels.inc"
#include "temporal_kernels.inc"
#include "exposure_kernels.inc"

}  // namespace

extern "C" {

int yart_hip_tonemap_agx(const float* d_hdr_rgba, uint32_t width, uint32_t height, int look, float* d_ldr_rgba,
                         void* stream) {
  return guarded([&] {
    require(d_hdr_rgba && d_ldr_rgba && width > 0 && height > 0 && look >= 0 && look <= 2, "tonemap: bad argument");
    const uint32_t n = width * height;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_tonemap_agx, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                       reinterpret_cast<const f4*>(d_hdr_rgba), reinterpret_cast<f4*>(d_ldr_rgba), n, look);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int yart_hip_encode_rgb8(const float* d_rgba, uint32_t width, uint32_t height, uint8_t* d_rgb8, void* stream) {
  return guarded([&] {
    require(d_rgba && d_rgb8 && width > 0 && height > 0, "encode: bad argument");
    const uint32_t n = width * height;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_encode_rgb8, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                       reinterpret_cast<const f4*>(d_rgba), d_rgb8, n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int yart_hip_tonemap_host(const float* hdr_rgba, uint32_t width, uint32_t height, int look, float* ldr_rgba,
                          uint8_t* rgb8) {
  return guarded([&] {
    require(hdr_rgba && width > 0 && height > 0 && look >= -1 && look <= 2, "tonemap: bad argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw HipError("no HIP device");
    const size_t n = size_t(width) * height;
    DevBuf<float> in, out; DevBuf<uint8_t> bytes;
    in.ensure(n * 4); out.ensure(n * 4); bytes.ensure(n * 3);
    HIP_CHECK(hipMemcpy(in.p, hdr_rgba, n * 16, hipMemcpyHostToDevice));
    const float* src = in.p;
    if (look >= 0) {                                           // look -1: no tonemapper (tile-renderer.hpp:238-240)
      hipLaunchKernelGGL(k_tonemap_agx, dim3((uint32_t(n) + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr,
                         reinterpret_cast<const f4*>(in.p), reinterpret_cast<f4*>(out.p), uint32_t(n), look);
      HIP_CHECK(hipGetLastError());
      src = out.p;
    }
    hipLaunchKernelGGL(k_encode_rgb8, dim3((uint32_t(n) + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr,
                       reinterpret_cast<const f4*>(src), bytes.p, uint32_t(n));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (ldr_rgba) HIP_CHECK(hipMemcpy(ldr_rgba, src, n * 16, hipMemcpyDeviceToHost));
    if (rgb8) HIP_CHECK(hipMemcpy(rgb8, bytes.p, n * 3, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
// Edge-avoiding à-trous filter (denoise_kernels.inc), plain (VAR = false, YartDenoiseParams) and variance-guided (VAR = true,
// YartDenoiseVarParams, with a variance buffer). The arguments are judged here, before any device is touched; the last thing the
// check asks is whether there is a device at all.
namespace {
struct DnCall { DnConst k; uint32_t iterations; bool demodulate; };
inline float dnSigmaFirst(const YartDenoiseParams& p) { return p.sigma_color; }
inline float dnSigmaFirst(const YartDenoiseVarParams& p) { return p.sigma_luma; }
template <bool VAR>
using DnParams = std::conditional_t<VAR, YartDenoiseVarParams, YartDenoiseParams>;

template <bool VAR>
DnCall denoiseCheck(const void* rgba, const void* variance, const void* albedo, const void* normal, const void* depth, uint32_t width,
                    uint32_t height, const DnParams<VAR>* params, const void* out) {
  require(rgba && out, "denoise: rgba / out pointer is null");
  if (VAR) require(variance != nullptr, "denoise: variance pointer is null");
  require(params != nullptr, "denoise: params pointer is null");
  require(params->struct_size >= sizeof(*params), VAR ? "denoise: struct_size is smaller than YartDenoiseVarParams"
                                                      : "denoise: struct_size is smaller than YartDenoiseParams");
  require(params->iterations <= 8u, "denoise: iterations > 8");
  require(width > 0 && height > 0, "denoise: width or height is 0");
  require(uint64_t(width) * height <= (1ull << 28), "denoise: more than 2^28 pixels");
  require(std::isfinite(dnSigmaFirst(*params)) && std::isfinite(params->sigma_normal) && std::isfinite(params->sigma_depth),
          "denoise: a sigma is not finite");
  require((params->flags & ~uint32_t(YART_DENOISE_DEMODULATE)) == 0u, "denoise: unknown flags bits");
  DnCall c;
  c.iterations = params->iterations;
  c.demodulate = (params->flags & YART_DENOISE_DEMODULATE) != 0u;
  require(!c.demodulate || albedo, "denoise: YART_DENOISE_DEMODULATE without an albedo buffer");
  c.k = dnConstants<VAR>(dnSigmaFirst(*params), params->sigma_normal, params->sigma_depth, normal != nullptr, depth != nullptr);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw HipError("no HIP device");
  return c;
}

// device pointers (variance: the variance-guided form only); enqueues on `st` and returns after completion
template <bool VAR>
void denoiseRun(const DnCall& c, const float* rgba, const float* variance, const float* albedo, const float* normal, const float* depth,
                uint32_t width, uint32_t height, float* out, hipStream_t st) {
  const uint32_t n = width * height;
  if (c.iterations == 0u) {                         // a plain copy: no demodulation round trip
    if (out != rgba) HIP_CHECK(hipMemcpyAsync(out, rgba, size_t(n) * 16, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return;
  }
  DevBuf<f4> scratch;                               // working colour image 0 | image 1 | guide records: 48 bytes per pixel
  scratch.ensure(size_t(n) * 3);
  f4 *img[2] = {scratch.p, scratch.p + n}, *guide = scratch.p + size_t(n) * 2;
  const dim3 flat((n + kBlock - 1) / kBlock), block(kBlock);
  DnPrepareArgs<VAR> pa{};
  if constexpr (VAR) pa.variance = variance;
  pa.rgba = rgba; pa.albedo = c.demodulate ? albedo : nullptr; pa.normal = normal; pa.depth = depth;
  pa.colour = img[0]; pa.guide = guide; pa.n = n;
  hipLaunchKernelGGL(k_dn_prepare<VAR>, flat, block, 0, st, pa);
  HIP_CHECK(hipGetLastError());
  for (uint32_t i = 0; i < c.iterations; i++) {
    DnAtrousArgs aa{img[i & 1u], guide, img[(i + 1u) & 1u], width, height, i, 0u, c.k};
    if (i < 2u) {
      aa.tilesX = (width + 15u) / 16u;
      hipLaunchKernelGGL((k_dn_atrous<VAR, 0>), dim3(aa.tilesX * ((height + 15u) / 16u)), block, 0, st, aa);
    } else {
      aa.tilesX = (width + 63u) / 64u;
      hipLaunchKernelGGL((k_dn_atrous<VAR, 1>), dim3(aa.tilesX * ((height + 3u) / 4u)), block, 0, st, aa);
    }
    HIP_CHECK(hipGetLastError());
  }
  DnFinishArgs fa{img[c.iterations & 1u], rgba, c.demodulate ? albedo : nullptr, out, n, 0u};
  hipLaunchKernelGGL(k_dn_finish, flat, block, 0, st, fa);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
}

// host pointers: upload the buffers that are present, filter the frame in place on the device, copy it back
template <bool VAR>
void denoiseHost(const DnCall& c, const float* rgba, const float* variance, const float* albedo, const float* normal, const float* depth,
                 uint32_t width, uint32_t height, float* out) {
  const size_t n = size_t(width) * height;
  DevBuf<float> frame, var, alb, nrm, dep;
  const auto upload = [](DevBuf<float>& b, const float* host, size_t floats) {
    if (!host) return;
    b.ensure(floats);
    HIP_CHECK(hipMemcpy(b.p, host, floats * 4, hipMemcpyHostToDevice));
  };
  upload(frame, rgba, n * 4);
  if (VAR) upload(var, variance, n);
  if (c.demodulate) upload(alb, albedo, n * 3);
  upload(nrm, normal, n * 3);
  upload(dep, depth, n);
  denoiseRun<VAR>(c, frame.p, var.p, alb.p, nrm.p, dep.p, width, height, frame.p, nullptr);
  HIP_CHECK(hipMemcpy(out, frame.p, n * 16, hipMemcpyDeviceToHost));
}
}  // namespace
extern "C" {

int yart_hip_denoise_atrous_device(const float* d_rgba, const float* d_albedo, const float* d_normal, const float* d_depth,
                                   uint32_t width, uint32_t height, const YartDenoiseParams* params, float* d_out_rgba,
                                   void* stream) {
  return guarded([&] {
    const DnCall c = denoiseCheck<false>(d_rgba, nullptr, d_albedo, d_normal, d_depth, width, height, params, d_out_rgba);
    denoiseRun<false>(c, d_rgba, nullptr, d_albedo, d_normal, d_depth, width, height, d_out_rgba, static_cast<hipStream_t>(stream));
  });
}

int yart_hip_denoise_atrous_host(const float* rgba, const float* albedo, const float* normal, const float* depth, uint32_t width,
                                 uint32_t height, const YartDenoiseParams* params, float* out_rgba) {
  return guarded([&] {
    const DnCall c = denoiseCheck<false>(rgba, nullptr, albedo, normal, depth, width, height, params, out_rgba);
    denoiseHost<false>(c, rgba, nullptr, albedo, normal, depth, width, height, out_rgba);
  });
}

int yart_hip_denoise_atrous_var_device(const float* d_rgba, const float* d_variance, const float* d_albedo, const float* d_normal,
                                       const float* d_depth, uint32_t width, uint32_t height, const YartDenoiseVarParams* params,
                                       float* d_out_rgba, void* stream) {
  return guarded([&] {
    const DnCall c = denoiseCheck<true>(d_rgba, d_variance, d_albedo, d_normal, d_depth, width, height, params, d_out_rgba);
    denoiseRun<true>(c, d_rgba, d_variance, d_albedo, d_normal, d_depth, width, height, d_out_rgba, static_cast<hipStream_t>(stream));
  });
}

int yart_hip_denoise_atrous_var_host(const float* rgba, const float* variance, const float* albedo, const float* normal,
                                     const float* depth, uint32_t width, uint32_t height, const YartDenoiseVarParams* params,
                                     float* out_rgba) {
  return guarded([&] {
    const DnCall c = denoiseCheck<true>(rgba, variance, albedo, normal, depth, width, height, params, out_rgba);
    denoiseHost<true>(c, rgba, variance, albedo, normal, depth, width, height, out_rgba);
  });
}

// Temporal accumulation (temporal_kernels.inc: k_tp_accumulate). The arguments are judged before any device is touched; the handle's
// history — two images of three record planes, 96 bytes per pixel; four planes, 128 bytes, in the moments form — is allocated by
// the first call that gets that far. A handle is in one form from its first accumulate to the next reset. The clip
// (yart_hip_temporal_set_clip) is a setting that stays; with one, a call whose output aliases its frame stages the frame first.
}  // extern "C"
struct YartTemporal {
  uint32_t width = 0, height = 0;
  int device = -1;                                  // < 0 until the first accumulate call: the device current then
  std::mutex mu;
  DevBuf<f4> hist;                                  // image 0 (rec0 | rec1 | rec2 (| rec3) planes) | image 1
  bool moments = false;                             // the form of the history, while haveHistory
  uint32_t current = 0;                             // the image that holds the last frame's records
  bool haveHistory = false;
  YartCameraDesc camera{};                          // of the last accumulated frame
  std::vector<float> motion;                        // yart_hip_temporal_set_motion: the pending records, 24 floats per node; empty: none
  std::vector<float> motionTaken;                   // what the running call consumed: the source of its upload
  DevBuf<f4> motionDev;
  const float* pixelMotion = nullptr;               // yart_hip_temporal_set_pixel_motion: the caller's pending records, 8 floats per pixel
  const float* pixelMotionTaken = nullptr;          // what the running call consumed (only one of the two motions is ever pending)
  bool clip = false;                                // yart_hip_temporal_set_clip: the setting; it stays until it is set again
  uint32_t clipRadius = 0;
  float clipGamma = 0.0f;
  DevBuf<f4> staging;                               // with a clip, the frame of a call whose d_out_rgba is d_rgba: 16 bytes per pixel
};
namespace {
struct TpCall { TpConst k; bool demodulate; YartAovBuffers aovs; };
// the feature buffers an accumulate call reads, in the order they are checked and staged (albedo: with YART_TEMPORAL_DEMODULATE only)
struct TemporalField { uint32_t bit; bool demodulateOnly; const char* missing; };
constexpr TemporalField kTemporalFields[] = {
    {YART_AOV_POSITION, false, "temporal: the position feature buffer (YART_AOV_POSITION) is missing"},
    {YART_AOV_NORMAL, false, "temporal: the normal feature buffer (YART_AOV_NORMAL) is missing"},
    {YART_AOV_DEPTH, false, "temporal: the depth feature buffer (YART_AOV_DEPTH) is missing"},
    {YART_AOV_COVERAGE, false, "temporal: the coverage feature buffer (YART_AOV_COVERAGE) is missing"},
    {YART_AOV_IDS, false, "temporal: the ids feature buffer (YART_AOV_IDS) is missing"},
    {YART_AOV_ALBEDO, true, "temporal: YART_TEMPORAL_DEMODULATE without an albedo feature buffer (YART_AOV_ALBEDO)"}};
uint32_t temporalMinMomentHistory(const YartTemporalParams&) { return 0u; }
uint32_t temporalMinMomentHistory(const YartTemporalMomentParams& p) { return p.min_moment_history; }

// Params: YartTemporalParams, or YartTemporalMomentParams (the same head, and min_moment_history)
template <class Params>
TpCall temporalCheck(const YartTemporal* t, const YartCameraDesc* cam, const void* rgba, const void* variance, const YartAovBuffers* aovs,
                     const Params* params, const void* out) {
  constexpr bool MOMENTS = std::is_same<Params, YartTemporalMomentParams>::value;
  require(t != nullptr, "temporal: handle pointer is null");
  require(cam != nullptr, "temporal: camera pointer is null");
  require(rgba && out, "temporal: rgba / out pointer is null");
  require(variance != nullptr, "temporal: variance pointer is null");
  require(aovs != nullptr, "temporal: feature buffers (aovs) pointer is null");
  require(params != nullptr, "temporal: params pointer is null");
  require(params->struct_size >= sizeof(Params), MOMENTS ? "temporal: struct_size is smaller than YartTemporalMomentParams"
                                                                 : "temporal: struct_size is smaller than YartTemporalParams");
  require((params->flags & ~uint32_t(YART_TEMPORAL_DEMODULATE)) == 0u, "temporal: unknown flags bits");
  require(std::isfinite(params->alpha_min) && std::isfinite(params->normal_cos_min) && std::isfinite(params->plane_tolerance),
          "temporal: a parameter is not finite");
  require(params->alpha_min >= 0.0f && params->alpha_min <= 1.0f, "temporal: alpha_min is outside [0, 1]");
  require(params->max_history >= 1u, "temporal: max_history is 0");
  if (MOMENTS) require(temporalMinMomentHistory(*params) >= 2u, "temporal: min_moment_history is smaller than 2");
  require(cam->width == t->width && cam->height == t->height, "temporal: the camera's image size is not the handle's");
  require(cam->focal_length > 0.0f, "temporal: camera: bad focal length");
  TpCall c{};
  c.demodulate = (params->flags & YART_TEMPORAL_DEMODULATE) != 0u;
  checkBufferHead(kAovTable, *aovs, "temporal: ");
  for (const TemporalField& f : kTemporalFields)
    if (!f.demodulateOnly || c.demodulate) require(takeBufferField(*aovs, kAovTable.field(f.bit), c.aovs), f.missing);
  c.k.alphaMin = params->alpha_min; c.k.normalCosMin = params->normal_cos_min; c.k.planeTolerance = params->plane_tolerance;
  c.k.maxHistory = params->max_history;
  c.k.minMomentHistory = temporalMinMomentHistory(*params);
  c.k.width = t->width; c.k.height = t->height;
  return c;
}

// the handle's mutex held, before any device is touched
template <bool MOMENTS>
void temporalCheckForm(const YartTemporal& t) {
  require(!t.haveHistory || t.moments == MOMENTS,
          MOMENTS ? "temporal: the handle's history is in the plain form: reset it before the moments form"
                  : "temporal: the handle's history is in the moments form: reset it before the plain form");
}

// the handle's mutex held, after the call's last argument check and before any device is touched: the call consumes the pending motion
void temporalTakeMotion(YartTemporal& t) {
  t.motionTaken.clear();
  t.motionTaken.swap(t.motion);
  t.pixelMotionTaken = t.pixelMotion;
  t.pixelMotion = nullptr;
}

// MOTION / PIXEL as k_tp_accumulate takes them; clip: the CLIP instantiation, which is launched only while a clip is set
template <bool MOMENTS, bool MOTION, bool PIXEL, class Motion>
void temporalLaunch(bool clip, dim3 grid, hipStream_t st, const TpArgs& a, const Motion& motion) {
  if (clip) hipLaunchKernelGGL((k_tp_accumulate<MOMENTS, MOTION, PIXEL, true>), grid, dim3(kBlock), 0, st, a, motion);
  else hipLaunchKernelGGL((k_tp_accumulate<MOMENTS, MOTION, PIXEL>), grid, dim3(kBlock), 0, st, a, motion);
}

// device pointers (c.aovs included); the handle's device is current and its mutex held; returns after completion on `st`
template <bool MOMENTS>
void temporalRun(YartTemporal& t, TpCall c, const YartCameraDesc& cam, const float* rgba, const float* variance, float* out,
                 float* outVariance, uint32_t* outLength, hipStream_t st) {
  const uint32_t n = t.width * t.height;
  constexpr size_t planes = MOMENTS ? 4 : 3;
  t.hist.ensure(size_t(n) * planes * 2);
  c.k.haveHistory = t.haveHistory ? 1u : 0u;
  TpArgs a{};
  a.rgba = rgba; a.variance = variance; a.albedo = c.demodulate ? c.aovs.albedo : nullptr;
  a.position = c.aovs.position; a.normal = c.aovs.normal; a.depth = c.aovs.depth; a.coverage = c.aovs.coverage; a.ids = c.aovs.ids;
  a.histIn = t.hist.p + size_t(t.current) * n * planes;
  a.histOut = t.hist.p + size_t(t.current ^ 1u) * n * planes;
  a.outRgba = out; a.outVariance = outVariance; a.outLength = outLength;
  a.n = n; a.tilesX = (t.width + 15u) / 16u;
  a.k = c.k;
  if (t.haveHistory) a.cam = tpCamera(makeCamera(t.camera));
  if (t.clip) {
    a.clipRadius = t.clipRadius; a.clipGamma = t.clipGamma;
    if (out == rgba) {                              // the kernel reads neighbours' rgba: a copy, on `st`, before the kernel overwrites it
      t.staging.ensure(n);
      HIP_CHECK(hipMemcpyAsync(t.staging.p, rgba, size_t(n) * sizeof(f4), hipMemcpyDeviceToDevice, st));
      a.rgba = reinterpret_cast<const float*>(t.staging.p);
    }
  }
  const dim3 grid(a.tilesX * ((t.height + 15u) / 16u));
  if (t.pixelMotionTaken) {                         // device records, written on `st` or complete before the call
    const TpDevicePixelRecords motion{reinterpret_cast<const f4*>(t.pixelMotionTaken)};
    temporalLaunch<MOMENTS, true, true>(t.clip, grid, st, a, motion);
  } else if (!t.motionTaken.empty()) {              // on `st`, before the kernel that reads it
    const size_t words = t.motionTaken.size() / 4;
    t.motionDev.ensure(words);
    HIP_CHECK(hipMemcpyAsync(t.motionDev.p, t.motionTaken.data(), words * sizeof(f4), hipMemcpyHostToDevice, st));
    const TpDeviceMotion motion{t.motionDev.p, uint32_t(words / kTpMotionWords)};
    temporalLaunch<MOMENTS, true, false>(t.clip, grid, st, a, motion);
  } else {
    temporalLaunch<MOMENTS, false, false>(t.clip, grid, st, a, TpNoMotion{});
  }
  HIP_CHECK(hipGetLastError());
  if (MOMENTS) {                                    // pass 2 on the image pass 1 wrote
    hipLaunchKernelGGL(k_tp_spatial_variance, grid, dim3(kBlock), 0, st, a);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipStreamSynchronize(st));
  t.current ^= 1u; t.haveHistory = true; t.moments = MOMENTS; t.camera = cam;
}

void temporalSelectDevice(YartTemporal& t) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw HipError("no HIP device");
  if (t.device < 0) HIP_CHECK(hipGetDevice(&t.device));
  HIP_CHECK(hipSetDevice(t.device));
}
}  // namespace
extern "C" {

int yart_hip_temporal_create(uint32_t width, uint32_t height, int device, YartTemporal** out) {
  return guarded([&] {
    require(out != nullptr, "temporal: out pointer is null");
    require(width > 0 && height > 0, "temporal: width or height is 0");
    require(uint64_t(width) * height <= (1ull << 28), "temporal: more than 2^28 pixels");
    auto* t = new YartTemporal;
    t->width = width; t->height = height; t->device = device;
    *out = t;
  });
}

void yart_hip_temporal_destroy(YartTemporal* temporal) {
  if (!temporal) return;
  if ((temporal->hist.p || temporal->staging.p) && temporal->device >= 0) (void)hipSetDevice(temporal->device);
  delete temporal;
}

int yart_hip_temporal_reset(YartTemporal* temporal) {
  return guarded([&] {
    require(temporal != nullptr, "temporal: handle pointer is null");
    std::lock_guard<std::mutex> lock(temporal->mu);
    temporal->haveHistory = false;
    temporal->motion.clear();
    temporal->pixelMotion = nullptr;
  });
}

int yart_hip_temporal_set_clip(YartTemporal* temporal, const YartTemporalClip* clip) {
  return guarded([&] {
    require(temporal != nullptr, "temporal: handle pointer is null");
    std::lock_guard<std::mutex> lock(temporal->mu);
    if (!clip) { temporal->clip = false; return; }  // (a refused clip keeps the previous setting: nothing is written before the checks)
    require(clip->struct_size >= sizeof(YartTemporalClip), "temporal: struct_size is smaller than YartTemporalClip");
    require(clip->radius >= 1u && clip->radius <= kTpClipMaxRadius, "temporal: clip: radius is outside 1 .. 3");
    require(std::isfinite(clip->gamma) && clip->gamma >= 0.0f, "temporal: clip: gamma is not finite or is negative");
    temporal->clip = true; temporal->clipRadius = clip->radius; temporal->clipGamma = clip->gamma;
  });
}

int yart_hip_temporal_set_motion(YartTemporal* temporal, const YartTemporalMotion* motion) {
  return guarded([&] {
    require(temporal != nullptr, "temporal: handle pointer is null");
    std::lock_guard<std::mutex> lock(temporal->mu);
    temporal->motion.clear();                       // a refused motion leaves nothing pending
    temporal->pixelMotion = nullptr;                // (one motion is pending at a time: a setter replaces what the other left)
    if (!motion) return;
    require(motion->struct_size >= sizeof(YartTemporalMotion), "temporal: struct_size is smaller than YartTemporalMotion");
    require(motion->n_nodes >= 1u && motion->n_nodes < kTpMotionMaxNodes, "temporal: motion: n_nodes is 0 or not below 2^20");
    require(motion->records != nullptr, "temporal: motion: records pointer is null");
    constexpr size_t kWords = kTpMotionWords * 4;
    for (uint32_t i = 0; i < motion->n_nodes; i++) {
      const float* r = motion->records + size_t(i) * kWords;
      const uint32_t kind = dnBits(r[15]);
      require(kind <= 1u, "temporal: motion: a record's kind is neither 0 (static) nor 1 (moving)");
      if (kind == 0u) continue;
      for (size_t j = 0; j < kWords; j++)
        require(j == 15 || std::isfinite(r[j]), "temporal: motion: a word of a moving node's record is not finite");
    }
    temporal->motion.assign(motion->records, motion->records + size_t(motion->n_nodes) * kWords);
  });
}

int yart_hip_temporal_set_pixel_motion(YartTemporal* temporal, const YartTemporalPixelMotion* motion) {
  return guarded([&] {
    require(temporal != nullptr, "temporal: handle pointer is null");
    std::lock_guard<std::mutex> lock(temporal->mu);
    temporal->motion.clear();                       // a refused motion leaves nothing pending
    temporal->pixelMotion = nullptr;
    if (!motion) return;
    require(motion->struct_size >= sizeof(YartTemporalPixelMotion), "temporal: struct_size is smaller than YartTemporalPixelMotion");
    require(motion->records != nullptr, "temporal: pixel motion: records pointer is null");
    temporal->pixelMotion = motion->records;
  });
}

}  // extern "C"
namespace {
template <bool MOMENTS, class Params>
int temporalAccumulateDevice(YartTemporal* temporal, const YartCameraDesc* cam, const float* d_rgba, const float* d_variance,
                             const YartAovBuffers* d_aovs, const Params* params, float* d_out_rgba, float* d_out_variance,
                             uint32_t* d_out_length, void* stream) {
  return guarded([&] {
    const TpCall c = temporalCheck(temporal, cam, d_rgba, d_variance, d_aovs, params, d_out_rgba);
    std::lock_guard<std::mutex> lock(temporal->mu);
    temporalCheckForm<MOMENTS>(*temporal);
    require((reinterpret_cast<uintptr_t>(temporal->pixelMotion) & 15u) == 0u, "temporal: the pending per-pixel motion records are not 16-byte aligned");
    temporalTakeMotion(*temporal);
    temporalSelectDevice(*temporal);
    temporalRun<MOMENTS>(*temporal, c, *cam, d_rgba, d_variance, d_out_rgba, d_out_variance, d_out_length, static_cast<hipStream_t>(stream));
  });
}

template <bool MOMENTS, class Params>
int temporalAccumulateHost(YartTemporal* temporal, const YartCameraDesc* cam, const float* rgba, const float* variance,
                           const YartAovBuffers* aovs, const Params* params, float* out_rgba, float* out_variance, uint32_t* out_length) {
  return guarded([&] {
    TpCall c = temporalCheck(temporal, cam, rgba, variance, aovs, params, out_rgba);
    std::lock_guard<std::mutex> lock(temporal->mu);
    temporalCheckForm<MOMENTS>(*temporal);
    temporalTakeMotion(*temporal);
    temporalSelectDevice(*temporal);
    const size_t n = size_t(temporal->width) * temporal->height;
    // per-pixel motion records (8, when pending) | frame (4) | variance (1) | position (3) | normal (3) | depth (1) | coverage (1) |
    // ids (4) | albedo (3) | length (1) words per pixel; frame and variance are accumulated in place
    DevBuf<float> buf;
    const float* hostRecords = temporal->pixelMotionTaken;
    buf.ensure(n * (hostRecords ? 29 : 21));
    float* w = buf.p;
    if (hostRecords) {
      HIP_CHECK(hipMemcpy(w, hostRecords, n * 8 * 4, hipMemcpyHostToDevice));
      temporal->pixelMotionTaken = w;
      w += n * 8;
    }
    auto put = [&](const void* src, size_t words) {
      float* dst = w; w += n * words;
      if (src) HIP_CHECK(hipMemcpy(dst, src, n * words * 4, hipMemcpyHostToDevice));
      return dst;
    };
    float* dFrame = put(rgba, 4);
    float* dVar = put(variance, 1);
    for (const TemporalField& tf : kTemporalFields) {        // (albedo without YART_TEMPORAL_DEMODULATE: null in c.aovs, room but no copy)
      const BufferField& f = kAovTable.field(tf.bit);
      setFieldPtr(c.aovs, f, put(fieldPtr(c.aovs, f), f.words));
    }
    uint32_t* dLen = reinterpret_cast<uint32_t*>(put(nullptr, 1));
    temporalRun<MOMENTS>(*temporal, c, *cam, dFrame, dVar, dFrame, dVar, dLen, nullptr);
    HIP_CHECK(hipMemcpy(out_rgba, dFrame, n * 16, hipMemcpyDeviceToHost));
    if (out_variance) HIP_CHECK(hipMemcpy(out_variance, dVar, n * 4, hipMemcpyDeviceToHost));
    if (out_length) HIP_CHECK(hipMemcpy(out_length, dLen, n * 4, hipMemcpyDeviceToHost));
  });
}
}  // namespace
extern "C" {

int yart_hip_temporal_accumulate_device(YartTemporal* temporal, const YartCameraDesc* cam, const float* d_rgba, const float* d_variance,
                                        const YartAovBuffers* d_aovs, const YartTemporalParams* params, float* d_out_rgba,
                                        float* d_out_variance, uint32_t* d_out_length, void* stream) {
  return temporalAccumulateDevice<false>(temporal, cam, d_rgba, d_variance, d_aovs, params, d_out_rgba, d_out_variance, d_out_length, stream);
}

int yart_hip_temporal_accumulate_host(YartTemporal* temporal, const YartCameraDesc* cam, const float* rgba, const float* variance,
                                      const YartAovBuffers* aovs, const YartTemporalParams* params, float* out_rgba,
                                      float* out_variance, uint32_t* out_length) {
  return temporalAccumulateHost<false>(temporal, cam, rgba, variance, aovs, params, out_rgba, out_variance, out_length);
}

int yart_hip_temporal_accumulate_moments_device(YartTemporal* temporal, const YartCameraDesc* cam, const float* d_rgba,
                                                const float* d_variance, const YartAovBuffers* d_aovs,
                                                const YartTemporalMomentParams* params, float* d_out_rgba, float* d_out_variance,
                                                uint32_t* d_out_length, void* stream) {
  return temporalAccumulateDevice<true>(temporal, cam, d_rgba, d_variance, d_aovs, params, d_out_rgba, d_out_variance, d_out_length, stream);
}

int yart_hip_temporal_accumulate_moments_host(YartTemporal* temporal, const YartCameraDesc* cam, const float* rgba, const float* variance,
                                              const YartAovBuffers* aovs, const YartTemporalMomentParams* params, float* out_rgba,
                                              float* out_variance, uint32_t* out_length) {
  return temporalAccumulateHost<true>(temporal, cam, rgba, variance, aovs, params, out_rgba, out_variance, out_length);
}

}  // extern "C"

// Auto-exposure (exposure_kernels.inc: k_ex_histogram, k_ex_resolve, k_ex_apply). The arguments are judged before any device is
// touched; the handle's device memory — the accumulating histogram, the last call's histogram and the state record — is allocated
// by the first call that gets that far. The state never leaves the device between a meter call and the apply calls that follow.
struct YartExposure {
  int device = -1;                                  // < 0 until the first call that needs one: the device current then
  std::mutex mu;
  DevBuf<uint32_t> words;                           // hist (256) | ignored (1) | pad | last (256) | record
  uint32_t* hist() const { return words.p; }
  uint32_t* last() const { return words.p + kExLastAt; }
  ExRecord* record() const { return reinterpret_cast<ExRecord*>(words.p + kExRecordAt); }
  static constexpr size_t kExLastAt = 260, kExRecordAt = 516, kExWords = kExRecordAt + sizeof(ExRecord) / 4;
};
namespace {
constexpr uint32_t kExMaxBlocks = 512u;            // k_ex_histogram's grid: at most 2 workgroups per CU, each striding over the window
#ifndef YART_EXPOSURE_HISTOGRAM
#define YART_EXPOSURE_HISTOGRAM 1                  // the kept form of k_ex_histogram (exposure_kernels.inc; profiles/auto_exposure.txt)
#endif
struct ExCall { ExConst k; uint32_t x0, y0, ww, wh; };

ExCall exposureCheckMeter(const YartExposure* e, const void* rgba, uint32_t width, uint32_t height, const YartExposureParams* p, float dt) {
  require(e != nullptr, "exposure: handle pointer is null");
  require(rgba != nullptr, "exposure: rgba pointer is null");
  require(p != nullptr, "exposure: params pointer is null");
  require(p->struct_size >= sizeof(YartExposureParams), "exposure: struct_size is smaller than YartExposureParams");
  require(width > 0 && height > 0, "exposure: width or height is 0");
  require(uint64_t(width) * height <= (1ull << 28), "exposure: more than 2^28 pixels");
  require(std::isfinite(p->ev_min) && std::isfinite(p->ev_max) && p->ev_min < p->ev_max, "exposure: ev_min / ev_max are not finite or ev_min >= ev_max");
  require(p->trim_low >= 0.0f && p->trim_low < 1.0f && p->trim_high >= 0.0f && p->trim_high < 1.0f && p->trim_low + p->trim_high < 1.0f,
          "exposure: trim_low / trim_high are outside [0, 1) or their sum is not below 1");
  require(std::isfinite(p->key) && p->key > 0.0f, "exposure: key is not finite or not positive");
  require(std::isfinite(p->compensation_ev), "exposure: compensation_ev is not finite");
  require(std::isfinite(p->gain_ev_min) && std::isfinite(p->gain_ev_max) && p->gain_ev_min <= p->gain_ev_max,
          "exposure: gain_ev_min / gain_ev_max are not finite or gain_ev_min > gain_ev_max");
  require(std::isfinite(p->speed_up) && std::isfinite(p->speed_down) && p->speed_up >= 0.0f && p->speed_down >= 0.0f,
          "exposure: speed_up / speed_down are not finite or negative");
  require(std::isfinite(dt) && dt >= 0.0f, "exposure: dt is not finite or negative");
  ExCall c{};
  if (p->x0 == 0u && p->y0 == 0u && p->x1 == 0u && p->y1 == 0u) {
    c.ww = width; c.wh = height;
  } else {
    require(p->x0 < p->x1 && p->x1 <= width && p->y0 < p->y1 && p->y1 <= height, "exposure: the metering window is empty or outside the frame");
    c.x0 = p->x0; c.y0 = p->y0; c.ww = p->x1 - p->x0; c.wh = p->y1 - p->y0;
  }
  c.k = exConstants(p->ev_min, p->ev_max, p->trim_low, p->trim_high, p->key, p->compensation_ev, p->gain_ev_min, p->gain_ev_max,
                    p->speed_up, p->speed_down, dt);
  return c;
}

void exposureCheckApply(const YartExposure* e, const void* rgba, uint32_t width, uint32_t height, int look, const void* ldr, const void* rgb8) {
  require(e != nullptr, "exposure: handle pointer is null");
  require(rgba != nullptr, "exposure: rgba pointer is null");
  require(ldr != nullptr || rgb8 != nullptr, "exposure: both outputs (ldr_rgba and rgb8) are null");
  require(width > 0 && height > 0, "exposure: width or height is 0");
  require(uint64_t(width) * height <= (1ull << 28), "exposure: more than 2^28 pixels");
  require(look >= -1 && look <= 2, "exposure: look is outside -1 .. 2");
}

void exposureAligned(const void* p, const char* what) { require((reinterpret_cast<uintptr_t>(p) & 15u) == 0u, what); }

// the handle's mutex held: its device made current, its memory allocated and a new handle's record written
void exposureSelect(YartExposure& e) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw HipError("no HIP device");
  if (e.device < 0) HIP_CHECK(hipGetDevice(&e.device));
  HIP_CHECK(hipSetDevice(e.device));
  if (e.words.p) return;
  e.words.ensure(YartExposure::kExWords);
  HIP_CHECK(hipMemset(e.words.p, 0, YartExposure::kExWords * 4));
  const ExRecord fresh = exNewRecord();
  HIP_CHECK(hipMemcpy(e.record(), &fresh, sizeof(fresh), hipMemcpyHostToDevice));
}

template <int V>
void exposureLaunchHistogram(const YartExposure& e, const ExCall& c, const float* rgba, uint32_t width, hipStream_t st) {
  ExHistArgs ha{reinterpret_cast<const f4*>(rgba), e.hist(), width, c.x0, c.y0, c.ww, c.ww * c.wh, c.k};
  constexpr uint32_t perPass = kBlock * kExUnroll;
  const uint32_t blocks = std::min<uint32_t>((ha.n + perPass - 1) / perPass, kExMaxBlocks);
  hipLaunchKernelGGL(k_ex_histogram<V>, dim3(blocks), dim3(kBlock), 0, st, ha);
  HIP_CHECK(hipGetLastError());
}
void exposureLaunchResolve(const YartExposure& e, const ExCall& c, hipStream_t st) {
  ExResolveArgs ra{e.hist(), e.last(), e.record(), c.k};
  hipLaunchKernelGGL(k_ex_resolve, dim3(1), dim3(kBlock), 0, st, ra);
  HIP_CHECK(hipGetLastError());
}
void exposureLaunchApply(const YartExposure& e, const float* rgba, uint32_t n, int look, float* ldr, uint8_t* rgb8, hipStream_t st) {
  ExApplyArgs aa{reinterpret_cast<const f4*>(rgba), e.record(), reinterpret_cast<f4*>(ldr), rgb8, n, look};
  const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
  if (ldr && rgb8) hipLaunchKernelGGL((k_ex_apply<true, true>), grid, block, 0, st, aa);
  else if (ldr) hipLaunchKernelGGL((k_ex_apply<true, false>), grid, block, 0, st, aa);
  else hipLaunchKernelGGL((k_ex_apply<false, true>), grid, block, 0, st, aa);
  HIP_CHECK(hipGetLastError());
}

// device pointers; the handle's device is current and its mutex held; returns after completion on `st`
void exposureMeter(YartExposure& e, const ExCall& c, const float* rgba, uint32_t width, hipStream_t st) {
  exposureLaunchHistogram<YART_EXPOSURE_HISTOGRAM>(e, c, rgba, width, st);
  exposureLaunchResolve(e, c, st);
  HIP_CHECK(hipStreamSynchronize(st));
}
}  // namespace
extern "C" {

int yart_hip_exposure_create(int device, YartExposure** out) {
  return guarded([&] {
    require(out != nullptr, "exposure: out pointer is null");
    auto* e = new YartExposure;
    e->device = device;
    *out = e;
  });
}

void yart_hip_exposure_destroy(YartExposure* exposure) {
  if (!exposure) return;
  if (exposure->words.p && exposure->device >= 0) (void)hipSetDevice(exposure->device);
  delete exposure;
}

int yart_hip_exposure_reset(YartExposure* exposure) {
  return guarded([&] {
    require(exposure != nullptr, "exposure: handle pointer is null");
    std::lock_guard<std::mutex> lock(exposure->mu);
    if (!exposure->words.p) return;                 // nothing metered yet: a new handle already
    HIP_CHECK(hipSetDevice(exposure->device));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(exposure->words.p, 0, YartExposure::kExWords * 4));
    const ExRecord fresh = exNewRecord();
    HIP_CHECK(hipMemcpy(exposure->record(), &fresh, sizeof(fresh), hipMemcpyHostToDevice));
  });
}

int yart_hip_exposure_meter_device(YartExposure* exposure, const float* d_rgba, uint32_t width, uint32_t height,
                                   const YartExposureParams* params, float dt, void* stream) {
  return guarded([&] {
    const ExCall c = exposureCheckMeter(exposure, d_rgba, width, height, params, dt);
    exposureAligned(d_rgba, "exposure: d_rgba is not 16-byte aligned");
    std::lock_guard<std::mutex> lock(exposure->mu);
    exposureSelect(*exposure);
    exposureMeter(*exposure, c, d_rgba, width, static_cast<hipStream_t>(stream));
  });
}

int yart_hip_exposure_meter_host(YartExposure* exposure, const float* rgba, uint32_t width, uint32_t height,
                                 const YartExposureParams* params, float dt) {
  return guarded([&] {
    const ExCall c = exposureCheckMeter(exposure, rgba, width, height, params, dt);
    std::lock_guard<std::mutex> lock(exposure->mu);
    exposureSelect(*exposure);
    const size_t n = size_t(width) * height;
    DevBuf<float> frame;
    frame.ensure(n * 4);
    HIP_CHECK(hipMemcpy(frame.p, rgba, n * 16, hipMemcpyHostToDevice));
    exposureMeter(*exposure, c, frame.p, width, nullptr);
  });
}

int yart_hip_exposure_apply_device(YartExposure* exposure, const float* d_rgba, uint32_t width, uint32_t height, int look,
                                   float* d_ldr_rgba, uint8_t* d_rgb8, void* stream) {
  return guarded([&] {
    exposureCheckApply(exposure, d_rgba, width, height, look, d_ldr_rgba, d_rgb8);
    exposureAligned(d_rgba, "exposure: d_rgba is not 16-byte aligned");
    exposureAligned(d_ldr_rgba, "exposure: d_ldr_rgba is not 16-byte aligned");
    std::lock_guard<std::mutex> lock(exposure->mu);
    exposureSelect(*exposure);
    hipStream_t st = static_cast<hipStream_t>(stream);
    exposureLaunchApply(*exposure, d_rgba, width * height, look, d_ldr_rgba, d_rgb8, st);
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int yart_hip_exposure_apply_host(YartExposure* exposure, const float* rgba, uint32_t width, uint32_t height, int look, float* ldr_rgba,
                                 uint8_t* rgb8) {
  return guarded([&] {
    exposureCheckApply(exposure, rgba, width, height, look, ldr_rgba, rgb8);
    std::lock_guard<std::mutex> lock(exposure->mu);
    exposureSelect(*exposure);
    const size_t n = size_t(width) * height;
    DevBuf<float> frame; DevBuf<uint8_t> bytes;     // the frame is tonemapped in place
    frame.ensure(n * 4);
    if (rgb8) bytes.ensure(n * 3);
    HIP_CHECK(hipMemcpy(frame.p, rgba, n * 16, hipMemcpyHostToDevice));
    exposureLaunchApply(*exposure, frame.p, uint32_t(n), look, ldr_rgba ? frame.p : nullptr, bytes.p, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (ldr_rgba) HIP_CHECK(hipMemcpy(ldr_rgba, frame.p, n * 16, hipMemcpyDeviceToHost));
    if (rgb8) HIP_CHECK(hipMemcpy(rgb8, bytes.p, n * 3, hipMemcpyDeviceToHost));
  });
}

int yart_hip_exposure_get(YartExposure* exposure, YartExposureState* state, uint32_t* hist256) {
  return guarded([&] {
    require(exposure != nullptr, "exposure: handle pointer is null");
    require(state != nullptr, "exposure: state pointer is null");
    require(state->struct_size >= sizeof(YartExposureState), "exposure: struct_size is smaller than YartExposureState");
    std::lock_guard<std::mutex> lock(exposure->mu);
    ExRecord r = exNewRecord();
    if (exposure->words.p) {                        // (a handle that has touched no device reports a new handle's state)
      HIP_CHECK(hipSetDevice(exposure->device));
      HIP_CHECK(hipMemcpy(&r, exposure->record(), sizeof(r), hipMemcpyDeviceToHost));
      if (hist256) HIP_CHECK(hipMemcpy(hist256, exposure->last(), kExBins * 4, hipMemcpyDeviceToHost));
    } else if (hist256) {
      std::fill(hist256, hist256 + kExBins, 0u);
    }
    state->cur_ev = r.curEv; state->target_ev = r.targetEv; state->mean_ev = r.meanEv; state->gain = r.gain;
    state->n_counted = r.nCounted; state->n_ignored = r.nIgnored; state->frames = r.frames; state->flags = r.flags;
  });
}

// Not part of the interface (tools/exposure_bench.py): the device time of one of the exposure kernels — or of the pair
// k_tonemap_agx + k_encode_rgb8 that k_ex_apply replaces — over `repeats` launches between two events, in ms per launch.
// what: 0 / 1 k_ex_histogram<0 / 1>, 2 k_ex_resolve, 3 k_ex_apply<true, true>, 4 the pair. d_ldr_rgba and d_rgb8: for 3 and 4.
int yart_hip_debug_exposure_time(YartExposure* exposure, const float* d_rgba, uint32_t width, uint32_t height,
                                 const YartExposureParams* params, int what, uint32_t repeats, float* d_ldr_rgba, uint8_t* d_rgb8,
                                 float* ms_out) {
  return guarded([&] {
    const ExCall c = exposureCheckMeter(exposure, d_rgba, width, height, params, 0.0f);
    require(what >= 0 && what <= 4 && repeats >= 1u && ms_out, "exposure: debug: bad argument");
    require(what < 3 || (d_ldr_rgba && d_rgb8), "exposure: debug: outputs are null");
    exposureAligned(d_rgba, "exposure: d_rgba is not 16-byte aligned");
    std::lock_guard<std::mutex> lock(exposure->mu);
    exposureSelect(*exposure);
    YartExposure& e = *exposure;
    const uint32_t n = width * height;
    hipEvent_t t0, t1;
    HIP_CHECK(hipEventCreate(&t0)); HIP_CHECK(hipEventCreate(&t1));
    HIP_CHECK(hipEventRecord(t0, nullptr));
    for (uint32_t i = 0; i < repeats; i++) {
      if (what == 0) exposureLaunchHistogram<0>(e, c, d_rgba, width, nullptr);
      else if (what == 1) exposureLaunchHistogram<1>(e, c, d_rgba, width, nullptr);
      else if (what == 2) exposureLaunchResolve(e, c, nullptr);
      else if (what == 3) exposureLaunchApply(e, d_rgba, n, 0, d_ldr_rgba, d_rgb8, nullptr);
      else {
        hipLaunchKernelGGL(k_tonemap_agx, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, reinterpret_cast<const f4*>(d_rgba),
                           reinterpret_cast<f4*>(d_ldr_rgba), n, 0);
        hipLaunchKernelGGL(k_encode_rgb8, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, reinterpret_cast<const f4*>(d_ldr_rgba), d_rgb8, n);
        HIP_CHECK(hipGetLastError());
      }
    }
    HIP_CHECK(hipEventRecord(t1, nullptr));
    HIP_CHECK(hipEventSynchronize(t1));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    *ms_out = ms / float(repeats);
    // what the timed histogram launches left behind: the sum of `repeats` histograms, which yart_hip_exposure_get then reports
    if (what < 2) HIP_CHECK(hipMemcpy(e.last(), e.hist(), kExBins * 4, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemset(e.hist(), 0, (kExBins + 1u) * 4));
  });
}

}  // extern "C"
