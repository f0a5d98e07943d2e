// scene_motion_kernels.inc — yart_hip_scene_keep_previous and yart_hip_scene_pixel_motion_*: the scene remembers the previous frame's
// node and vertex arrays, and says per pixel where the surface point it shows was in that frame (included by yart_hip.hip, unit 0,
// after postprocess.inc whose 16-byte load / store it uses: the entries use YartScene and guarded). The arithmetic is
// csrc/scene_motion.hpp's; the definition is the header comment of include/yart_hip.h.
//
//   k_sm_node_chains  one lane per scene node: the node's composed transforms of both frames (binary64 along the chain, rounded to
//                     binary32 at the end) and its changed flag and mesh — thirteen 16-byte words per node. A scene has few nodes
//                     next to its pixels; the walk is suWorldBox's.
//   k_sm_pixels       one lane per pixel in the 16 x 16 tile of k_tp_accumulate: reads the pixel's position, normal, coverage and ids
//                     (44 bytes), the head word of its node's chain record, two words of the mesh record, the triangle's vertex
//                     ids and its three current and three previous positions, and — unless the pixel is static — the twelve matrix
//                     words: aligned 16-byte loads all. Neighbouring lanes mostly share the node and the triangle, so all but the
//                     first load of a line are hits in the CU's vector cache. Writes the pixel's record, two aligned 16-byte
//                     stores. Neither LDS nor scratch memory.
#include "scene_motion.hpp"

namespace {

struct SmChainArgs { const NodeDev *prev, *cur; f4* chains; uint32_t nNodes; };
__global__ void __launch_bounds__(kBlock) k_sm_node_chains(SmChainArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nNodes) return;
  f4 w[kSmChainWords];
  smNodeChain(a.prev, a.cur, i, w);
  for (uint32_t k = 0; k < kSmChainWords; k++) dnSt(a.chains + size_t(i) * kSmChainWords + k, w[k]);
}

struct SmDeviceScene {
  const f4* chains; const MeshDev* meshes; const u4* triVerts; const f4 *vCur, *vPrev;
  uint32_t nNodes;
  __device__ __forceinline__ static u4 asU4(f4 v) { u4 r; r.x = dnBits(v.x); r.y = dnBits(v.y); r.z = dnBits(v.z); r.w = dnBits(v.w); return r; }
  __device__ __forceinline__ uint32_t nodes() const { return nNodes; }
  __device__ __forceinline__ f4 chain(uint32_t node, uint32_t i) const { return dnLd(chains + size_t(node) * kSmChainWords + i); }
  __device__ __forceinline__ u4 mesh(uint32_t m, uint32_t i) const { return asU4(dnLd(reinterpret_cast<const f4*>(meshes + m) + i)); }
  __device__ __forceinline__ u4 tri(size_t t) const { return asU4(dnLd(reinterpret_cast<const f4*>(triVerts + t))); }
  __device__ __forceinline__ f4 cur(size_t v) const { return dnLd(vCur + v); }
  __device__ __forceinline__ f4 prev(size_t v) const { return dnLd(vPrev + v); }
};

struct SmPixelArgs {
  SmDeviceScene sc;
  const float *position, *normal, *coverage;
  const int32_t* ids;                              // 4 per pixel: node, mesh, material, triangle
  f4* records;                                     // kSmRecordWords per pixel
  uint32_t width, height, tilesX;
};
__global__ void __launch_bounds__(kBlock) k_sm_pixels(SmPixelArgs a) {
  const uint32_t ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
  const uint32_t x = tx * 16u + (threadIdx.x % 16u), y = ty * 16u + (threadIdx.x / 16u);
  if (x >= a.width || y >= a.height) return;
  const size_t p = size_t(y) * a.width + x;
  const f3 P = mk3(a.position[p * 3], a.position[p * 3 + 1], a.position[p * 3 + 2]);
  const f3 n = mk3(a.normal[p * 3], a.normal[p * 3 + 1], a.normal[p * 3 + 2]);
  f4 w0, w1;
  smPixel(a.sc, P, n, a.coverage[p], uint32_t(a.ids[p * 4]), uint32_t(a.ids[p * 4 + 3]), w0, w1);
  dnSt(a.records + p * kSmRecordWords, w0);
  dnSt(a.records + p * kSmRecordWords + 1u, w1);
}

void smCheck(bool ok, const char* what) {
  if (!ok) throw std::invalid_argument(std::string("scene_pixel_motion: ") + what);
}

// Everything that can refuse a call, before a device is touched; returns the four buffers it reads
YartAovBuffers smValidate(const YartScene* scene, const YartAovBuffers* aovs, uint32_t width, uint32_t height, const float* records,
                          bool device) {
  smCheck(scene != nullptr, "scene pointer is null");
  smCheck(aovs != nullptr, "feature buffers (aovs) pointer is null");
  smCheck(records != nullptr, "records pointer is null");
  smCheck(width > 0u && height > 0u, "width or height is 0");
  smCheck(uint64_t(width) * height <= (1ull << 28), "more than 2^28 pixels");
  smCheck(!device || (reinterpret_cast<uintptr_t>(records) & 15u) == 0u, "d_records is not 16-byte aligned");
  checkBufferHead(kAovTable, *aovs, "scene_pixel_motion: ");
  YartAovBuffers b{};
  smCheck(takeBufferField(*aovs, kAovTable.field(YART_AOV_POSITION), b), "the position feature buffer (YART_AOV_POSITION) is missing");
  smCheck(takeBufferField(*aovs, kAovTable.field(YART_AOV_NORMAL), b), "the normal feature buffer (YART_AOV_NORMAL) is missing");
  smCheck(takeBufferField(*aovs, kAovTable.field(YART_AOV_COVERAGE), b), "the coverage feature buffer (YART_AOV_COVERAGE) is missing");
  smCheck(takeBufferField(*aovs, kAovTable.field(YART_AOV_IDS), b), "the ids feature buffer (YART_AOV_IDS) is missing");
  return b;
}

// device pointers; the scene's lock held and its device current; returns after completion on `stream`
void smRun(YartScene& s, const YartAovBuffers& b, uint32_t width, uint32_t height, float* records, hipStream_t stream) {
  const uint32_t nn = uint32_t(s.host.nodes.size());
  s.smChains.ensure(size_t(nn) * kSmChainWords);
  SmChainArgs ca{s.nodesPrev.p, s.nodes.p, s.smChains.p, nn};
  hipLaunchKernelGGL(k_sm_node_chains, dim3((nn + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, ca);
  HIP_CHECK(hipGetLastError());
  SmPixelArgs pa{};
  pa.sc = SmDeviceScene{s.smChains.p, s.meshes.p, s.triVerts.p, s.vPos.p, s.vPosPrev.p, nn};
  pa.position = b.position; pa.normal = b.normal; pa.coverage = b.coverage; pa.ids = b.ids;
  pa.records = reinterpret_cast<f4*>(records);
  pa.width = width; pa.height = height; pa.tilesX = (width + 15u) / 16u;
  hipLaunchKernelGGL(k_sm_pixels, dim3(pa.tilesX * ((height + 15u) / 16u)), dim3(kBlock), 0, stream, pa);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
}

}  // namespace

extern "C" {

int yart_hip_scene_keep_previous(YartScene* scene, void* stream) {
  return guarded([&] {
    require(scene != nullptr, "scene_keep_previous: scene pointer is null");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    HIP_CHECK(hipSetDevice(s.device));
    const size_t nn = s.host.nodes.size(), nv = s.host.vPos.size();
    s.nodesPrev.ensure(std::max<size_t>(nn, 1)); s.vPosPrev.ensure(std::max<size_t>(nv, 1));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nn) HIP_CHECK(hipMemcpyAsync(s.nodesPrev.p, s.nodes.p, nn * sizeof(NodeDev), hipMemcpyDeviceToDevice, st));
    if (nv) HIP_CHECK(hipMemcpyAsync(s.vPosPrev.p, s.vPos.p, nv * sizeof(f4), hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    s.havePrevious = true;
  });
}

int yart_hip_scene_pixel_motion_device(YartScene* scene, const YartAovBuffers* d_aovs, uint32_t width, uint32_t height, float* d_records,
                                       void* stream) {
  return guarded([&] {
    const YartAovBuffers b = smValidate(scene, d_aovs, width, height, d_records, true);
    std::lock_guard<std::mutex> lock(scene->mu);
    smCheck(scene->havePrevious, "yart_hip_scene_keep_previous was never called on this scene");
    HIP_CHECK(hipSetDevice(scene->device));
    smRun(*scene, b, width, height, d_records, static_cast<hipStream_t>(stream));
  });
}

int yart_hip_scene_pixel_motion_host(YartScene* scene, const YartAovBuffers* aovs, uint32_t width, uint32_t height, float* records) {
  return guarded([&] {
    const YartAovBuffers b = smValidate(scene, aovs, width, height, records, false);
    std::lock_guard<std::mutex> lock(scene->mu);
    smCheck(scene->havePrevious, "yart_hip_scene_keep_previous was never called on this scene");
    HIP_CHECK(hipSetDevice(scene->device));
    // records (8) | position (3) | normal (3) | coverage (1) | ids (4) words per pixel
    const size_t n = size_t(width) * height;
    scene->smStage.ensure(n * 19);
    float* w = scene->smStage.p + n * 8;
    YartAovBuffers d{};
    auto put = [&](const void* src, size_t words) {
      float* dst = w; w += n * words;
      HIP_CHECK(hipMemcpy(dst, src, n * words * 4, hipMemcpyHostToDevice));
      return dst;
    };
    d.position = put(b.position, 3); d.normal = put(b.normal, 3); d.coverage = put(b.coverage, 1);
    d.ids = reinterpret_cast<int32_t*>(put(b.ids, 4));
    smRun(*scene, d, width, height, scene->smStage.p, nullptr);
    HIP_CHECK(hipMemcpy(records, scene->smStage.p, n * 8 * 4, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
