// yart_hip.hip — unit 0 of libyart_hip.so: the frame kernels, the host side of a render and the C ABI.
//
// Stands where reference cpu/tile-renderer.hpp:118-309 (TileRenderer::renderImpl /
// finishTile) and cpu/integrator.cpp:5-28 (Integrator::render) stand: tiles of the
// image are rendered for `waveSamples` samples per pixel, each pixel's samples go
// through GMoN, and waves are blended into the HDR framebuffer. The thread pool of
// the reference becomes a persistent grid; the per-sample work is in integrator.hpp.
//
// Kernels in this file
//   k_render_mega   one lane = one (pixel, sample) path from camera to termination
//                   (BASELINE config "megakernel integrator"); persistent waves pull
//                   64 paths at a time from an atomic cursor; LDS traversal stack.
//   k_gmon_blend    one wave = one pixel: bucket sums in sample order, GMoN value,
//                   blend into the HDR buffer (integrator.cpp:17-25, tile-renderer.hpp:220-232).
//   k_tile_rays     ray counts per pixel block (tile callbacks);  k_tex_quads  the textures' 2x2 footprint records, at upload.
// Host side in this file: YartScene and its upload, the render plan, the batch runners and the wave loop (renderToDevice), and the
// scene, render, multi-device, debug and BVH entries of the C ABI.
//
// The library is five translation units (csrc/Makefile), so that the device code builds in parallel. Which file a unit compiles
// decides what it emits; every kernel is emitted in exactly one unit:
//   unit 0     yart_hip.hip (this file), with
//                stream_kernels.inc     the streaming passes of the wavefront pipelines and the sampler tables
//                aov_kernels.inc, moment_kernels.inc, bvh_build_device.inc      feature buffers, sample moments, the device BVH build
//                multi_device.inc       several GPUs behind one handle, with its pixel pack / unpack / copy kernels
//                postprocess.inc        tonemap / encode, the a-trous denoiser (denoise_kernels.inc) and temporal accumulation
//                                       (temporal_kernels.inc): kernels, drivers and entries
//                scene_update_common.inc, tlas_build_kernels.inc, scene_update_kernels.inc, graph_update_kernels.inc, mesh_update_kernels.inc, lighting_update_kernels.inc, texture_update_kernels.inc,
//                scene_motion_kernels.inc      a scene's next frame in place: new transforms, a new node list, new vertices, new materials / light
//                                       emission / environment images, new texels of material textures, and the per-pixel motion
//                                       between the two frames
//                probes.inc             the diagnostic kernels k_probe_* and the yart_hip_probe_* entries
//   units 1-4  wavefront_units.hip under -DYART_TU=1..4: the path kernels, which are templates and are emitted where they are
//              instantiated — 1 the lean closest-hit kernels k_wf_extend_lean<MODE, NODES>, 2 the lean any-hit kernels
//              k_wf_shadow_lean<MODE, NODES>, 3 the retry (resumed walks), one-ray-per-lane lean and general kernels, 4 the shade
//              kernel k_wf_shade<SORT, FIT, ENV1>
//   all five   hip_common.hpp (constants, HIP_CHECK, DevBuf), wavefront_kernels.inc (WfArgs, the queue helpers, the path
//              kernels' templates: unit 0 needs the types and instantiates none) and kernel_units.hpp (yart_hip::tu: the
//              type-erased host stubs through which unit 0 launches the kernels of units 1-4)
#include "hip_common.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "../../include/yart_hip.h"
#include "estimator.hpp"
#include "host_scene.hpp"
#include "tlas_build.hpp"
#include "graph_update.hpp"
#include "mesh_update.hpp"
#include "mesh_replace.hpp"
#include "lighting_update.hpp"
#include "texture_update.hpp"
#include "integrator.hpp"
#include "scene_file.hpp"
#include "gltf_reader.hpp"
#include "wavefront.hpp"
#include "trace_lean.hpp"
#include "moments.hpp"
#include "trace_ranges.hpp"
#include "kernel_units.hpp"

using namespace yart_hip;

namespace {

constexpr uint64_t kDefaultBatchPaths = 1ull << 28;   // YartRenderParams::max_batch_paths = 0: 268 M paths (batch-synchronous: 67 GB; path pool: 4.3 GB of per-sample records)
constexpr uint64_t kDefaultPoolPaths = 1ull << 25;    // YartRenderParams::pool_paths = 0: 33.5 M slots, 5.6 GB
constexpr int kPoolLag = 4;                            // the host looks at the counters of the round before the previous one (ring of 4)

thread_local std::string g_lastError;

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
struct MegaArgs {
  SceneDev sc;
  CameraDev cam;
  RenderConst rc;
  const uint32_t* pixels;      // packed x | y << 16, tile-major order
  uint32_t nPixels, spp, sampleOffset, pad;
  f4* L;                    // 3 floats per (pixel, sample)
  uint32_t* cursor;
  unsigned long long* rays;
  uint64_t* spill;             // kSpillDepth entries per launched thread, lane-interleaved
  // feature buffers (k_render_mega<true> only): the three record arrays (per path of the batch) and the ids of sample 0 (per pixel of the rank)
  f4 *aov0, *aov1, *aov2;
  int32_t* aovIds;
  uint32_t pixBase, padA;
};

// AOV: also writes the feature record of every path's first hit (aov.hpp); <false> is the kernel as it was before feature buffers existed
template <bool AOV>
__global__ void __launch_bounds__(kBlock) k_render_mega(MegaArgs a) {
  __shared__ uint64_t ldsStack[kLdsStack * kBlock];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nthreads = gridDim.x * blockDim.x;
  PathCtx cx;
  cx.sc = &a.sc;
  cx.sobol = reinterpret_cast<const uint32_t*>(a.sc.lut + LutDev::sobol);
  cx.stk.lds = (lds_u64*)(ldsStack + threadIdx.x); cx.stk.ldsStride = kBlock; cx.stk.ldsDepth = kLdsStack;
  cx.stk.spill = a.spill + gtid; cx.stk.spillStride = nthreads;
  cx.rc = a.rc;
  const uint32_t total = a.nPixels * a.spp;
  uint32_t rays = 0;
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.cursor, 64u);
    base = __shfl(base, 0);
    if (base >= total) break;            // wave-uniform exit: every wave drains the cursor
    const uint32_t w = base + lane;
    if (w < total) {
      const uint32_t pi = w / a.spp, s = w - pi * a.spp;
      const uint32_t pk = a.pixels[pi];
      const uint32_t before = rays;
      AovRecord rec; AovIds ids;
      f3 L = samplePixel<AOV>(cx, a.cam, pk & 0xffffu, pk >> 16, s + a.sampleOffset, rays, &rec, &ids);
      a.L[w] = mk4(L.x, L.y, L.z, asF(rays - before));
      if (AOV) {
        wfSt(a.aov0 + w, rec.r0); wfSt(a.aov1 + w, rec.r1); wfSt(a.aov2 + w, rec.r2);
        if (s + a.sampleOffset == 0u) {
          int32_t* o = a.aovIds + size_t(a.pixBase + pi) * 4;
          o[0] = ids.node; o[1] = ids.mesh; o[2] = ids.material; o[3] = ids.tri;
        }
      }
    }
  }
  // one atomic per wave
  unsigned long long r = rays;
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o);
  if (lane == 0 && r) atomicAdd(a.rays, r);
#if defined(YART_COUNT_TRAVERSAL)
  unsigned long long c[4] = {cx.nTrav, cx.nBox, cx.nTri, cx.nShade};
  for (int k = 0; k < 4; k++) {
    unsigned long long v = c[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0 && v) atomicAdd(a.rays + 1 + k, v);
  }
#endif
}

struct GmonArgs {
  const f4* L;                 // per (pixel, sample): radiance.xyz, ray count
  uint32_t* pixRays;           // per pixel of the batch: the wave's ray count of that pixel (nullptr: not wanted)
  const uint32_t* pixels;
  uint32_t nPixels, spp, width;
  int kind;                    // EstimatorKind
  float exposureScale, wCurrent, wWave, pad1;
  float* hdr;                  // RGBA32F, width * height
};

// 16 lanes per pixel (lane b < m sums bucket b in increasing sample order, as the reference's
// accumulation does), 4 pixels per wave; the serial GMoN tail runs on one lane per pixel.
constexpr int kGmonLanes = 16;
static_assert(kGmonMax <= kGmonLanes, "one lane per bucket");
constexpr int kGmonPixPerBlock = kBlock / kGmonLanes;
__global__ void __launch_bounds__(kBlock) k_gmon_blend(GmonArgs a) {
  // bucket sums / counts live in LDS and are sorted there: private arrays with run-time indices would be scratch
  __shared__ f3 sAcc[kGmonPixPerBlock][kGmonMax];
  __shared__ uint32_t sCnt[kGmonPixPerBlock][kGmonMax];
  const uint32_t sub = threadIdx.x & (kGmonLanes - 1), lp = threadIdx.x / kGmonLanes;
  const uint32_t pi = blockIdx.x * kGmonPixPerBlock + lp;
  const bool valid = pi < a.nPixels;
  const int m = estimatorBuckets(a.kind, int32_t(a.spp));
  __shared__ uint32_t sRays[kGmonPixPerBlock][kGmonMax];
  if (valid && int(sub) < m) {
    f3 acc = mk3(0); uint32_t cnt = 0, rays = 0;
    const f4* p = a.L + size_t(pi) * a.spp;
    // bucket k mod m, increasing k; four samples' loads in flight, accumulated in order
    const uint32_t um = uint32_t(m);
    uint32_t s = sub;
    for (; s + 3u * um < a.spp; s += 4u * um) {
      f4 v[4];
      for (uint32_t j = 0; j < 4u; j++) v[j] = p[s + j * um];
      for (uint32_t j = 0; j < 4u; j++) {
        const f3 w = mk3(v[j].x, v[j].y, v[j].z) * a.exposureScale;
        if (estimatorAccepts(a.kind, w)) { acc += w; cnt++; }
        rays += __builtin_bit_cast(uint32_t, v[j].w);
      }
    }
    for (; s < a.spp; s += um) {
      const f4 q = p[s];
      f3 v = mk3(q.x, q.y, q.z) * a.exposureScale;
      if (estimatorAccepts(a.kind, v)) { acc += v; cnt++; }
      rays += __builtin_bit_cast(uint32_t, q.w);
    }
    sAcc[lp][sub] = acc;
    sCnt[lp][sub] = cnt;
    sRays[lp][sub] = rays;
  }
  __syncthreads();
  if (valid && sub == 0 && a.pixRays != nullptr) {
    uint32_t r = 0;
    for (int b = 0; b < m; b++) r += sRays[lp][b];
    a.pixRays[pi] = r;
  }
  if (valid && sub == 0) {
    f3 v = estimatorFinish(a.kind, sAcc[lp], sCnt[lp], m, a.spp);
    const uint32_t pk = a.pixels[pi];
    float* o = a.hdr + (size_t(pk >> 16) * a.width + (pk & 0xffffu)) * 4;
    // m_hdrBuffer = current * wCurrent + wave * wWave   (tile-renderer.hpp:230)
    o[0] = o[0] * a.wCurrent + v.x * a.wWave;
    o[1] = o[1] * a.wCurrent + v.y * a.wWave;
    o[2] = o[2] * a.wCurrent + v.z * a.wWave;
    o[3] = o[3] * a.wCurrent + 1.0f * a.wWave;
  }
}

// Renderer::TileData.rays (renderer.hpp:40-50; tile-renderer.hpp:183 passes the tile integrator's ray count): per pixel block of
// this rank the sum of its pixels' ray counts of the wave (k_gmon_blend's pixRays); one wave per block
__global__ void __launch_bounds__(64) k_tile_rays(const uint32_t* pixRays, const uint32_t* tileStart, const uint32_t* tileCount,
                                                  uint32_t firstTile, uint32_t nTiles, unsigned long long* out) {
  const uint32_t t = firstTile + blockIdx.x;
  if (blockIdx.x >= nTiles) return;
  unsigned long long r = 0;
  for (uint32_t i = threadIdx.x; i < tileCount[t]; i += 64u) r += pixRays[tileStart[t] + i];
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o);
  if (threadIdx.x == 0) out[t] = r;
}

// 2x2 footprint records of one texture (scene_types.hpp TexDev::quadOffset), expanded on the device at upload from the plain
// texel arrays: record (x, y) = the four taps texture.cpp:21-35 reads for a lookup whose base texel is (x, y)
struct TexQuadArgs { const uint8_t* u8; const float* f32; TexDev t; uint8_t* out; };
__global__ void __launch_bounds__(kBlock) k_tex_quads(TexQuadArgs a) {
  const uint32_t w = a.t.width, h = a.t.height, C = a.t.channels;
  const uint32_t rec = texQuadRecordBytes(C, a.t.isFloat);
  const uint32_t stride = a.t.quadStride ? a.t.quadStride : rec;     // (a record inside a material's shared 64-byte record)
  const size_t n = size_t(w) * h;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    const uint32_t x = uint32_t(i % w), y = uint32_t(i / w);
    const uint32_t x1 = x + 1u < w ? x + 1u : x, y1 = y + 1u < h ? y + 1u : y;      // (records of the last column / row are never read)
    const size_t idx[4] = {size_t(y) * w + x, size_t(y1) * w + x, size_t(y) * w + x1, size_t(y1) * w + x1};
    uint8_t* o = a.out + i * stride;
    if (a.t.isFloat) {
      float* of = reinterpret_cast<float*>(o);
      for (uint32_t k = 0; k < rec / 4u; k++) of[k] = 0.0f;
      for (uint32_t tap = 0; tap < 4u; tap++)
        for (uint32_t c = 0; c < C; c++) of[tap * C + c] = a.f32[size_t(a.t.offset) + C * idx[tap] + c];
    } else {
      uint32_t word[4];
      for (uint32_t tap = 0; tap < 4u; tap++) {
        word[tap] = 0u;
        for (uint32_t c = 0; c < C; c++) word[tap] |= uint32_t(a.u8[size_t(a.t.offset) + C * idx[tap] + c]) << (8u * c);
      }
      uint32_t* ow = reinterpret_cast<uint32_t*>(o);
      if (C >= 3u) { ow[0] = word[0]; ow[1] = word[1]; ow[2] = word[2]; ow[3] = word[3]; }
      else if (C == 2u) { ow[0] = word[0] | (word[1] << 16); ow[1] = word[2] | (word[3] << 16); }
      else ow[0] = word[0] | (word[1] << 8) | (word[2] << 16) | (word[3] << 24);
    }
  }
}

#include "wavefront_kernels.inc"     // what every unit shares, and the path kernels' templates (instantiated in units 1-4 only)
#include "stream_kernels.inc"
#include "aov_kernels.inc"
#include "moment_kernels.inc"
#include "bvh_build_device.inc"

static_assert(devbvh::kMaxLevels == int(kMaxStackBound), "the stack bound's cap is the device builder's level limit");
// Spill entries per lane for a scene: what they always were (the reference's 64-entry stack) unless one of the scene's trees
// needs more (host_scene.hpp: HostImage::stackBound, at most kMaxStackBound — deeper meshes do not get past scene creation).
// wholeStack: the area is sized for the whole stack (the render kernels: their LDS parts differ, the shallowest has 8 entries);
// otherwise for what lies beyond the kLdsStack entries of the probe kernels.
static size_t spillDepthFor(const HostImage& im, bool wholeStack) {
  if (wholeStack) return size_t(std::max<uint32_t>(uint32_t(kSpillDepthMax), im.stackBound));
  return size_t(std::max<int>(kSpillDepth, int(im.stackBound) - kLdsStack));
}
}  // namespace
#include "render_host.hpp"     // (host only: the wave schedule and the buffer tables)
namespace {
typedef void (*WfKernelFn)(WfArgs);
inline WfKernelFn wfKernel(yart_hip::tu::AnyKernel k) { return reinterpret_cast<WfKernelFn>(k); }

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct Timer {
  hipEvent_t a{}, b{};
  Timer() { HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b)); }
  ~Timer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
};

}  // namespace

// What a device build of the top-level hierarchy keeps (tlas_build_kernels.inc): the tables of a leaf list — its shape and the leaves'
// first order, on the host and uploaded — and the working arrays: the leaves' current order, the keys, the ranges' centre extents.
struct TlasBuildState {
  bool ready = false;
  TlasShape shape;
  std::vector<uint32_t> leafIds;
  DevBuf<uint32_t> dLeafIds, dRecA, dOrder, dRoots, ids, ext;
  DevBuf<unsigned long long> keys;
};

// What yart_hip_scene_update keeps per scene (scene_update_kernels.inc): tables of the topology, built at the first update, and
// the staging buffers of the uploaded transforms.
struct SceneUpdateTables {
  bool ready = false, tlasReady = false;
  uint32_t levels = 0;                                  // levels of the scene graph (deepest node's depth + 1)
  DevBuf<uint32_t> parents, childOff, childIdx;         // nodes with children by level; their children as a CSR list
  std::vector<uint32_t> levelFirst, levelBig, levelSmall;   // per level: its range of `parents` (kSuFanOut and more children first)
  DevBuf<SuBox> meshBox;
  DevBuf<uint32_t> tlasOrder; std::vector<uint32_t> tlasFirst;   // the top-level tree's nodes by level
  DevBuf<uint32_t> stageDesc, stageFlags;
  TlasBuildState tlasBuild;                             // YART_UPDATE_REBUILD_TOP_DEVICE: allocated at its first use
};

// What yart_hip_scene_update_meshes keeps per scene (mesh_update_kernels.inc), all grown on demand so that an animation allocates
// nothing per frame: the device build's working arrays, per listed mesh the staging arrays a rebuilt mesh waits in until every
// listed mesh has built, and the second node array the meshes are repacked into when a node count changes.
struct MeshStage {
  DevBuf<float> pos, nrm, tan;                          // the caller's arrays, packed as given
  DevBuf<BvhNode> nodes; DevBuf<uint32_t> idx; DevBuf<LeafTri> leaf;
  std::vector<uint32_t> idxHost;
  uint32_t nNodes = 0, hasAlpha = 0, need = 0;
  // yart_hip_scene_replace_meshes (mesh_replace_kernels.inc) only: the caller's uvs and faces, and the mesh's records of the pools
  // that are indexed by triangle and by vertex, as create lays them out
  DevBuf<float> uv;
  DevBuf<u4> faces; DevBuf<int32_t> light; DevBuf<ShadeTri> shade;
  DevBuf<f4> vPos, vNormal, vTangent; DevBuf<f2> vUV;
};
// The second array of every pool yart_hip_scene_replace_meshes repacks (bvhNodes: MeshUpdateState::nodesAlt, which
// yart_hip_scene_update_meshes repacks into as well). A repack writes the second array and swaps the two, so each holds the pool of
// the frame before; grown by half beyond what a frame needs, and kept.
struct MeshReplacePools {
  DevBuf<ShadeTri> shadeTris; DevBuf<LeafTri> leafTris; DevBuf<u4> triVerts; DevBuf<int32_t> triLight;
  DevBuf<f4> vPos, vNormal, vTangent; DevBuf<f2> vUV;
  DevBuf<MrSource> segments;                            // the segment tables of one call, pool after pool
};
struct MeshUpdateState {
  devbvh::Scratch scratch;
  std::vector<std::unique_ptr<MeshStage>> stages;
  DevBuf<uint32_t> prefix, result;
  DevBuf<BvhNode> nodesAlt;
  MeshReplacePools alt;
  std::vector<int8_t> meshAlpha;                        // per mesh: a face has an alpha-tested material (-1: not looked at yet)
};

// What yart_hip_scene_update_lighting keeps per scene (lighting_update_kernels.inc): the material descriptors as the scene was last
// given them (create's, then an update's: what an update's tex_* / thin_transmission are compared with), and per EnvDev record the
// sequential texel sum of its map (Lavg's numerator), taken when an update first needs it.
struct LightingUpdateState {
  std::vector<YartMaterialDesc> materialDesc;
  std::vector<LuSum> envSum; std::vector<uint8_t> envSumKnown;
};

// What yart_hip_scene_update_textures keeps per scene (texture_update_kernels.inc): the words its kernels report in, and per mesh
// the materials of its faces, listed when a material's alpha flag first changes.
struct TextureUpdateState {
  DevBuf<uint32_t> result;
  std::vector<std::vector<uint32_t>> meshMaterials;
};

// What yart_hip_scene_update_graph keeps per scene (graph_update_kernels.inc): the last call's topology pass — the host arrays its
// copies on the stream read — and the staged topology records.
struct GraphUpdateState {
  GuDerived derived;
  DevBuf<uint32_t> stageTopo;
};

// The scenes that exist: what YART_UPDATE_REBUILD_TOP_DEVICE is checked against before an update reads its handle
// (scene_update_common.inc::checkDeviceRebuildHandle). (Never destroyed: scenes may outlive the library's static objects at exit.)
struct SceneRegistry {
  std::mutex mu;
  std::unordered_set<const void*> live;
  static SceneRegistry& get() { static SceneRegistry* r = new SceneRegistry; return *r; }
  void add(const void* s) { std::lock_guard<std::mutex> l(mu); live.insert(s); }
  void remove(const void* s) { std::lock_guard<std::mutex> l(mu); live.erase(s); }
  bool has(const void* s) { std::lock_guard<std::mutex> l(mu); return live.count(s) != 0; }
};

struct YartScene {
  YartScene() { SceneRegistry::get().add(this); }
  int device = 0;
  HostImage host;
  SceneDev dev{};
  int numCUs = 256;
  bool texQuadsOn = true;      // the textures' 2x2 footprint records are on the device (uploadScene: they fit the budget)
  // device copies of the scene image
  DevBuf<f4> resumeRec; DevBuf<ShadeTri> shadeTris; DevBuf<BvhNode> bvhNodes; DevBuf<LeafTri> leafTris; DevBuf<u4> triVerts; DevBuf<int32_t> triLight;
  DevBuf<f4> vPos, vNormal, vTangent; DevBuf<f2> vUV; DevBuf<MeshDev> meshes; DevBuf<NodeDev> nodes;
  DevBuf<MaterialDev> materials; DevBuf<TexDev> textures; DevBuf<uint8_t> texU8; DevBuf<float> texF32; DevBuf<uint8_t> texQuads;
  DevBuf<LightDev> lights; DevBuf<EnvDev> envs; DevBuf<float> envData; DevBuf<uint32_t> envGuide; DevBuf<f4> nodeWorld; DevBuf<TlasNode> tlas; DevBuf<unsigned long long> nodeBits;
  DevBuf<uint32_t> infiniteLights, areaLights; DevBuf<float> areaPowerCdf; DevBuf<float> lut;
  DevBuf<uint8_t> matClass;                // host_scene.hpp::lobeClass per material
  // render scratch (grown on demand, reused across calls)
  DevBuf<uint32_t> pixels; DevBuf<f4> L; DevBuf<uint32_t> cursor; DevBuf<unsigned long long> counters;
  DevBuf<uint32_t> pixRays, tileStart, tileCount; DevBuf<unsigned long long> tileRays;   // per-block ray counts (tile callbacks only)
  std::vector<unsigned long long> tileRaysHost;
  DevBuf<uint64_t> spill; DevBuf<float> hdr; DevBuf<uint32_t> probeIn; DevBuf<float> probeOut;
  DevBuf<f4> wf[9];                        // wavefront path state (wavefront.hpp::WfState)
  DevBuf<f4> wfTail[1][9];                 // compacted state of the late bounces (1/2 of the batch; the second one is the batch-sized state itself)
  DevBuf<uint32_t> wfTailMap[2];
  DevBuf<WfDyn> wfDyn;
  DevBuf<unsigned long long> pathsLog;     // paths entering bounce b, summed over the batches of a render (YartStats::paths_at_bounce)
  // feature buffers (aov_kernels.inc): running sums / ray counts / ids per pixel of the rank; the records of the megakernel and path-pool
  // pipelines (3 x 16 B per path of the batch); the device side of the host-pointer entry point's buffers
  DevBuf<f4> aovAcc[3], aovRec; DevBuf<uint32_t> aovRays; DevBuf<int32_t> aovIds; DevBuf<uint32_t> aovOut;
  // sample moments (moment_kernels.inc): the running state per pixel of the rank, and the host entry point's staging buffers
  DevBuf<MomentState> momState; DevBuf<uint32_t> momOut;
  DevBuf<uint32_t> poolMap;                // path pool: the path (index of L) each slot carries, kWfFreeSlot = free
  uint32_t* poolHost = nullptr;            // pinned: the queue counters of the last rounds (the host's view of "is the batch done")
  ~YartScene() { SceneRegistry::get().remove(this); if (poolHost) (void)hipHostFree(poolHost); }
  DevBuf<uint32_t> qA, qB, qS, qR, wfCounters; // wavefront queues
  DevBuf<uint64_t> smpEntries, smpHash; DevBuf<uint32_t> smpSobol1;   // SamplerTables of the current render
  std::vector<uint32_t> pixelsHost;
  struct TileRec { uint32_t x, y, w, h, start, count; };     // a pixel block of this rank: its rectangle and its range of pixelsHost
  std::vector<TileRec> tiles;
  unsigned long long lastCounters[32] = {0};
  uint32_t pixW = 0, pixH = 0, pixTile = 0, pixRank = 0, pixWorld = 0;
  SceneUpdateTables su;
  MeshUpdateState meshUp;
  LightingUpdateState lightUp;
  TextureUpdateState texUp;
  GraphUpdateState graphUp;
  // yart_hip_scene_keep_previous (scene_motion_kernels.inc): the node and vertex arrays of the previous frame, allocated by the first
  // call; the nodes' composed transforms and the host entry's staging buffer of yart_hip_scene_pixel_motion_*
  DevBuf<NodeDev> nodesPrev; DevBuf<f4> vPosPrev, smChains; DevBuf<float> smStage;
  bool havePrevious = false;
  std::mutex mu;
};

namespace {

void uploadScene(YartScene& s) {
  const HostImage& h = s.host;
  s.shadeTris.upload(h.shadeTris);
  s.bvhNodes.upload(h.bvhNodes); s.leafTris.upload(h.leafTris); s.triVerts.upload(h.triVerts);
  s.triLight.upload(h.triLight); s.vPos.upload(h.vPos); s.vNormal.upload(h.vNormal);
  s.vTangent.upload(h.vTangent); s.vUV.upload(h.vUV); s.meshes.upload(h.meshes); s.nodes.upload(h.nodes);
  s.materials.upload(h.materials); s.textures.upload(h.textures); s.texU8.upload(h.texU8);
  s.texF32.upload(h.texF32); s.lights.upload(h.lights); s.envs.upload(h.envs); s.envData.upload(h.envData); s.envGuide.upload(h.envGuide); s.nodeWorld.upload(h.nodeWorld); s.tlas.upload(h.tlas);
  s.infiniteLights.upload(h.infiniteLights); s.areaLights.upload(h.areaLights);
  s.areaPowerCdf.upload(h.areaPowerCdf); s.lut.upload(h.lut);
  {
    std::vector<uint8_t> cls;
    for (const MaterialDev& m : h.materials) cls.push_back(lobeClass(m));
    while (cls.size() % 4u) cls.push_back(0);          // (the shade kernel copies the classes into LDS a word at a time)
    s.matClass.upload(cls);
  }
  // The textures' 2x2 footprint records: expanded here from the plain texel arrays just uploaded — unless they do not fit a
  // budget: more than a third of the free device memory (or YART_TEX_QUADS_MAX_MB megabytes) and the kernels take their bilinear
  // taps from the plain texel arrays (bsdf.hpp::texQuad: sc.texQuads == nullptr; same taps, same arithmetic, same frame).
  bool quads = true;
  {
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    size_t budget = freeB / 3;
    if (const char* e = std::getenv("YART_TEX_QUADS_MAX_MB")) budget = size_t(std::max<long long>(0, std::atoll(e))) << 20;
    if (h.texQuadUnits * 16u > budget) quads = false;
  }
  s.texQuadsOn = quads;
  s.texQuads.ensure(quads ? std::max<size_t>(h.texQuadUnits, 1) * 16u : 16u);
  for (const TexDev& t : h.textures) {
    if (!quads || t.width == 0u || t.quadOffset == kNoTexQuads) continue;
    TexQuadArgs qa{s.texU8.p, s.texF32.p, t, s.texQuads.p + size_t(t.quadOffset) * 16u};
    const size_t n = size_t(t.width) * t.height;
    hipLaunchKernelGGL(k_tex_quads, dim3(uint32_t(std::min<size_t>((n + kBlock - 1) / kBlock, 65535u))), dim3(kBlock), 0, nullptr, qa);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipDeviceSynchronize());
  SceneDev d = h.view();       // counts and totals; pointers replaced below
  d.shadeTris = s.shadeTris.p;
  d.bvhNodes = s.bvhNodes.p; d.leafTris = s.leafTris.p; d.triVerts = s.triVerts.p; d.triLight = s.triLight.p;
  d.vPos = s.vPos.p; d.vNormal = s.vNormal.p; d.vTangent = s.vTangent.p; d.vUV = s.vUV.p;
  d.meshes = s.meshes.p; d.nodes = s.nodes.p; d.materials = s.materials.p; d.textures = s.textures.p;
  d.texU8 = s.texU8.p; d.texF32 = s.texF32.p; d.texQuads = s.texQuadsOn ? s.texQuads.p : nullptr; d.lights = s.lights.p; d.envs = s.envs.p;
  d.envData = s.envData.p; d.envGuide = s.envGuide.p; d.nodeWorld = s.nodeWorld.p; d.tlas = s.tlas.p; d.nTlas = h.tlas.size() > 1 || (h.tlas.size() == 1 && h.tlas[0].b) ? uint32_t(h.tlas.size()) : 0u; d.infiniteLights = s.infiniteLights.p; d.areaLights = s.areaLights.p;
  d.areaPowerCdf = s.areaPowerCdf.p; d.lut = s.lut.p;
  s.dev = d;
}

int resolveDevice(int device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) return -1;
  if (device < 0) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return -1;
    return cur;
  }
  return device < count ? device : -1;
}

// the device build of one mesh's BVH (same bytes as the host build; a mesh it refuses — NaN coordinates — is left to the host)
static bool deviceMeshBvh(void* ctx, const float* positions, uint32_t nVerts, const uint32_t* faces, uint32_t stride, uint32_t nFaces,
                          std::vector<BvhNode>& nodes, std::vector<uint32_t>& indices) {
  // any failure of the device build (out of device memory for its scratch arrays, ...) leaves the mesh to the host builder
  try {
    return devbvh::build(*static_cast<int*>(ctx), positions, nVerts, faces, stride, nFaces, nodes, indices, nullptr);
  } catch (const std::exception&) {
    (void)hipGetLastError();
    nodes.clear(); indices.clear();
    return false;
  }
}
YartScene* createScene(const YartSceneDesc& desc, int device, uint32_t sceneFlags = 0) {
  int dev = resolveDevice(device);
  if (dev < 0) throw HipError("no usable HIP device (libyart_hip has no CPU fallback)");
  HIP_CHECK(hipSetDevice(dev));
  auto s = std::make_unique<YartScene>();
  s->device = dev;
  // the meshes' BVHs are built on the device unless the caller (YART_SCENE_HOST_BVH) or the environment (YART_HOST_BVH) asks
  // for the host builder; the two give the same bytes, and every GPU test that compares a frame with the reference's checks it
  if ((sceneFlags & YART_SCENE_HOST_BVH) || std::getenv("YART_HOST_BVH")) s->host = buildHostImage(desc);
  else s->host = buildHostImage(desc, deviceMeshBvh, &dev);
  if (desc.n_materials) s->lightUp.materialDesc.assign(desc.materials, desc.materials + desc.n_materials);
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  s->numCUs = prop.multiProcessorCount;
  uploadScene(*s);
  return s.release();
}

uint32_t morton2(uint32_t x, uint32_t y) { return uint32_t(encodeMorton2(x, y)); }

// Pixels of the tiles this rank owns, tile-major (row-major inside a tile). Tiles are
// the reference's unit of parallel work (tile-renderer.hpp:126-144); across ranks they
// are dealt round-robin in Morton order.
std::vector<uint32_t> makePixelList(uint32_t W, uint32_t H, uint32_t tile, uint32_t rank, uint32_t world,
                                    std::vector<YartScene::TileRec>* tilesOut) {
  const uint32_t tx = (W + tile - 1) / tile, ty = (H + tile - 1) / tile;
  std::vector<std::pair<uint32_t, uint32_t>> order;   // (morton, linear tile)
  for (uint32_t y = 0; y < ty; y++)
    for (uint32_t x = 0; x < tx; x++) order.push_back({morton2(x, y), y * tx + x});
  std::sort(order.begin(), order.end());
  std::vector<uint32_t> pixels;
  if (tilesOut) tilesOut->clear();
  for (size_t k = 0; k < order.size(); k++) {
    if (k % world != rank) continue;
    const uint32_t x0 = (order[k].second % tx) * tile, y0 = (order[k].second / tx) * tile;
    const uint32_t x1 = std::min(W, x0 + tile), y1 = std::min(H, y0 + tile);
    if (tilesOut) tilesOut->push_back({x0, y0, x1 - x0, y1 - y0, uint32_t(pixels.size()), (x1 - x0) * (y1 - y0)});
    for (uint32_t y = y0; y < y1; y++)
      for (uint32_t x = x0; x < x1; x++) pixels.push_back(x | (y << 16));
  }
  return pixels;
}
void buildPixelList(YartScene& s, uint32_t W, uint32_t H, uint32_t tile, uint32_t rank, uint32_t world) {
  if (s.pixW == W && s.pixH == H && s.pixTile == tile && s.pixRank == rank && s.pixWorld == world) return;
  s.pixelsHost = makePixelList(W, H, tile, rank, world, &s.tiles);
  s.pixels.upload(s.pixelsHost);
  {
    std::vector<uint32_t> start, count;
    for (const YartScene::TileRec& t : s.tiles) { start.push_back(t.start); count.push_back(t.count); }
    s.tileStart.upload(start); s.tileCount.upload(count);
  }
  s.pixW = W; s.pixH = H; s.pixTile = tile; s.pixRank = rank; s.pixWorld = world;
}

void validate(const YartCameraDesc* cam, const YartRenderParams* p) {
  require(cam && p, "camera / params pointer is null");
  require(cam->width > 0 && cam->height > 0 && cam->width < 65536 && cam->height < 65536,
          "image size must be in [1, 65535]");
  require(p->samples > 0 && p->first_wave_samples > 0 && p->max_wave_samples > 0, "sample counts must be > 0");
  require(p->tile_size > 0 && p->tile_size <= 4096, "tile_size out of range");
  require(p->shard_tile <= 4096, "shard_tile out of range");
  require(p->world_size > 0 && p->rank < p->world_size, "rank / world_size");
  // (the path flags keep the depth in 8 bits and the count of unoccluded NEE rays in the next 8: wavefront.hpp WF_DEPTH_MASK / WF_NEE_MASK)
  require(p->max_depth > 0 && p->max_depth <= 255, "max_depth must be in [1, 255]");
  require(p->start_sample < p->samples && (p->stop_sample == 0 || (p->stop_sample > p->start_sample && p->stop_sample <= p->samples)),
          "start_sample / stop_sample out of range");
  require(p->estimator <= YART_ESTIMATOR_GMONB, "estimator must be one of YART_ESTIMATOR_*");
}

RenderConst makeRenderConst(const YartRenderParams& p) {
  RenderConst rc;
  // the sampler is constructed with the TOTAL sample count and the tile size
  // (tile-renderer.hpp:153-156)
  rc.sampler = makeSamplerConfig(p.samples, p.tile_size);
  rc.maxDepth = p.max_depth;
  rc.background = mk3(p.background[0], p.background[1], p.background[2]);
  return rc;
}

int persistentGrid(const YartScene& s, const void* kernel, int cap, int block = kBlock) {
  int perCU = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, block, 0));
  if (perCU < 1) perCU = 1;
  if (perCU > cap) perCU = cap;
  return s.numCUs * perCU;
}

// HIP-event stopwatch for one class of launches on the render stream: record(begin/end)
// around each launch, resolve() after the stream has been synchronised.
struct StageTimer {
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  double ms = 0.0;
  uint32_t launches = 0;
  ~StageTimer() { for (auto e : ev) (void)hipEventDestroy(e); }
  hipEvent_t next() {
    if (used == ev.size()) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); ev.push_back(e); }
    return ev[used++];
  }
  void begin(hipStream_t st) { HIP_CHECK(hipEventRecord(next(), st)); }
  void end(hipStream_t st) { HIP_CHECK(hipEventRecord(next(), st)); launches++; }
  void resolve() {
    for (size_t i = 0; i + 1 < used; i += 2) {
      float t = 0; HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      ms += t;
    }
    used = 0;
  }
};
// The stopwatches of a render: the megakernel; the extend, shade (every streaming pass of the wavefront pipelines) and connect
// stages; the estimator; and inside those stages the lean closest-hit kernel, the shade kernel and the lean any-hit kernel alone.
struct StageTimers {
  StageTimer mega, extend, shade, connect, gmon, lean, shadeK, shadowLean;
  void resolveAll() { for (StageTimer* t : {&mega, &extend, &shade, &connect, &gmon, &lean, &shadeK, &shadowLean}) t->resolve(); }
};

// Called after every batch of a wave, once its pixels are final for that wave in the output frame (the stream has been
// synchronised): the range [c0, c0 + n) of this rank's pixel list. Returning true stops the render after this batch.
struct BatchInfo { uint32_t c0, n, wave, waveSamples, samplesTaken, totalSamples; };
typedef std::function<bool(const BatchInfo&)> BatchHook;

// Everything a render decides before its first wave (makeRenderPlan); the buffers are allocated from it (prepareBuffers) and the
// batch runners launch from it.
// aov: feature buffers to fill as well (device pointers, checked by checkAovs; nullptr: none — nothing differs from a plain render then)
// mom: sample moments to fill as well (device pointers, checked by checkMoments; nullptr: none, and nothing differs either)
struct RenderPlan {
  const YartRenderParams* p;
  const YartAovBuffers* aov;
  const YartMomentBuffers* mom;
  uint32_t W, H, nPix;
  CameraDev cam;
  RenderConst rc, rcw;                       // rcw: rc with the sampler tables of this render (launchSamplerTables), for the wavefront kernels
  uint32_t effFlags;                         // after the defaults (reported in YartStats::pipeline_flags)
  bool mega, pool, compact, general, refill, samplerTables;
  int nodesForm;
  uint32_t nodeBitWords;
  void (*kMega)(MegaArgs);
  WfKernelFn kExtendFast, kShadowFast, kRetryE, kRetryS, kExtendGen, kExtendGenRetry, kShadowGen, kShadowGenRetry, kShade;
  int gridMega, gridExtendFast, gridShadowFast, gridExtend, gridShadow, gridShade, gridRetryE, gridRetryS, gridMax;
  uint32_t chunk, waveCap;                   // pixels per batch; the largest wave of the schedule
  size_t aovStride;                          // paths of the largest batch: L, and each feature record array of the megakernel / path pool
  size_t slots;                              // wavefront pipelines: path slots (the batch's paths, or the pool's slots)
  uint32_t poolSlots, resumeCap;
};

// Batch = the pixels (x all samples of a wave) rendered together: max_batch_paths, by default kDefaultBatchPaths — a fixed
// number, no longer a share of the free device memory (round 3 sized ONE batch to 60 % of it: 150 GB for the C3 frame); only if
// that does not fit the device is it cut down to what does. The default pipeline is batch-synchronous: one slot per path of the
// batch (251 bytes with the compacted tail state), every bounce one launch per stage over the paths still alive. What a smaller
// batch costs (profiles/r4_ab_path_pool.txt): ~10 ms per batch of any size — the tail of every launch, when the GPU waits for
// the slowest rays of the last waves — so the C3 frame in 2 / 4 / 8 / 16 batches is 1.4 / 4.5 / 9.7 / 19 % slower than in one.
// YART_FLAG_PATH_POOL: the batch runs through a POOL of pool_paths slots with path regeneration instead (168 bytes per slot +
// 16 per path of the batch): bounded memory at any frame size, every launch pool-sized until the batch runs out — and ~25 %
// slower on the C3 frame, because a wave's lanes then hold paths of every generation (same file).
// Returns the paths a batch may hold and — path pool — the slots the device can hold next to the batch's radiance records.
// Reads the plan's switches, grids and waveCap; the traversal scratch has been allocated (the free memory is looked at here).
struct BatchBudget { uint64_t maxPaths, poolFit; };
BatchBudget batchBudget(const YartScene& s, const RenderPlan& pl) {
  const YartRenderParams& p = *pl.p;
  const uint32_t nPix = pl.nPix;
  uint64_t maxPaths = p.max_batch_paths ? p.max_batch_paths : kDefaultBatchPaths;
  uint64_t poolFit = ~0ull;                     // path pool: the slots the device can hold next to the batch's radiance records
  if (!pl.mega) {
    // (safety only: a device that cannot hold the batch renders smaller ones)
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    if (const char* e = std::getenv("YART_FAKE_FREE_MB")) freeB = size_t(std::max<long long>(1, std::atoll(e))) << 20;   // (tests of the clamp)
    uint64_t held = uint64_t(s.L.n) * 16 + (uint64_t(s.qA.n) + s.qB.n + s.qS.n + s.qR.n) * 4 + uint64_t(s.resumeRec.n) * 16;
    for (auto& b : s.wf) held += uint64_t(b.n) * 16;
    for (auto& t : s.wfTail) for (auto& b : t) held += uint64_t(b.n) * 16;
    held += (uint64_t(s.wfTailMap[0].n) + s.wfTailMap[1].n) * 4;
    held += uint64_t(s.smpEntries.n) * 8;      // the sampler tables of the previous render stay allocated
    held += uint64_t(s.aovRec.n) * 16;
    if (std::getenv("YART_FAKE_FREE_MB")) held = 0;
    // what grows with the batch: 9 x 16 B of path state + 4 queue words + 16 B of radiance = 176 B per path; with compaction two
    // a tail state of 1/2 of the batch (9 x 16 B + a slot map word) and a slot map of 1/4 = 75 B more; the resume records of an eighth of
    // the paths (kResumeWords x 16 B each = 24 B per path). What does not: the sampler tables (8 B x dims per PIXEL of the rank),
    // the resume records' per-wave ranges and the traversal spill area — taken off the budget first.
    const uint64_t perPath = (pl.compact ? 251 : 176) + ((p.flags & YART_FLAG_NO_RESUME) ? 0 : (kResumeWords * 16 + 7) / 8);
    const uint64_t dimsEst = std::min<uint32_t>(256u, (4u + 8u * p.max_depth + 16u + 7u) & ~7u);
    const uint64_t fixedB = uint64_t(nPix) * dimsEst * 8 + uint64_t(pl.gridMax) * kBlock * (kResumeWords * 16 + uint64_t(spillDepthFor(s.host, true)) * 8) +
                            (pl.mom ? uint64_t(nPix) * sizeof(MomentState) : 0u);      // (sample moments: 48 B per pixel of the rank)
    const uint64_t budget = (uint64_t(freeB) + held) * 8 / 10;
    const uint64_t avail = budget > fixedB ? budget - fixedB : 0;
    if (!pl.pool) {
      const uint64_t fits = std::max<uint64_t>(avail / perPath, 1u << 16);
      maxPaths = std::min<uint64_t>(std::min<uint64_t>(maxPaths, fits), kWfMaxPaths);
    } else {
      // pool: 16 B of radiance per path of the batch + 168 B (+ resume records) per slot of the pool: the batch gets at most half
      // of the budget, the pool what is left
      // (feature buffers: + 48 B of feature record per path of the batch; the default pipeline keeps its records in the shadow-ray arrays)
      const uint64_t perBatchPath = pl.aov ? 16 + 48 : 16;
      const uint64_t fits = std::max<uint64_t>(avail / 2 / perBatchPath, 1u << 16);
      maxPaths = std::min<uint64_t>(maxPaths, fits);
      const uint64_t left = avail > std::min<uint64_t>(maxPaths, uint64_t(nPix ? nPix : 1) * pl.waveCap) * perBatchPath ? avail - std::min<uint64_t>(maxPaths, uint64_t(nPix ? nPix : 1) * pl.waveCap) * perBatchPath : 0;
      poolFit = std::max<uint64_t>(left / (176 + (kResumeWords * 16 + 7) / 8), 64);
    }
  }
  return {std::min<uint64_t>(maxPaths, (1ull << 31) - 64), poolFit};
}

// The pixel list of the rank is built (buildPixelList). Allocates the traversal scratch the chosen grids need — spill area and
// node bitsets, before the batch budget looks at the free memory — and nothing else.
RenderPlan makeRenderPlan(YartScene& s, const YartCameraDesc& camDesc, const YartRenderParams& p, const YartAovBuffers* aov,
                          const YartMomentBuffers* mom, hipStream_t stream) {
  RenderPlan pl{};
  pl.p = &p; pl.aov = aov; pl.mom = mom;
  pl.W = camDesc.width; pl.H = camDesc.height; pl.nPix = uint32_t(s.pixelsHost.size());
  pl.cam = makeCamera(camDesc);
  pl.rc = pl.rcw = makeRenderConst(p);
  pl.mega = (p.flags & YART_FLAG_MEGAKERNEL) != 0;
  pl.effFlags = p.flags;
  if (!pl.mega && !(pl.effFlags & YART_FLAG_NO_SHADE_SORT)) pl.effFlags |= YART_FLAG_SHADE_SORT;

  // lean traversal kernels when the scene allows them (every node transform chain the identity ->
  // identity-only variant); YART_FLAG_GENERAL_TRACE forces the general kernels for everything
  pl.general = (p.flags & YART_FLAG_GENERAL_TRACE) != 0;
  const bool ident = s.host.allIdentity;
  pl.refill = (p.flags & YART_FLAG_NO_REFILL) == 0;
  // the kNodesMask form of trace_lean.hpp keeps one 64-bit node candidate mask per ray and uses the all-ones mask as its "new ray"
  // marker, which a ray that can reach all of exactly 64 nodes would keep: 64 nodes and more go to the windowed forms
  const bool chunked = s.host.nodes.size() >= 64;
  // 64 nodes and more: candidate windows from the top-level hierarchy (kNodesTlas; measured the fastest form at every size from 65 to 4252
  // nodes, profiles/r2_many_nodes.txt). Without it (no mesh nodes, more than 16384 nodes = 2 KB of bitset per lane, or debug bit
  // 262144): chunked masks (kNodesChunked) below kLeanWalkNodes nodes, the per-lane walk (kNodesWalk) from there on (debug bit 65536: the walk at any size)
  const bool tlasOk = s.dev.nTlas != 0u && s.host.nodes.size() <= 16384u && !(pl.effFlags & (262144u | 65536u));
  const bool leanLds = !chunked && s.host.nodes.size() <= kLeanSceneNodes && s.host.meshes.size() <= kLeanSceneNodes;
  pl.nodesForm = !chunked ? (leanLds ? kNodesMaskLds : kNodesMask) : tlasOk ? kNodesTlas
               : ((pl.effFlags & 65536u) || s.host.nodes.size() >= kLeanWalkNodes) ? kNodesWalk : kNodesChunked;
  pl.kExtendFast = wfKernel(pl.refill ? tu::extendLean(pl.nodesForm, ident) : tu::extendFast(ident));
  pl.kShadowFast = wfKernel(pl.refill ? tu::shadowLean(pl.nodesForm, ident) : tu::shadowFast(ident));
  pl.kRetryE = wfKernel(tu::extendRetry(pl.nodesForm));
  pl.kRetryS = wfKernel(tu::shadowRetry(pl.nodesForm));
  pl.kExtendGen = wfKernel(tu::extendGeneral(false)); pl.kExtendGenRetry = wfKernel(tu::extendGeneral(true));
  pl.kShadowGen = wfKernel(tu::shadowGeneral(false)); pl.kShadowGenRetry = wfKernel(tu::shadowGeneral(true));
  pl.kMega = aov ? k_render_mega<true> : k_render_mega<false>;
  pl.gridMega = persistentGrid(s, reinterpret_cast<const void*>(pl.kMega), 3);
  pl.gridExtendFast = persistentGrid(s, reinterpret_cast<const void*>(pl.kExtendFast), 8);
  pl.gridShadowFast = persistentGrid(s, reinterpret_cast<const void*>(pl.kShadowFast), 8);
  pl.gridExtend = persistentGrid(s, reinterpret_cast<const void*>(pl.kExtendGen), 8);
  pl.gridShadow = persistentGrid(s, reinterpret_cast<const void*>(pl.kShadowGen), 8);
  // the shade kernel's LDS copies of the scene's small tables: FIT when the sampler tables are in use and every table fits its slot
  // sampler tables (sampler.hpp::SamplerTables) for the wavefront pipeline; they require every
  // sample index to fit the sampler's log2spp bits (log2Int rounds to nearest, e.g. 90 spp -> 6)
  pl.samplerTables = !pl.mega && !(p.flags & YART_FLAG_DIRECT_SAMPLER) && pl.nPix > 0 && uint64_t(p.samples) <= (1ull << pl.rc.sampler.log2spp);
  const bool shadeFit = pl.samplerTables && s.dev.nMaterials <= kShadeMatSlots && s.dev.nTextures <= kShadeTexSlots && s.dev.nLights <= kShadeLightSlots &&
                        s.dev.nEnvs <= kShadeEnvSlots && s.dev.nNodes <= kShadeNodeSlots && s.dev.nInfinite <= kShadeLightSlots;
  const bool envOnly = shadeFit && s.dev.nArea == 0u && s.dev.nInfinite == 1u && s.dev.nLights == 1u;    // (variant of the FIT kernels only)
  pl.kShade = wfKernel(tu::shade((pl.effFlags & YART_FLAG_SHADE_SORT) != 0, shadeFit, envOnly));
  pl.gridShade = persistentGrid(s, reinterpret_cast<const void*>(pl.kShade), 8, kShadeBlock);
  pl.gridRetryE = persistentGrid(s, reinterpret_cast<const void*>(pl.kRetryE), 8);
  pl.gridRetryS = persistentGrid(s, reinterpret_cast<const void*>(pl.kRetryS), 8);
  pl.gridMax = std::max(pl.gridMega, std::max(pl.gridExtend, pl.gridShadow));
  pl.gridMax = std::max(pl.gridMax, std::max(pl.gridExtendFast, pl.gridShadowFast));
  pl.gridMax = std::max(pl.gridMax, std::max(pl.gridRetryE, pl.gridRetryS));
  s.spill.ensure(size_t(pl.gridMax) * kBlock * spillDepthFor(s.host, true));
  // the lanes' node bitsets of the top-level-hierarchy form (kNodesTlas, trace_lean.hpp): all zero between launches
  pl.nodeBitWords = pl.nodesForm == kNodesTlas ? uint32_t((s.host.nodes.size() + 63u) / 64u) : 0u;
  if (pl.nodeBitWords) {
    const size_t need = size_t(pl.gridMax) * kBlock * pl.nodeBitWords;
    if (s.nodeBits.n < need) { s.nodeBits.ensure(need); HIP_CHECK(hipMemsetAsync(s.nodeBits.p, 0, need * 8, stream)); }
  }

  const uint32_t maxWave = std::min(p.max_wave_samples, p.samples);
  pl.waveCap = std::max(std::min(p.first_wave_samples, p.samples), maxWave);
  pl.pool = !pl.mega && (p.flags & YART_FLAG_PATH_POOL) != 0;
  pl.compact = !pl.mega && !pl.pool && !(p.flags & YART_FLAG_NO_COMPACTION);
  const BatchBudget fit = batchBudget(s, pl);
  pl.chunk = uint32_t(std::min<uint64_t>(pl.nPix ? pl.nPix : 1, std::max<uint64_t>(fit.maxPaths / pl.waveCap, 1)));
  if (pl.nPix > pl.chunk) {                      // batches of equal size (the last one is not a sliver)
    const uint32_t nb = (pl.nPix + pl.chunk - 1) / pl.chunk;
    pl.chunk = (pl.nPix + nb - 1) / nb;
  }
  pl.aovStride = size_t(pl.chunk) * pl.waveCap;
  if (!pl.mega) {
    pl.slots = pl.aovStride;
    if (pl.pool) {
      const size_t want = std::min<uint64_t>(p.pool_paths ? p.pool_paths : kDefaultPoolPaths, fit.poolFit);
      pl.slots = std::max<size_t>(64, (std::min(want, pl.aovStride) + 63) & ~size_t(63));
      pl.poolSlots = uint32_t(pl.slots);
    }
    // resume records of the rays the lean kernels hand to the general ones (traverse.hpp: 192 B each): room for an eighth of
    // the slots (C3 hands over 6-7 % of its rays; a ray that finds no record is restarted, as all of them were before).
    // YART_RESUME_CAP: records (tests of the fallback), 0 = restarts only.
    if (!(p.flags & YART_FLAG_NO_RESUME)) {
      // (+ one range of 64 per wave of the largest grid: a wave takes its records 64 at a time and may leave a range unfinished)
      size_t cap = std::max<size_t>(pl.slots / 8, std::min<size_t>(pl.slots, 1u << 16)) + size_t(pl.gridMax) * kBlock;
      if (const char* e = std::getenv("YART_RESUME_CAP")) cap = size_t(std::max<long long>(0, std::atoll(e)));
      pl.resumeCap = uint32_t(std::min<size_t>(cap, 0x7fffff00u));
    }
  }
  return pl;
}

// The scene's buffers a render of this plan needs, grown on demand; the per-pixel accumulators and the caller's feature and moment
// buffers cleared as the frame is.
void prepareBuffers(YartScene& s, const RenderPlan& pl, hipStream_t stream) {
  const size_t np1 = std::max<uint32_t>(pl.nPix, 1u), wh = size_t(pl.W) * pl.H;
  const auto clear = [&](void* ptr, int byte, size_t bytes) { HIP_CHECK(hipMemsetAsync(ptr, byte, bytes, stream)); };
  s.L.ensure(pl.aovStride);
  // feature buffers: per-pixel accumulators (zero; ids -1), the caller's buffers, and — megakernel / path pool — the record arrays of the batch
  if (pl.aov) {
    for (auto& b : s.aovAcc) { b.ensure(np1); clear(b.p, 0, np1 * sizeof(f4)); }
    s.aovRays.ensure(np1); clear(s.aovRays.p, 0, np1 * sizeof(uint32_t));
    s.aovIds.ensure(np1 * 4); clear(s.aovIds.p, 0xff, np1 * 4 * sizeof(int32_t));
    s.pixRays.ensure(np1);
    if (pl.mega || pl.pool) s.aovRec.ensure(3 * pl.aovStride);
    clearBuffers(kAovTable, *pl.aov, wh, clear);
  }
  // sample moments: the running state per pixel of the rank (zero), the caller's buffers
  if (pl.mom) {
    s.momState.ensure(np1); clear(s.momState.p, 0, np1 * sizeof(MomentState));
    clearBuffers(kMomentTable, *pl.mom, wh, clear);
  }
  if (pl.mega) return;
  if (pl.pool) {
    s.poolMap.ensure(pl.slots);
    if (!s.poolHost) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.poolHost), kPoolLag * WC_COUNT * sizeof(uint32_t)));
  }
  for (auto& b : s.wf) b.ensure(pl.slots);
  if (pl.compact) {
    // Two dense "tail" states take the survivors in turn: the first is an array set of half the batch; the second is the BATCH-SIZED
    // state itself — by the time a second compaction happens the paths live in the first tail and the large arrays hold nothing
    // that is still read, so the survivors go back to their front (round 5: 36 B per path less than a third array set).
    for (auto& b : s.wfTail[0]) b.ensure(pl.slots / 2 + 64);
    s.wfTailMap[0].ensure(pl.slots / 2 + 64);
    s.wfTailMap[1].ensure(pl.slots / 4 + 64);
    s.wfDyn.ensure(1);
  }
  s.qA.ensure(pl.slots); s.qB.ensure(pl.slots); s.qS.ensure(pl.slots); s.qR.ensure(pl.slots); s.wfCounters.ensure(WC_COUNT);
  if (pl.resumeCap) s.resumeRec.ensure(size_t(pl.resumeCap) * kResumeWords);
}

// The sampler tables of this render, for the wavefront kernels (pl.rcw carries them from here on)
void launchSamplerTables(YartScene& s, RenderPlan& pl, StageTimers& t, hipStream_t stream) {
  if (!pl.samplerTables) return;
  const uint32_t dims = std::min<uint32_t>(256u, (4u + 8u * pl.p->max_depth + 16u + 7u) & ~7u);     // (+ 3 <= kShadeHashSlots)
  s.smpEntries.ensure(size_t(dims) * pl.nPix); s.smpHash.ensure(dims + 3); s.smpSobol1.ensure(8 * 256);
  SamplerTabArgs ta{};
  ta.cfg = pl.rc.sampler; ta.pixels = s.pixels.p; ta.nPixels = pl.nPix; ta.dims = dims;
  ta.entries = s.smpEntries.p; ta.hash = s.smpHash.p; ta.sobol1 = s.smpSobol1.p;
  ta.matrix52 = reinterpret_cast<const uint32_t*>(s.dev.lut + LutDev::sobol);
  TraceRange rg("yart:sampler_tables", stream);
  t.shade.begin(stream);
  hipLaunchKernelGGL(k_sampler_tables, dim3(s.numCUs * 8), dim3(kBlock), 0, stream, ta);
  HIP_CHECK(hipGetLastError());
  t.shade.end(stream);
  pl.rcw.sampler.tab.entries = s.smpEntries.p; pl.rcw.sampler.tab.hash = s.smpHash.p; pl.rcw.sampler.tab.sobol1 = s.smpSobol1.p;
  pl.rcw.sampler.tab.dims = dims; pl.rcw.sampler.tab.stride = pl.nPix;
}

// One batch of one wave: pixels [c0, c0 + n) of the rank's list, samples [takenBefore, takenBefore + waveSamples) of each
struct Batch { uint32_t c0, n, waveSamples, takenBefore; };

// feature buffers: the arguments of the batch's capture / reduce kernels (all zero without feature buffers)
AovArgs aovArgs(const YartScene& s, const RenderPlan& pl, const Batch& b) {
  AovArgs av{};
  if (pl.aov) {
    av.acc0 = s.aovAcc[0].p; av.acc1 = s.aovAcc[1].p; av.acc2 = s.aovAcc[2].p; av.accRays = s.aovRays.p; av.ids = s.aovIds.p;
    av.nPixels = b.n; av.spp = b.waveSamples; av.pixBase = b.c0; av.sampleOffset = b.takenBefore;
    if (pl.mega || pl.pool) { av.r0 = s.aovRec.p; av.r1 = s.aovRec.p + pl.aovStride; av.r2 = s.aovRec.p + 2 * pl.aovStride; }
  }
  return av;
}
void aovReduce(const AovArgs& av, hipStream_t stream) {
  TraceRange rgA("yart:aov_reduce", stream);
  hipLaunchKernelGGL(k_aov_reduce, dim3((av.nPixels * 4u + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, av);
  HIP_CHECK(hipGetLastError());
}

void runMegaBatch(YartScene& s, const RenderPlan& pl, const Batch& b, StageTimers& t, hipStream_t stream) {
  const AovArgs av = aovArgs(s, pl, b);
  HIP_CHECK(hipMemsetAsync(s.cursor.p, 0, sizeof(uint32_t), stream));
  MegaArgs a{};
  a.sc = s.dev; a.cam = pl.cam; a.rc = pl.rc; a.pixels = s.pixels.p + b.c0; a.nPixels = b.n;
  a.spp = b.waveSamples; a.sampleOffset = b.takenBefore; a.L = s.L.p;
  a.cursor = s.cursor.p; a.rays = s.counters.p; a.spill = s.spill.p;
  a.aov0 = av.r0; a.aov1 = av.r1; a.aov2 = av.r2; a.aovIds = av.ids; a.pixBase = b.c0;
  TraceRange rgMega("yart:megakernel", stream);
  t.mega.begin(stream);
  hipLaunchKernelGGL(pl.kMega, dim3(pl.gridMega), dim3(kBlock), 0, stream, a);
  HIP_CHECK(hipGetLastError());
  t.mega.end(stream);
  if (pl.aov) aovReduce(av, stream);
}

// what the path pool and the batch-synchronous pipeline pass to every kernel of a batch
WfArgs wfArgs(const YartScene& s, const RenderPlan& pl, const Batch& b) {
  WfArgs a{};
  a.sc = s.dev; a.cam = pl.cam; a.rc = pl.rcw; a.pixBase = b.c0;
  a.st.ray0 = s.wf[0].p; a.st.ray1 = s.wf[1].p; a.st.thr = s.wf[2].p; a.st.acc = s.wf[3].p;
  a.st.hit0 = s.wf[4].p; a.st.hit1 = s.wf[5].p; a.st.sh0 = s.wf[6].p; a.st.sh1 = s.wf[7].p; a.st.sh2 = s.wf[8].p;
  a.qA = s.qA.p; a.qB = s.qB.p; a.qS = s.qS.p; a.qR = s.qR.p; a.counters = s.wfCounters.p;
  a.pixels = s.pixels.p + b.c0; a.nPaths = b.n * b.waveSamples; a.spp = b.waveSamples;
  a.sampleOffset = b.takenBefore; a.L = s.L.p; a.stats = s.counters.p; a.spill = s.spill.p;
  a.matClass = s.matClass.p;
  a.resumeRec = pl.resumeCap ? s.resumeRec.p : nullptr; a.resumeCap = pl.resumeCap;
  a.sc.nodeBits = s.nodeBits.p; a.sc.nodeBitWords = pl.nodeBitWords;
  return a;
}

// The extend stage over the queue of `a`: the general kernel, or the lean kernel and then the retry pass over the rays it handed
// over (the lean retry kernel, or — one-ray-per-lane lean kernels — the general one)
void extendStage(const RenderPlan& pl, const WfArgs& a, StageTimers& t, hipStream_t stream) {
  t.extend.begin(stream);
  if (pl.general) {
    hipLaunchKernelGGL(pl.kExtendGen, dim3(pl.gridExtend), dim3(kBlock), 0, stream, a);
  } else {
    t.lean.begin(stream);
    hipLaunchKernelGGL(pl.kExtendFast, dim3(pl.gridExtendFast), dim3(kBlock), 0, stream, a);
    t.lean.end(stream);
    if (pl.refill) hipLaunchKernelGGL(pl.kRetryE, dim3(pl.gridRetryE), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(pl.kExtendGenRetry, dim3(pl.gridExtend), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(k_wf_reset_retry, dim3(1), dim3(64), 0, stream, a.counters);
  }
  HIP_CHECK(hipGetLastError());
  t.extend.end(stream);
}
// The shadow stage, likewise
void shadowStage(const RenderPlan& pl, const WfArgs& a, StageTimers& t, hipStream_t stream) {
  t.connect.begin(stream);
  if (pl.general) {
    hipLaunchKernelGGL(pl.kShadowGen, dim3(pl.gridShadow), dim3(kBlock), 0, stream, a);
  } else {
    t.shadowLean.begin(stream);
    hipLaunchKernelGGL(pl.kShadowFast, dim3(pl.gridShadowFast), dim3(kBlock), 0, stream, a);
    t.shadowLean.end(stream);
    if (pl.refill) hipLaunchKernelGGL(pl.kRetryS, dim3(pl.gridRetryS), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(pl.kShadowGenRetry, dim3(pl.gridShadow), dim3(kBlock), 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
  t.connect.end(stream);
}
void shadeStage(const RenderPlan& pl, const WfArgs& a, StageTimers& t, hipStream_t stream) {
  t.shade.begin(stream);
  t.shadeK.begin(stream);
  hipLaunchKernelGGL(pl.kShade, dim3(pl.gridShade), dim3(kShadeBlock), 0, stream, a);
  HIP_CHECK(hipGetLastError());
  t.shadeK.end(stream);
  t.shade.end(stream);
}
// a streaming pass of the wavefront pipelines (generate, refill, roulette, compact), on the shade stopwatch
void streamingPass(const YartScene& s, WfKernelFn k, const WfArgs& a, StageTimers& t, hipStream_t stream) {
  t.shade.begin(stream);
  hipLaunchKernelGGL(k, dim3(s.numCUs * YART_STREAM_BLOCKS), dim3(kBlock), 0, stream, a);
  HIP_CHECK(hipGetLastError());
  t.shade.end(stream);
}

void runPoolBatch(YartScene& s, const RenderPlan& pl, const Batch& b, StageTimers& t, hipStream_t stream) {
  const AovArgs av = aovArgs(s, pl, b);
  WfArgs a = wfArgs(s, pl, b);
  a.slotMap = s.poolMap.p;
  a.poolSlots = uint32_t(std::min<uint64_t>(pl.poolSlots, (uint64_t(a.nPaths) + 63u) & ~uint64_t(63)));
  const uint32_t init[WC_COUNT] = {a.poolSlots, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(s.wfCounters.p, init, sizeof(init), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_wf_pool_init, dim3(s.numCUs * 4), dim3(kBlock), 0, stream, s.poolMap.p, a.poolSlots);
  HIP_CHECK(hipGetLastError());
  // Rounds: every round starts new paths in the free slots and takes every live path one bounce further. The host does not
  // know when the batch is done; it reads the counters of the round before the previous one (a copy into pinned memory and
  // an event per round, never waited for) and stops launching when that round left no live path and nothing to start:
  // two or three empty rounds at the end instead of a host synchronisation per round.
  struct RoundEvents {                      // (destroyed on every way out of the round loop, a thrown HipError included)
    hipEvent_t ev[kPoolLag] = {};
    ~RoundEvents() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
  } roundEv;
  hipEvent_t* evRound = roundEv.ev;
  for (int k = 0; k < kPoolLag; k++) HIP_CHECK(hipEventCreateWithFlags(&evRound[k], hipEventDisableTiming));
  const uint64_t maxRounds = (uint64_t(a.nPaths) / a.poolSlots + 2u) * (pl.rc.maxDepth + 1u) + 16u;   // (a path lives at most maxDepth rounds)
  bool done = false;
  for (uint64_t round = 0; !done; round++) {
    if (round > maxRounds) throw HipError("path pool: the batch did not finish within its bound of rounds");
    streamingPass(s, k_wf_refill, a, t, stream);
    {   // the live slots of this round, for the host (WC_NEXT: k_wf_refill)
      uint32_t* snap = s.poolHost + size_t(round % kPoolLag) * WC_COUNT;
      HIP_CHECK(hipMemcpyAsync(snap, s.wfCounters.p, WC_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipEventRecord(evRound[round % kPoolLag], stream));
    }
    extendStage(pl, a, t, stream);
    if (pl.aov) {                             // the paths this round's refill started stand at bounce 0 with their hit records final
      hipLaunchKernelGGL(k_aov_capture, dim3(s.numCUs * YART_STREAM_BLOCKS), dim3(kBlock), 0, stream, a, av);
      HIP_CHECK(hipGetLastError());
    }
    shadeStage(pl, a, t, stream);
    shadowStage(pl, a, t, stream);
    streamingPass(s, k_wf_roulette, a, t, stream);
    hipLaunchKernelGGL(k_wf_pool_advance, dim3(1), dim3(64), 0, stream, s.wfCounters.p, a.poolSlots);
    HIP_CHECK(hipGetLastError());
    if (round >= 2) {
      const uint64_t old = round - 2;
      // (rounds far ahead of the device would only queue launches: wait for the round before the previous one)
      HIP_CHECK(hipEventSynchronize(evRound[old % kPoolLag]));
      const uint32_t* c = s.poolHost + size_t(old % kPoolLag) * WC_COUNT;
      if (c[WC_NEXT] == 0u) done = true;                  // no live slot after its refill: nothing left to start either
    }
  }
  if (pl.aov) aovReduce(av, stream);
}

void runWavefrontBatch(YartScene& s, const RenderPlan& pl, const Batch& b, StageTimers& t, hipStream_t stream) {
  AovArgs av = aovArgs(s, pl, b);
  WfArgs a = wfArgs(s, pl, b);
  const uint32_t maxDepth = pl.rc.maxDepth;
  if (pl.compact) {
    for (int k = 0; k < 2; k++) {
      f4** f = &a.tail[k].ray0;                  // the nine pointers of WfState, in declaration order
      for (int j = 0; j < 9; j++) f[j] = k == 0 ? s.wfTail[0][j].p : s.wf[j].p;      // (second tail: the batch-sized state, see prepareBuffers)
      a.tailMap[k] = s.wfTailMap[k].p;
      a.tailCap[k] = a.nPaths / (k == 0 ? 2u : 4u);
    }
    WfDyn d0{};
    d0.st = a.st; d0.slotMap = nullptr; d0.extent = a.nPaths; d0.inTail = 0;
    HIP_CHECK(hipMemcpyAsync(s.wfDyn.p, &d0, sizeof(d0), hipMemcpyHostToDevice, stream));
    a.dyn = s.wfDyn.p;
  }
  const uint32_t init[WC_COUNT] = {a.nPaths, 0, 0, 0, 0, 0, 0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(s.wfCounters.p, init, sizeof(init), hipMemcpyHostToDevice, stream));
  {
    TraceRange rgGen("yart:generate", stream);
    streamingPass(s, k_wf_generate, a, t, stream);
  }
  for (uint32_t bounce = 0; bounce < maxDepth; bounce++) {
    a.bounce = bounce;
    char rgName[32]; std::snprintf(rgName, sizeof(rgName), "yart:bounce %u", bounce);
    TraceRange rgBounce(rgName);
    {
      TraceRange rgExtend("yart:extend", stream);
      extendStage(pl, a, t, stream);
    }
    if (pl.aov && bounce == 0) {
      // feature records of every path of the batch, written into the shadow-ray arrays (unused until the shade stage below
      // writes bounce 0's shadow rays) and summed per pixel at once, before that happens
      {
        TraceRange rgA("yart:aov_capture", stream);
        av.r0 = a.st.sh0; av.r1 = a.st.sh1; av.r2 = a.st.sh2;
        hipLaunchKernelGGL(k_aov_capture, dim3(s.numCUs * YART_STREAM_BLOCKS), dim3(kBlock), 0, stream, a, av);
        HIP_CHECK(hipGetLastError());
      }
      aovReduce(av, stream);
    }
    {
      TraceRange rgShade("yart:shade", stream);
      shadeStage(pl, a, t, stream);
    }
    {
      TraceRange rgShadow("yart:shadow", stream);
      shadowStage(pl, a, t, stream);
    }
    // Russian roulette thins the paths from the second bounce on (at depth 1 none applies), not after the last one (every
    // path is written out then). It is no stage: k_wf_shade decides, the general shadow kernels repair what an alpha test's
    // draw reverses (wavefront.hpp: wfRouletteTentative, wfShadowCommitGeneral). The range stays, empty, where the pass
    // ran until then: tools that read the trace by name find the bounce's layout unchanged.
    const bool thinning = bounce >= 1 && bounce + 1 < maxDepth;
    if (thinning) { TraceRange rgR("yart:roulette"); }
    hipLaunchKernelGGL(k_wf_advance, dim3(1), dim3(64), 0, stream, s.wfCounters.p, bounce + 1 < 16u ? s.pathsLog.p + bounce + 1 : nullptr);
    HIP_CHECK(hipGetLastError());
    std::swap(a.qA, a.qB);
    if (pl.compact && thinning) {               // Russian roulette starts thinning at depth 2
      TraceRange rgC("yart:compact", stream);
      t.shade.begin(stream);
      hipLaunchKernelGGL(k_wf_compact, dim3(s.numCUs * YART_STREAM_BLOCKS), dim3(kBlock), 0, stream, a);
      hipLaunchKernelGGL(k_wf_compact_commit, dim3(1), dim3(64), 0, stream, a);
      HIP_CHECK(hipGetLastError());
      t.shade.end(stream);
    }
  }
}

// What follows every batch's runner: the batch's samples through the estimator and blended into the frame (weights wCurrent /
// wWave of the wave), the moments and ray counts summed, the stream synchronised and the stopwatches resolved; then — tile
// callbacks — the ray counts of the blocks the batch completed and the hook. true: the hook asked to stop.
struct WaveInfo { uint32_t wave, samplesTaken; float wCurrent, wWave; size_t tileDone; };   // tileDone: blocks of this wave whose ray counts have been summed
bool finishBatch(YartScene& s, const RenderPlan& pl, const Batch& b, WaveInfo& w, float* dOut, StageTimers& t, const BatchHook* hook,
                 hipStream_t stream) {
  const uint32_t c0 = b.c0, n = b.n;
  const bool hooked = hook && *hook;
  GmonArgs g{};
  if (hooked) { s.pixRays.ensure(std::max<uint32_t>(pl.nPix, 1u)); g.pixRays = s.pixRays.p + c0; }
  if (pl.aov) g.pixRays = s.pixRays.p + c0;
  g.L = s.L.p; g.pixels = s.pixels.p + c0; g.nPixels = n; g.spp = b.waveSamples; g.width = pl.W;
  g.exposureScale = pl.cam.exposureScale; g.wCurrent = w.wCurrent; g.wWave = w.wWave; g.hdr = dOut;
  g.kind = int(pl.p->estimator);
  {
    TraceRange rgBlend("yart:gmon_blend", stream);
    t.gmon.begin(stream);
    hipLaunchKernelGGL(k_gmon_blend, dim3((n + kGmonPixPerBlock - 1) / kGmonPixPerBlock), dim3(kBlock), 0, stream, g);
    HIP_CHECK(hipGetLastError());
    t.gmon.end(stream);
    if (pl.mom) {                            // the same records, before the next batch overwrites them
      MomentArgs ma{};
      ma.L = s.L.p; ma.state = s.momState.p; ma.nPixels = n; ma.spp = b.waveSamples; ma.pixBase = c0;
      ma.exposureScale = pl.cam.exposureScale;
      TraceRange rgM("yart:moments_accumulate", stream);
      hipLaunchKernelGGL(k_moments_accumulate, dim3((n + kMomentPixPerBlock - 1) / kMomentPixPerBlock), dim3(kBlock), 0, stream, ma);
      HIP_CHECK(hipGetLastError());
    }
    if (pl.aov) {
      hipLaunchKernelGGL(k_aov_add_rays, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, s.aovRays.p + c0, s.pixRays.p + c0, n);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  t.resolveAll();
  if (!hooked) return false;
  // ray counts of the blocks this batch completed (their pixels' counts of this wave are all in pixRays now)
  size_t done = w.tileDone;
  while (done < s.tiles.size() && s.tiles[done].start + s.tiles[done].count <= c0 + n) done++;
  if (done > w.tileDone) {
    s.tileRays.ensure(s.tiles.size()); s.tileRaysHost.resize(s.tiles.size());
    hipLaunchKernelGGL(k_tile_rays, dim3(uint32_t(done - w.tileDone)), dim3(64), 0, stream, s.pixRays.p, s.tileStart.p, s.tileCount.p,
                       uint32_t(w.tileDone), uint32_t(done - w.tileDone), s.tileRays.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(s.tileRaysHost.data() + w.tileDone, s.tileRays.p + w.tileDone, (done - w.tileDone) * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    w.tileDone = done;
  }
  return (*hook)(BatchInfo{c0, n, w.wave, b.waveSamples, w.samplesTaken, pl.p->samples});
}

// After the last wave: the accumulators of the feature buffers and the moments written to the caller's buffers
void launchFinishKernels(const YartScene& s, const RenderPlan& pl, hipStream_t stream) {
  if (pl.nPix == 0) return;
  if (pl.aov) {
    const YartAovBuffers* aov = pl.aov;
    AovFinishArgs f{};
    f.acc0 = s.aovAcc[0].p; f.acc1 = s.aovAcc[1].p; f.acc2 = s.aovAcc[2].p; f.accRays = s.aovRays.p; f.ids = s.aovIds.p;
    f.pixels = s.pixels.p; f.nPixels = pl.nPix; f.width = pl.W; f.samples = pl.p->samples; f.mask = aov->mask;
    f.albedo = aov->albedo; f.normal = aov->normal; f.position = aov->position; f.depth = aov->depth; f.coverage = aov->coverage;
    f.outIds = aov->ids; f.outRays = aov->rays;
    TraceRange rgA("yart:aov_finish", stream);
    hipLaunchKernelGGL(k_aov_finish, dim3((pl.nPix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, f);
    HIP_CHECK(hipGetLastError());
  }
  if (pl.mom) {
    const YartMomentBuffers* mom = pl.mom;
    MomentFinishArgs f{};
    f.state = s.momState.p; f.pixels = s.pixels.p; f.nPixels = pl.nPix; f.width = pl.W; f.mask = mom->mask;
    f.mean = mom->mean; f.variance = mom->variance; f.count = mom->count;
    TraceRange rgM("yart:moments_finish", stream);
    hipLaunchKernelGGL(k_moments_finish, dim3((pl.nPix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, f);
    HIP_CHECK(hipGetLastError());
  }
}

// YartStats of a finished render (ms_total is the caller's); cnt: the device counters, renderedSamples: per pixel
YartStats makeStats(const YartScene& s, const RenderPlan& pl, const StageTimers& t, const unsigned long long* cnt, float msAll,
                    uint32_t waves, uint64_t renderedSamples) {
  YartStats st{};
  st.samples = uint64_t(pl.nPix) * renderedSamples;
  st.rays = cnt[0];
  st.traversals = cnt[1]; st.box_tests = cnt[2]; st.tri_tests = cnt[3]; st.shaded_hits = cnt[4];
  st.ms_device = msAll;
  st.ms_traverse = pl.mega ? t.mega.ms : t.extend.ms + t.connect.ms;
  st.launches_traverse = pl.mega ? t.mega.launches : t.extend.launches + t.connect.launches;
  st.ms_extend = t.extend.ms; st.ms_shade = t.shade.ms; st.ms_connect = t.connect.ms; st.ms_gmon = t.gmon.ms;
  st.ms_extend_lean = t.lean.ms; st.launches_extend_lean = t.lean.launches;
  st.lean_traversals = cnt[5]; st.lean_box_tests = cnt[6]; st.lean_tri_tests = cnt[7];
  st.ms_shade_kernel = t.shadeK.ms; st.launches_shade_kernel = t.shadeK.launches;
  st.ms_shadow_lean = t.shadowLean.ms; st.launches_shadow_lean = t.shadowLean.launches;
  st.shadow_lean_traversals = cnt[24]; st.shadow_lean_box_tests = cnt[25]; st.shadow_lean_tri_tests = cnt[26];
  st.shade_entries = cnt[28]; st.retry_extend_traversals = cnt[29]; st.retry_shadow_traversals = cnt[30];
  st.pipeline_flags = pl.effFlags;
  {
    unsigned long long paths[16] = {0};
    HIP_CHECK(hipMemcpy(paths, s.pathsLog.p, sizeof(paths), hipMemcpyDeviceToHost));
    for (int b = 0; b < 16; b++) st.paths_at_bounce[b] = paths[b];
    st.paths_at_bounce[0] = pl.mega || pl.pool ? 0 : uint64_t(pl.nPix) * renderedSamples;     // (every path enters bounce 0)
  }
#if defined(YART_COUNT_TRAVERSAL)
  {
    unsigned long long tb = 0;
    HIP_CHECK(hipMemcpyFromSymbol(&tb, HIP_SYMBOL(g_texTapBytes), sizeof(tb)));
    tb += tu::texTapRead1() + tu::texTapRead2() + tu::texTapRead3() + tu::texTapRead4();
    st.texture_tap_bytes = tb;
  }
#endif
  st.launches_extend = t.extend.launches; st.launches_connect = t.connect.launches;
  st.waves = waves;
  return st;
}

// Plan, buffers, sampler tables; then wave by wave (resumable accumulation: only the waves inside [start_sample, stop_sample))
// and batch by batch through the plan's pipeline; then the finish kernels and the statistics. true: the hook stopped the render.
bool renderToDevice(YartScene& s, const YartCameraDesc& camDesc, const YartRenderParams& p, float* dOut,
                    hipStream_t stream, YartStats* stats, const BatchHook* hook = nullptr, const YartAovBuffers* aov = nullptr,
                    const YartMomentBuffers* mom = nullptr) {
  bool aborted = false;
  auto wall0 = std::chrono::high_resolution_clock::now();
  TraceRange rgRender("yart:render");
  HIP_CHECK(hipSetDevice(s.device));
  buildPixelList(s, camDesc.width, camDesc.height, p.shard_tile ? p.shard_tile : p.tile_size, p.rank, p.world_size);
  const uint64_t startSample = p.start_sample, stopSample = p.stop_sample ? p.stop_sample : p.samples;
  if (startSample == 0) HIP_CHECK(hipMemsetAsync(dOut, 0, size_t(camDesc.width) * camDesc.height * 4 * sizeof(float), stream));
  s.cursor.ensure(1); s.counters.ensure(kNumCounters); s.pathsLog.ensure(16);
  HIP_CHECK(hipMemsetAsync(s.pathsLog.p, 0, 16 * sizeof(unsigned long long), stream));
  HIP_CHECK(hipMemsetAsync(s.counters.p, 0, kNumCounters * sizeof(unsigned long long), stream));
#if defined(YART_COUNT_TRAVERSAL)
  { const unsigned long long zero = 0; HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_texTapBytes), &zero, sizeof(zero))); tu::texTapReset1(); tu::texTapReset2(); tu::texTapReset3(); tu::texTapReset4(); }
#endif
  RenderPlan pl = makeRenderPlan(s, camDesc, p, aov, mom, stream);
  prepareBuffers(s, pl, stream);

  Timer tAll;
  StageTimers t;
  uint32_t waves = 0;
  uint64_t renderedSamples = 0;
  HIP_CHECK(hipEventRecord(tAll.a, stream));
  launchSamplerTables(s, pl, t, stream);
  const auto runBatch = pl.mega ? runMegaBatch : pl.pool ? runPoolBatch : runWavefrontBatch;

  for (WaveSchedule ws(p.samples, p.first_wave_samples, p.max_wave_samples); !aborted && ws.next();) {
    // resumable accumulation: waves outside [start_sample, stop_sample) are not rendered by this call
    const bool inRange = ws.takenBefore >= startSample && ws.takenBefore < stopSample;
    if (!inRange && ws.takenBefore < startSample && ws.takenAfter > startSample) throw std::invalid_argument("start_sample is not a wave boundary");
    if (inRange && ws.takenAfter > stopSample) throw std::invalid_argument("stop_sample is not a wave boundary");
    if (!inRange) continue;
    waves++; renderedSamples += ws.samples;
    WaveInfo w{uint32_t(ws.wave), uint32_t(ws.takenAfter), float(ws.takenBefore) / float(ws.takenAfter), float(ws.samples) / float(ws.takenAfter), 0};
    for (uint32_t c0 = 0; !aborted && c0 < pl.nPix; c0 += pl.chunk) {
      const Batch b{c0, std::min(pl.chunk, pl.nPix - c0), uint32_t(ws.samples), uint32_t(ws.takenBefore)};
      runBatch(s, pl, b, t, stream);
      aborted = finishBatch(s, pl, b, w, dOut, t, hook, stream);
    }
  }
  if (!aborted) launchFinishKernels(s, pl, stream);
  HIP_CHECK(hipEventRecord(tAll.b, stream));
  HIP_CHECK(hipEventSynchronize(tAll.b));
  float msAll = 0; HIP_CHECK(hipEventElapsedTime(&msAll, tAll.a, tAll.b));
  unsigned long long cnt[kNumCounters] = {0};
  HIP_CHECK(hipMemcpy(cnt, s.counters.p, sizeof(cnt), hipMemcpyDeviceToHost));
  for (int i = 0; i < kNumCounters; i++) s.lastCounters[i] = cnt[i];
  if (stats) {
    *stats = makeStats(s, pl, t, cnt, msAll, waves, renderedSamples);
    stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - wall0).count();
  }
  return aborted;
}

struct RcclFailure : std::runtime_error { using std::runtime_error::runtime_error; };

template <class F>
int guarded(F&& f) {
  try {
    f();
    return YART_OK;
  } catch (const RcclFailure& e) {
    g_lastError = e.what(); return YART_E_RCCL;
  } catch (const std::invalid_argument& e) {
    g_lastError = e.what(); return YART_E_INVALID;
  } catch (const HipError& e) {
    g_lastError = e.what();
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return YART_E_NO_DEVICE;
    return YART_E_HIP;
  } catch (const std::exception& e) {
    g_lastError = e.what(); return YART_E_IO;
  }
}

}  // namespace

namespace {
std::unique_ptr<LoadedScene> importGltf(const char* path, const YartImportOptions* opts) {
  auto loaded = gltf::loadGltf(path);
  if (opts) {
    const float radius = opts->env_radius > 0.0f ? opts->env_radius : 100.0f;      // frontend main.cpp:82
    if (opts->env_hdr_path && opts->env_hdr_path[0]) gltf::addImageEnvironment(*loaded, opts->env_hdr_path, radius);
    if (opts->uniform_env) gltf::addUniformEnvironment(*loaded, opts->uniform_emission, radius);
  }
  return loaded;
}
}  // namespace

#include "multi_device.inc"

extern "C" {

int yart_hip_abi_version(void) { return YART_HIP_ABI_VERSION; }

int yart_hip_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

const char* yart_hip_last_error(void) { return g_lastError.c_str(); }

int yart_hip_scene_create(const YartSceneDesc* desc, int device, YartScene** out) {
  return guarded([&] {
    require(desc && out, "desc / out pointer is null");
    *out = createScene(*desc, device);
  });
}

int yart_hip_scene_create_flags(const YartSceneDesc* desc, int device, uint32_t scene_flags, YartScene** out) {
  return guarded([&] {
    require(desc && out, "desc / out pointer is null");
    *out = createScene(*desc, device, scene_flags);
  });
}

int yart_hip_scene_load(const char* path, int device, YartScene** out) {
  return guarded([&] {
    require(path && out, "path / out pointer is null");
    auto loaded = loadSceneFile(path);
    *out = createScene(loaded->desc, device);
  });
}

int yart_hip_scene_load_gltf(const char* path, const YartImportOptions* opts, int device, YartScene** out) {
  return guarded([&] {
    require(path && out, "path / out pointer is null");
    auto loaded = importGltf(path, opts);
    *out = createScene(loaded->desc, device);
  });
}

int yart_hip_gltf_to_yscn(const char* gltf_path, const YartImportOptions* opts, const char* yscn_path) {
  return guarded([&] {
    require(gltf_path && yscn_path, "path pointer is null");
    auto loaded = importGltf(gltf_path, opts);
    saveSceneFile(loaded->desc, yscn_path);
  });
}

void yart_hip_scene_destroy(YartScene* scene) {
  if (!scene) return;
  (void)hipSetDevice(scene->device);
  delete scene;
}

int yart_hip_render_device(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                           float* d_out_rgba, void* stream, YartStats* stats) {
  return guarded([&] {
    require(scene && d_out_rgba, "scene / output pointer is null");
    validate(cam, params);
    std::lock_guard<std::mutex> lock(scene->mu);
    renderToDevice(*scene, *cam, *params, d_out_rgba, static_cast<hipStream_t>(stream), stats);
  });
}

// The frame of the host-pointer render entries, opened after an entry's last argument check: the scene's lock, the call's clock,
// the scene's device, and its frame buffer holding the caller's accumulated frame when the render resumes
struct HostFrame {
  YartScene& s;
  float* const out; const size_t n;                                     // the caller's frame, its floats
  std::lock_guard<std::mutex> lock;
  const std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
  HostFrame(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba)
      : s(*scene), out(out_rgba), n(size_t(cam->width) * cam->height * 4), lock(scene->mu) {
    HIP_CHECK(hipSetDevice(s.device));
    s.hdr.ensure(n);
    if (params->start_sample > 0) HIP_CHECK(hipMemcpy(s.hdr.p, out, n * sizeof(float), hipMemcpyHostToDevice));
  }
  void copyBack() const { HIP_CHECK(hipMemcpy(out, s.hdr.p, n * sizeof(float), hipMemcpyDeviceToHost)); }
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count(); }
};

int yart_hip_render(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba, YartStats* stats) {
  return guarded([&] {
    require(scene && out_rgba, "scene / output pointer is null");
    validate(cam, params);
    HostFrame f(scene, cam, params, out_rgba);
    renderToDevice(*scene, *cam, *params, scene->hdr.p, nullptr, stats);
    f.copyBack();
    if (stats) stats->ms_total = f.ms();                        // the whole call's wall time, copies included
  });
}

// Feature buffers: the caller's YartAovBuffers checked (before anything touches a device) and copied into a struct of this
// build's size; false: nothing is requested (a plain render)
static bool checkAovs(const YartAovBuffers* in, const YartCameraDesc* cam, const YartRenderParams* params, YartAovBuffers& out) {
  out = YartAovBuffers{};
  if (in) checkAndCopyBuffers(kAovTable, *in, out);
  validate(cam, params);
  if (out.mask != 0u)
    require(params->start_sample == 0 && (params->stop_sample == 0 || params->stop_sample == params->samples),
            "feature buffers need the full sample range (start_sample = 0, stop_sample = 0 or samples)");
  return out.mask != 0u;
}

// Sample moments: the caller's YartMomentBuffers checked (before anything touches a device) and copied into a struct of this
// build's size; false: nothing is requested
static bool checkMoments(const YartMomentBuffers* in, const YartRenderParams* params, YartMomentBuffers& out) {
  out = YartMomentBuffers{};
  if (in) checkAndCopyBuffers(kMomentTable, *in, out);
  if (out.mask != 0u && params)
    require(params->start_sample == 0 && (params->stop_sample == 0 || params->stop_sample == params->samples),
            "sample moments need the full sample range (start_sample = 0, stop_sample = 0 or samples)");
  return out.mask != 0u;
}

int yart_hip_render_moments_device(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* d_out_rgba,
                                   const YartAovBuffers* d_aovs, const YartMomentBuffers* d_moments, void* stream, YartStats* stats) {
  return guarded([&] {
    YartAovBuffers av;
    YartMomentBuffers mv;
    const bool any = checkAovs(d_aovs, cam, params, av);
    const bool anyM = checkMoments(d_moments, params, mv);
    require(scene && d_out_rgba, "scene / output pointer is null");
    std::lock_guard<std::mutex> lock(scene->mu);
    renderToDevice(*scene, *cam, *params, d_out_rgba, static_cast<hipStream_t>(stream), stats, nullptr, any ? &av : nullptr,
                   anyM ? &mv : nullptr);
  });
}

int yart_hip_render_aovs_device(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* d_out_rgba,
                                const YartAovBuffers* d_aovs, void* stream, YartStats* stats) {
  return yart_hip_render_moments_device(scene, cam, params, d_out_rgba, d_aovs, nullptr, stream, stats);
}

int yart_hip_render_moments(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                            const YartAovBuffers* aovs, const YartMomentBuffers* moments, YartStats* stats) {
  return guarded([&] {
    YartAovBuffers host;
    YartMomentBuffers hostM;
    const bool any = checkAovs(aovs, cam, params, host);
    const bool anyM = checkMoments(moments, params, hostM);
    require(scene && out_rgba, "scene / output pointer is null");
    HostFrame f(scene, cam, params, out_rgba);
    const size_t wh = f.n / 4;
    // the requested buffers side by side in one device allocation each (render_host.hpp: kAovTable, kMomentTable)
    YartAovBuffers dev = host;
    if (any) {
      scene->aovOut.ensure(layOutBuffers(kAovTable, host.mask, wh, nullptr, dev));
      layOutBuffers(kAovTable, host.mask, wh, scene->aovOut.p, dev);
    }
    YartMomentBuffers devM = hostM;
    if (anyM) {
      scene->momOut.ensure(layOutBuffers(kMomentTable, hostM.mask, wh, nullptr, devM));
      layOutBuffers(kMomentTable, hostM.mask, wh, scene->momOut.p, devM);
    }
    renderToDevice(*scene, *cam, *params, scene->hdr.p, nullptr, stats, nullptr, any ? &dev : nullptr, anyM ? &devM : nullptr);
    f.copyBack();
    const auto toHost = [](void* dst, const void* src, size_t bytes) { HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); };
    if (any) copyBuffers(kAovTable, host, dev, wh, toHost);
    if (anyM) copyBuffers(kMomentTable, hostM, devM, wh, toHost);
    if (stats) stats->ms_total = f.ms();
  });
}

int yart_hip_render_aovs(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                         const YartAovBuffers* aovs, YartStats* stats) {
  return yart_hip_render_moments(scene, cam, params, out_rgba, aovs, nullptr, stats);
}

// One wave of the schedule at a time, and inside a wave one batch at a time (tile-renderer.hpp:200-309: finishTile
// fires onRenderTileComplete per tile and onRenderWaveComplete after a wave's last tile).
static int renderProgressive(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                             YartStats* stats, YartWaveCallback on_wave, YartTileCallback on_tile, void* user) {
  bool aborted = false;
  const int rc = guarded([&] {
    require(scene && out_rgba, "scene / output pointer is null");
    validate(cam, params);
    HostFrame f(scene, cam, params, out_rgba);
    const uint32_t W = cam->width;
    const uint32_t stop = params->stop_sample ? params->stop_sample : params->samples;
    if (params->start_sample == 0 && on_tile) std::memset(out_rgba, 0, f.n * sizeof(float));   // tiles arrive one by one: the rest of the frame is defined
    YartStats total{};
    for (WaveSchedule ws(params->samples, params->first_wave_samples, params->max_wave_samples); !aborted && ws.next();) {
      const uint32_t taken = uint32_t(ws.takenBefore);
      const uint64_t wave = ws.wave, waveSamples = ws.samples;
      if (taken >= params->start_sample && taken < stop) {
        YartRenderParams q = *params;
        q.start_sample = taken; q.stop_sample = uint32_t(taken + waveSamples);
        YartStats st{};
        auto tw = std::chrono::high_resolution_clock::now();
        size_t nextTile = 0;                 // tiles are in pixel-list order: everything before nextTile has been reported
        BatchHook hook = [&](const BatchInfo& b) {
          // the tiles whose last pixel lies in this batch are final for this wave: copy them out and report them
          const auto& tiles = scene->tiles;
          bool stopNow = false;
          while (nextTile < tiles.size() && tiles[nextTile].start + tiles[nextTile].count <= b.c0 + b.n) {
            const YartScene::TileRec& t = tiles[nextTile++];
            const size_t off = (size_t(t.y) * W + t.x) * 4;
            HIP_CHECK(hipMemcpy2D(out_rgba + off, size_t(W) * 16, scene->hdr.p + off, size_t(W) * 16, size_t(t.w) * 16, t.h,
                                  hipMemcpyDeviceToHost));
            YartTileInfo ti{};
            ti.x = t.x; ti.y = t.y; ti.width = t.w; ti.height = t.h;
            ti.index = uint32_t(nextTile); ti.total = uint32_t(tiles.size());
            ti.wave = b.wave; ti.wave_samples = b.waveSamples; ti.samples_taken = b.samplesTaken; ti.total_samples = b.totalSamples;
            ti.rays = nextTile - 1 < scene->tileRaysHost.size() ? scene->tileRaysHost[nextTile - 1] : 0;
            ti.ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - tw).count();
            if (on_tile(user, &ti) != 0) stopNow = true;
          }
          return stopNow;
        };
        const bool stopped = renderToDevice(*scene, *cam, q, scene->hdr.p, nullptr, &st, on_tile ? &hook : nullptr);
        // after a wave the whole frame (with a tile callback: every tile has been copied already unless the render stopped)
        if (!on_tile || stopped) f.copyBack();
        total.rays += st.rays; total.waves += st.waves; total.ms_device += st.ms_device; total.samples += st.samples;
        total.ms_extend += st.ms_extend; total.ms_shade += st.ms_shade; total.ms_connect += st.ms_connect; total.ms_gmon += st.ms_gmon;
        total.ms_traverse += st.ms_traverse; total.launches_traverse += st.launches_traverse;
        total.pipeline_flags = st.pipeline_flags;
        st.ms_total = f.ms();
        if (stopped) aborted = true;
        else if (on_wave && on_wave(user, &st, uint32_t(wave), uint32_t(waveSamples), uint32_t(taken + waveSamples), params->samples) != 0)
          aborted = true;
      }
    }
    total.ms_total = f.ms();
    if (stats) *stats = total;
  });
  return rc == YART_OK && aborted ? YART_ABORTED : rc;
}

int yart_hip_render_waves(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                          float* out_rgba, YartStats* stats, YartWaveCallback on_wave, void* user) {
  return renderProgressive(scene, cam, params, out_rgba, stats, on_wave, nullptr, user);
}

int yart_hip_render_tiles(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                          float* out_rgba, YartStats* stats, YartWaveCallback on_wave, YartTileCallback on_tile, void* user) {
  return renderProgressive(scene, cam, params, out_rgba, stats, on_wave, on_tile, user);
}

int yart_hip_multi_create(const YartSceneDesc* desc, const int* devices, uint32_t n_devices, YartMulti** out) {
  return guarded([&] {
    require(desc && out, "desc / out pointer is null");
    *out = createMulti(*desc, devices, n_devices);
  });
}

int yart_hip_multi_load(const char* path, const YartImportOptions* opts, const int* devices, uint32_t n_devices, YartMulti** out) {
  return guarded([&] {
    require(path && out, "path / out pointer is null");
    const std::string p(path);
    const bool gltf = p.size() > 4 && (p.rfind(".glb") == p.size() - 4 || p.rfind(".gltf") == p.size() - 5);
    auto loaded = gltf ? importGltf(path, opts) : loadSceneFile(path);
    *out = createMulti(loaded->desc, devices, n_devices);
  });
}

void yart_hip_multi_destroy(YartMulti* multi) { delete multi; }

int yart_hip_multi_rccl_selftest(int device, uint32_t n_floats) {
  return guarded([&] {
    require(n_floats > 0 && n_floats <= (1u << 26), "n_floats out of range");
    const int dev = resolveDevice(device);
    if (dev < 0) throw HipError("no usable HIP device (libyart_hip has no CPU fallback)");
    HIP_CHECK(hipSetDevice(dev));
    // the calls of mergeSlabs on a one-rank communicator: the rank sends a slab to itself (matching send / recv in one group)
    const RcclApi& R = rccl();
    ncclComm_t comm = nullptr;
    RCCL_CHECK(R.CommInitAll(&comm, 1, &dev));
    hipStream_t st = nullptr;
    DevBuf<float> a, b;
    std::vector<float> h(n_floats), back(n_floats, 0.0f);
    for (uint32_t i = 0; i < n_floats; i++) h[i] = float(i % 8191u) * 0.25f - 3.0f;
    try {
      HIP_CHECK(hipStreamCreate(&st));
      a.upload(h); b.ensure(n_floats);
      HIP_CHECK(hipMemsetAsync(b.p, 0, size_t(n_floats) * 4, st));
      RCCL_CHECK(R.GroupStart());
      ncclResult_t e = R.Send(a.p, n_floats, ncclFloat, 0, comm, st);
      if (e == ncclSuccess) e = R.Recv(b.p, n_floats, ncclFloat, 0, comm, st);
      const ncclResult_t ge = R.GroupEnd();                 // closed whatever the calls inside returned
      RCCL_CHECK(e);
      RCCL_CHECK(ge);
      HIP_CHECK(hipStreamSynchronize(st));
      HIP_CHECK(hipMemcpy(back.data(), b.p, size_t(n_floats) * 4, hipMemcpyDeviceToHost));
    } catch (...) {
      if (st) (void)hipStreamDestroy(st);
      (void)R.CommDestroy(comm);
      throw;
    }
    (void)hipStreamDestroy(st);
    RCCL_CHECK(R.CommDestroy(comm));
    if (std::memcmp(h.data(), back.data(), size_t(n_floats) * 4) != 0) throw RcclFailure("rccl selftest: the received slab differs from the sent one");
  });
}

int yart_hip_multi_device_count(const YartMulti* multi) { return multi ? int(multi->scenes.size()) : 0; }

int yart_hip_multi_failed_devices(const YartMulti* multi, int* replicas_out, uint32_t capacity) {
  if (!multi) return 0;
  int nf = 0;
  for (size_t i = 0; i < multi->failed.size(); i++)
    if (multi->failed[i]) { if (replicas_out && uint32_t(nf) < capacity) replicas_out[nf] = int(i); nf++; }
  if (nf) g_lastError = multi->failureNote;
  return nf;
}

int yart_hip_multi_render(YartMulti* multi, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                          YartStats* stats) {
  return guarded([&] {
    require(multi && out_rgba, "multi / output pointer is null");
    validate(cam, params);
    renderMulti(*multi, *cam, *params, out_rgba, stats);
  });
}

int yart_hip_multi_render_tiles(YartMulti* multi, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                                YartStats* stats, YartWaveCallback on_wave, YartTileCallback on_tile, void* user) {
  bool aborted = false;
  const int rc = guarded([&] {
    require(multi && out_rgba, "multi / output pointer is null");
    validate(cam, params);
    aborted = renderMultiProgressive(*multi, *cam, *params, out_rgba, stats, on_wave, on_tile, user) == YART_ABORTED;
  });
  return rc == YART_OK && aborted ? YART_ABORTED : rc;
}

int yart_hip_debug_counters(YartScene* scene, uint64_t* out32) {
  return guarded([&] {
    require(scene && out32, "null pointer");
    for (int i = 0; i < kNumCounters; i++) out32[i] = scene->lastCounters[i];
  });
}

/* debug build -DYART_SHADE_REGIONS=1 only (tools/shade_regions.py): cycles / visits / lanes per code region of k_wf_shade,
 * summed over the renders since the last call (16 regions x 3); -1 otherwise */
int yart_hip_debug_shade_regions(uint64_t* out48) {
#if defined(YART_SHADE_REGIONS)
  return guarded([&] {
    require(out48 != nullptr, "null pointer");
    unsigned long long v[3 * 16];
    tu::shadeRegionsTake(v);
    for (int i = 0; i < 48; i++) out48[i] = v[i];
  });
#else
  (void)out48;
  return YART_E_INVALID;
#endif
}

int yart_hip_bvh_info(YartScene* scene, uint32_t mesh, uint32_t* n_nodes, uint32_t* n_tris) {
  return guarded([&] {
    require(scene && n_nodes && n_tris, "null pointer");
    require(mesh < scene->host.meshes.size(), "mesh index out of range");
    *n_nodes = scene->host.meshes[mesh].nNodes;
    *n_tris = scene->host.meshes[mesh].nTris;
  });
}

int yart_hip_bvh_copy(YartScene* scene, uint32_t mesh, uint32_t* nodes_out, uint32_t* indices_out) {
  return guarded([&] {
    require(scene && nodes_out && indices_out, "null pointer");
    require(mesh < scene->host.meshes.size(), "mesh index out of range");
    const MeshDev& m = scene->host.meshes[mesh];
    // read the node array back from the DEVICE copy: this is what the kernels traverse
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipMemcpy(nodes_out, scene->bvhNodes.p + m.nodeOffset, size_t(m.nNodes) * sizeof(BvhNode),
                        hipMemcpyDeviceToHost));
    for (uint32_t n = 0; n < m.nNodes; n++) nodes_out[size_t(n) * 8 + 6] &= kLinkIndexMask;   // the reference's index only
    std::memcpy(indices_out, scene->host.bvhIndices[mesh].data(), size_t(m.nTris) * 4);
  });
}

// the arguments yart_hip_bvh_build_device and yart_hip_bvh_build_host share
static void checkBvhBuildArgs(const float* positions, uint32_t n_verts, const uint32_t* faces, uint32_t face_stride, uint32_t n_faces,
                              const uint32_t* nodes_out, const uint32_t* indices_out, const uint32_t* n_nodes) {
  require(positions && faces && nodes_out && indices_out && n_nodes, "null pointer");
  require(n_faces >= 1 && n_faces <= kLinkIndexMask && face_stride >= 3, "bvh build: bad triangle count or stride");
  for (size_t k = 0; k < size_t(n_faces) * face_stride; k += face_stride)
    for (int c = 0; c < 3; c++) require(faces[k + c] < n_verts, "bvh build: vertex index out of range");
}

int yart_hip_bvh_build_device(int device, const float* positions, uint32_t n_verts, const uint32_t* faces, uint32_t face_stride,
                              uint32_t n_faces, uint32_t* nodes_out, uint32_t* indices_out, uint32_t* n_nodes, double* ms_device) {
  return guarded([&] {
    checkBvhBuildArgs(positions, n_verts, faces, face_stride, n_faces, nodes_out, indices_out, n_nodes);
    std::vector<BvhNode> nodes;
    std::vector<uint32_t> indices;
    require(devbvh::build(device, positions, n_verts, faces, face_stride, n_faces, nodes, indices, ms_device),
            "bvh build: refused on the device (NaN coordinate or tree deeper than 192 levels): build on the host");
    *n_nodes = uint32_t(nodes.size());
    std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(BvhNode));
    std::memcpy(indices_out, indices.data(), indices.size() * 4);
  });
}

int yart_hip_bvh_build_host(const float* positions, uint32_t n_verts, const uint32_t* faces, uint32_t face_stride, uint32_t n_faces,
                            uint32_t threads, uint32_t* nodes_out, uint32_t* indices_out, uint32_t* n_nodes, double* ms_host) {
  return guarded([&] {
    checkBvhBuildArgs(positions, n_verts, faces, face_stride, n_faces, nodes_out, indices_out, n_nodes);
    const auto t0 = std::chrono::steady_clock::now();
    SahBvhBuilder b;
    b.setThreads(threads);
    b.build(positions, faces, face_stride, n_faces);
    if (ms_host) *ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *n_nodes = uint32_t(b.nodes.size());
    std::memcpy(nodes_out, b.nodes.data(), b.nodes.size() * sizeof(BvhNode));
    std::memcpy(indices_out, b.indices.data(), b.indices.size() * 4);
  });
}

}  // extern "C"

#include "postprocess.inc"
#include "scene_update_common.inc"
#include "tlas_build_kernels.inc"
#include "scene_update_kernels.inc"
#include "graph_update_kernels.inc"
#include "mesh_update_kernels.inc"
#include "mesh_replace_kernels.inc"
#include "lighting_update_kernels.inc"
#include "texture_update_kernels.inc"
#include "scene_motion_kernels.inc"
#include "probes.inc"
