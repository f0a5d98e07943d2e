// multi_device.inc — several GPUs of one node behind one C-ABI handle (included by yart_hip.hip, unit 0).
//
// Stands where the reference's worker pool stands: TileRenderer::renderImpl starts `threadCount` threads that pull
// tiles (tile-renderer.hpp:150-197) and finishTile merges every finished tile into the one m_hdrBuffer (:225-241).
// Here a "worker" is a GPU: the scene is replicated on every device, device i of N renders the pixel blocks
// b with b % N == i (Morton order, as YartRenderParams.rank / world_size do across processes), one host thread per
// device drives its launches, and the merge moves each device's pixels — a slab holding ONLY its own pixels, in its
// pixel-list order (1/N of the frame per device, no zero-summing) — to device 0 over xGMI with RCCL point-to-point
// calls (ncclSend / ncclRecv in one group), where an unpack kernel scatters them into the frame.
//
// Devices listed more than once (a one-GPU box) take the same path except for the transport, which is then a
// device-to-device copy on that GPU: RCCL cannot put two ranks of one communicator on one device. That form exists so
// that the threading, the slab layout and the scatter run on the hardware at hand; the RCCL form is what an 8-GPU
// node runs.
#include <rccl/rccl.h>      // types and prototypes only: the library itself is loaded on first use (below)
#include <dlfcn.h>

#include <thread>

namespace {

// RCCL is loaded with dlopen the first time a multi-device entry point needs it, so that libyart_hip.so loads — and the
// single-GPU path works — on a host without librccl. A missing library surfaces as YART_E_RCCL from those entry points.
struct RcclApi {
  decltype(&::ncclCommInitAll) CommInitAll = nullptr;
  decltype(&::ncclCommDestroy) CommDestroy = nullptr;
  decltype(&::ncclCommAbort) CommAbort = nullptr;
  decltype(&::ncclGroupStart) GroupStart = nullptr;
  decltype(&::ncclGroupEnd) GroupEnd = nullptr;
  decltype(&::ncclSend) Send = nullptr;
  decltype(&::ncclRecv) Recv = nullptr;
  decltype(&::ncclGetErrorString) GetErrorString = nullptr;
};
const RcclApi& rccl() {
  static RcclApi api;
  static std::once_flag once;
  static std::string error;
  std::call_once(once, [] {
    void* h = nullptr;
    // YART_RCCL_LIB names the library (an RCCL build elsewhere; tests/fake_rccl: a stand-in that runs this file's RCCL branch, and
    // its failure paths, on a one-GPU box). Named and not loadable = an error, not a silent fall-back to the system's.
    const char* named = std::getenv("YART_RCCL_LIB");
    if (named && *named) {
      h = dlopen(named, RTLD_NOW | RTLD_LOCAL);
      if (!h) { const char* why = dlerror(); error = std::string("YART_RCCL_LIB=") + named + " could not be loaded: " + (why ? why : "not found"); return; }
    }
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
      if (h) break;
      h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    }
    // (dlerror() clears the message it returns: one call)
    if (!h) { const char* why = dlerror(); error = std::string("librccl.so could not be loaded: ") + (why ? why : "not found"); return; }
    auto sym = [&](const char* n) -> void* {
      void* f = dlsym(h, n);
      if (!f && error.empty()) error = std::string("librccl.so lacks ") + n;
      return f;
    };
    api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(sym("ncclCommInitAll"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.CommAbort = reinterpret_cast<decltype(api.CommAbort)>(sym("ncclCommAbort"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
  });
  if (!error.empty()) throw RcclFailure(error);
  return api;
}

#define RCCL_CHECK(expr)                                                                    \
  do {                                                                                      \
    ncclResult_t _r = (expr);                                                               \
    if (_r != ncclSuccess) throw RcclFailure(std::string(#expr) + ": " + rccl().GetErrorString(_r)); \
  } while (0)

__global__ void __launch_bounds__(kBlock) k_pack_pixels(const f4* frame, const uint32_t* pixels, uint32_t n, uint32_t W, f4* slab) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t pk = pixels[i];
    slab[i] = frame[size_t(pk >> 16) * W + (pk & 0xffffu)];
  }
}
__global__ void __launch_bounds__(kBlock) k_unpack_pixels(const f4* slab, const uint32_t* pixels, uint32_t n, uint32_t W, f4* frame) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t pk = pixels[i];
    frame[size_t(pk >> 16) * W + (pk & 0xffffu)] = slab[i];
  }
}

// (re-queued share: its pixels from the frame it was rendered into, both on devices[0])
__global__ void __launch_bounds__(kBlock) k_copy_pixels(const f4* src, const uint32_t* pixels, uint32_t n, uint32_t W, f4* dst) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t pk = pixels[i];
    const size_t at = size_t(pk >> 16) * W + (pk & 0xffffu);
    dst[at] = src[at];
  }
}

}  // namespace

struct YartMulti {
  std::vector<YartScene*> scenes;          // one replica per entry of `devices`
  std::vector<int> devices;
  bool distinct = true;                    // every device listed once -> RCCL transport
  bool rcclBroken = false;                 // a merge failed inside its RCCL group: the communicators were aborted
  // A replica whose device failed a render (a HIP error on its thread) is taken out of service; its pixel blocks are re-queued on
  // devices[0] from then on (SURVEY §5 "failure detection": tiles are idempotent; the reference has nothing of the kind — a worker
  // that dies takes the process with it). yart_hip_multi_failed_devices reports them.
  std::vector<uint8_t> failed;
  std::string failureNote;
  DevBuf<float> requeueFrame;              // on devices[0]: the frame a re-queued share is rendered into
  uint32_t rendersDone = 0;                // (fault injection counts renders: YART_FAULT_REPLICA / YART_FAULT_AT)
  std::vector<ncclComm_t> comms;           // distinct only
  std::vector<hipStream_t> streams;        // one merge stream per replica
  std::vector<DevBuf<f4>> slab;            // per replica: its own pixels, packed
  std::vector<DevBuf<f4>> recv;            // on devices[0]: the slab of replica i (i > 0)
  std::vector<DevBuf<uint32_t>> recvPixels;// on devices[0]: the pixel list of replica i
  std::vector<std::vector<uint32_t>> pixelLists;
  uint32_t plW = 0, plH = 0, plTile = 0, plRank = 0, plWorld = 0;
  std::mutex mu;
  ~YartMulti() {
    for (size_t i = 0; i < comms.size(); i++) if (comms[i]) (void)rccl().CommDestroy(comms[i]);
    for (size_t i = 0; i < streams.size(); i++) if (streams[i]) { (void)hipSetDevice(devices[i]); (void)hipStreamDestroy(streams[i]); }
    for (size_t i = 0; i < scenes.size(); i++) if (scenes[i]) { (void)hipSetDevice(devices[i]); delete scenes[i]; }
    // DevBufs of device 0 / device i are released by their destructors on whichever device is current: hipFree takes any
  }
};

namespace {

YartMulti* createMulti(const YartSceneDesc& desc, const int* devices, uint32_t n) {
  require(devices && n > 0 && n <= 64, "devices: 1 to 64 device indices");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw HipError("no usable HIP device (libyart_hip has no CPU fallback)");
  auto m = std::make_unique<YartMulti>();
  for (uint32_t i = 0; i < n; i++) {
    require(devices[i] >= 0 && devices[i] < count, "devices: index out of range");
    for (uint32_t k = 0; k < i; k++) if (devices[k] == devices[i]) m->distinct = false;
    m->devices.push_back(devices[i]);
  }
  // Rehearsal of the RCCL branch on a one-GPU box: with a stand-in library named by YART_RCCL_LIB (the real one refuses two
  // ranks of one communicator on one device) YART_MULTI_ASSUME_DISTINCT=1 sends a repeated device list down the distinct path.
  if (!m->distinct && std::getenv("YART_RCCL_LIB") && std::getenv("YART_MULTI_ASSUME_DISTINCT")) m->distinct = true;
  // BVH build (on the first device, as createScene does) and flattening once; every replica uploads a copy
  int dev0 = m->devices[0];
  HostImage host = std::getenv("YART_HOST_BVH") ? buildHostImage(desc) : buildHostImage(desc, deviceMeshBvh, &dev0);
  m->scenes.resize(n, nullptr); m->streams.resize(n, nullptr); m->failed.assign(n, 0);
  m->slab = std::vector<DevBuf<f4>>(n); m->recv = std::vector<DevBuf<f4>>(n); m->recvPixels = std::vector<DevBuf<uint32_t>>(n);
  for (uint32_t i = 0; i < n; i++) {
    HIP_CHECK(hipSetDevice(m->devices[i]));
    auto s = std::make_unique<YartScene>();
    s->device = m->devices[i];
    s->host = host;
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, s->device));
    s->numCUs = prop.multiProcessorCount;
    uploadScene(*s);
    m->scenes[i] = s.release();
    HIP_CHECK(hipStreamCreateWithFlags(&m->streams[i], hipStreamNonBlocking));   // (replicas that share a device run side by side)
  }
  if (m->distinct && n > 1) {
    m->comms.resize(n, nullptr);
    RCCL_CHECK(rccl().CommInitAll(m->comms.data(), int(n), m->devices.data()));
  }
  return m.release();
}

// merge of the replicas' frames into replica 0's (s0.hdr); see the head of this file
void mergeSlabs(YartMulti& m, uint32_t W, uint32_t H, uint32_t block, uint32_t rank, uint32_t world) {
  const uint32_t n = uint32_t(m.scenes.size());
  if (m.plW != W || m.plH != H || m.plTile != block || m.plRank != rank || m.plWorld != world) {
    m.pixelLists.assign(n, {});
    HIP_CHECK(hipSetDevice(m.devices[0]));
    for (uint32_t i = 1; i < n; i++) {
      m.pixelLists[i] = makePixelList(W, H, block, rank * n + i, world * n, nullptr);
      m.recvPixels[i].upload(m.pixelLists[i]);
      m.recv[i].ensure(std::max<size_t>(m.pixelLists[i].size(), 1));
    }
    m.plW = W; m.plH = H; m.plTile = block; m.plRank = rank; m.plWorld = world;
  }
  // (a replica out of service contributes nothing here: its share is re-queued after the merge)
  auto count = [&](uint32_t i) -> size_t { return m.failed[i] ? 0 : m.scenes[i]->pixelsHost.size(); };
  // pack on every device i > 0 (its scene's own pixel list is on that device already)
  for (uint32_t i = 1; i < n; i++) {
    YartScene& s = *m.scenes[i];
    const uint32_t np = uint32_t(count(i));
    if (np == 0) continue;
    HIP_CHECK(hipSetDevice(m.devices[i]));
    m.slab[i].ensure(np);
    hipLaunchKernelGGL(k_pack_pixels, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, m.streams[i],
                       reinterpret_cast<const f4*>(s.hdr.p), s.pixels.p, np, W, m.slab[i].p);
    HIP_CHECK(hipGetLastError());
  }
  if (m.distinct && m.rcclBroken) throw RcclFailure("the RCCL communicators of this handle were aborted after an earlier failure");
  if (m.distinct) {
    // Everything that can fail for a reason of ours is checked BEFORE the group opens (devices can be made current, buffers and
    // counts are set): inside the group only RCCL itself can refuse a call. The group is closed on EVERY path: an exception
    // between ncclGroupStart and ncclGroupEnd would leave the group open on this thread and the next RCCL call would hang.
    const RcclApi& R = rccl();
    for (uint32_t i = 0; i < n; i++) HIP_CHECK(hipSetDevice(m.devices[i]));
    for (uint32_t i = 1; i < n; i++) require(count(i) == 0 || (m.slab[i].p && m.recv[i].p && m.comms[i] && m.comms[0]), "slab merge: a buffer or communicator is missing");
    auto abortAll = [&] { for (ncclComm_t& c : m.comms) if (c) { (void)R.CommAbort(c); c = nullptr; } };
    RCCL_CHECK(R.GroupStart());
    std::string failure;
    bool unmatchedSend = false;             // a send is queued whose receive was refused
    for (uint32_t i = 1; i < n && failure.empty(); i++) {
      const size_t cnt = count(i) * 4;
      if (cnt == 0) continue;
      (void)hipSetDevice(m.devices[i]);                                     // (each call on its communicator's device; checked above)
      ncclResult_t ne = R.Send(m.slab[i].p, cnt, ncclFloat, 0, m.comms[i], m.streams[i]);
      if (ne != ncclSuccess) { failure = std::string("ncclSend of slab ") + std::to_string(i) + ": " + R.GetErrorString(ne); break; }
      (void)hipSetDevice(m.devices[0]);
      ne = R.Recv(m.recv[i].p, cnt, ncclFloat, int(i), m.comms[0], m.streams[0]);
      if (ne != ncclSuccess) { failure = std::string("ncclRecv of slab ") + std::to_string(i) + ": " + R.GetErrorString(ne); unmatchedSend = true; }
    }
    if (!failure.empty()) {
      // The handle is unusable for the merge from here on (every later render on it fails with YART_E_RCCL) and the error is
      // reported now. How the group is left depends on what it holds (ADVICE r4: aborting communicators that still have
      // operations in an open group is not a documented sequence):
      //  * a refused SEND: every queued send has its receive — the group is closed first (its pairs complete), the communicators
      //    are aborted afterwards, outside any group;
      //  * a refused RECEIVE: the group holds a send without its receive; submitting it would wait for a peer that never posts
      //    (a hang instead of an error). The communicators are aborted first — their queued operations go with them — and the
      //    group is closed on what is left. tests/test_fake_rccl.py runs both orders against a stand-in library that logs them.
      if (unmatchedSend) { abortAll(); (void)R.GroupEnd(); }
      else { (void)R.GroupEnd(); abortAll(); }
      m.rcclBroken = true;
      throw RcclFailure(failure);
    }
    const ncclResult_t ge = R.GroupEnd();
    if (ge != ncclSuccess) {
      abortAll();                                                           // (the group is closed: a plain abort)
      m.rcclBroken = true;
      throw RcclFailure(std::string("ncclGroupEnd: ") + R.GetErrorString(ge));
    }
  } else {
    for (uint32_t i = 1; i < n; i++) {
      const size_t bytes = count(i) * sizeof(f4);
      if (bytes == 0) continue;
      HIP_CHECK(hipSetDevice(m.devices[i]));
      HIP_CHECK(hipStreamSynchronize(m.streams[i]));                      // the pack has finished
      HIP_CHECK(hipMemcpyPeerAsync(m.recv[i].p, m.devices[0], m.slab[i].p, m.devices[i], bytes, m.streams[0]));
    }
  }
  HIP_CHECK(hipSetDevice(m.devices[0]));
  for (uint32_t i = 1; i < n; i++) {
    const uint32_t np = m.failed[i] ? 0u : uint32_t(m.pixelLists[i].size());
    if (np == 0) continue;
    hipLaunchKernelGGL(k_unpack_pixels, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, m.streams[0],
                       reinterpret_cast<const f4*>(m.recv[i].p), m.recvPixels[i].p, np, W, reinterpret_cast<f4*>(m.scenes[0]->hdr.p));
    HIP_CHECK(hipGetLastError());
  }
  for (uint32_t i = 0; i < n; i++) {
    if (m.failed[i]) continue;
    HIP_CHECK(hipSetDevice(m.devices[i]));
    HIP_CHECK(hipStreamSynchronize(m.streams[i]));
  }
}

void renderMulti(YartMulti& m, const YartCameraDesc& cam, const YartRenderParams& p, float* out_rgba, YartStats* stats,
                 bool wantTileRays = false) {
  std::lock_guard<std::mutex> lock(m.mu);
  const uint32_t n = uint32_t(m.scenes.size());
  const uint32_t W = cam.width, H = cam.height;
  const size_t words = size_t(W) * H * 4;
  std::vector<YartStats> st(n);
  std::vector<std::exception_ptr> err(n);
  auto t0 = std::chrono::high_resolution_clock::now();
  // fault injection (tests): YART_FAULT_REPLICA = i makes replica i's render number YART_FAULT_AT (default 0, counted per handle)
  // fail as a device would: a HipError on its thread
  int faultReplica = -1; uint32_t faultAt = 0;
  if (const char* e = std::getenv("YART_FAULT_REPLICA")) faultReplica = std::atoi(e);
  if (const char* e = std::getenv("YART_FAULT_AT")) faultAt = uint32_t(std::max(0, std::atoi(e)));
  const uint32_t renderNo = m.rendersDone++;
  auto work = [&](uint32_t i) {
    try {
      if (m.failed[i]) return;                                            // out of service: its share is re-queued below
      YartScene& s = *m.scenes[i];
      std::lock_guard<std::mutex> sl(s.mu);
      HIP_CHECK(hipSetDevice(s.device));
      if (int(i) == faultReplica && renderNo == faultAt) throw HipError("injected device failure (YART_FAULT_REPLICA)");
      s.hdr.ensure(words);
      if (p.start_sample > 0) HIP_CHECK(hipMemcpy(s.hdr.p, out_rgba, words * sizeof(float), hipMemcpyHostToDevice));
      YartRenderParams q = p;
      q.rank = p.rank * n + i; q.world_size = p.world_size * n;           // device i of N of process rank r of R
      const BatchHook noop = [](const BatchInfo&) { return false; };      // with a hook the blocks' ray counts are summed (YartScene::tileRaysHost)
      renderToDevice(s, cam, q, s.hdr.p, m.streams[i], &st[i], wantTileRays ? &noop : nullptr);
    } catch (...) { err[i] = std::current_exception(); }
  };
  std::vector<std::thread> th;
  for (uint32_t i = 1; i < n; i++) th.emplace_back(work, i);
  work(0);
  for (auto& t : th) t.join();
  // A HIP error on a replica other than the first takes THAT device out of service; anything else (bad parameters: every replica
  // throws the same; a failure of devices[0], where the frame is merged) is the call's error as before.
  for (uint32_t i = 0; i < n; i++) {
    if (!err[i]) continue;
    bool deviceFailure = false; std::string what;
    try { std::rethrow_exception(err[i]); }
    catch (const HipError& e) { deviceFailure = true; what = e.what(); }
    catch (...) {}
    if (!deviceFailure || i == 0) std::rethrow_exception(err[i]);
    m.failed[i] = 1;
    m.failureNote = "replica " + std::to_string(i) + " (device " + std::to_string(m.devices[i]) + ") failed: " + what +
                    "; its pixel blocks are rendered on device " + std::to_string(m.devices[0]) + " from now on";
  }
  if (n > 1) mergeSlabs(m, W, H, p.shard_tile ? p.shard_tile : p.tile_size, p.rank, p.world_size);
  // re-queue: the shares of the replicas out of service, one after the other on devices[0] (its own share is merged already:
  // a share is rendered into a frame of its own and its pixels copied over)
  const std::vector<YartScene::TileRec> ownTiles = m.scenes[0]->tiles;          // (the tile callbacks read every replica's own blocks)
  const std::vector<unsigned long long> ownTileRays = m.scenes[0]->tileRaysHost;
  bool requeued = false;
  for (uint32_t i = 1; i < n; i++) {
    if (!m.failed[i]) continue;
    requeued = true;
    YartScene& s0 = *m.scenes[0];
    std::lock_guard<std::mutex> sl(s0.mu);
    HIP_CHECK(hipSetDevice(s0.device));
    m.requeueFrame.ensure(words);
    if (p.start_sample > 0) HIP_CHECK(hipMemcpy(m.requeueFrame.p, out_rgba, words * sizeof(float), hipMemcpyHostToDevice));
    YartRenderParams q = p;
    q.rank = p.rank * n + i; q.world_size = p.world_size * n;
    YartStats extra{};
    const BatchHook noop = [](const BatchInfo&) { return false; };
    renderToDevice(s0, cam, q, m.requeueFrame.p, m.streams[0], &extra, wantTileRays ? &noop : nullptr);
    const uint32_t np = uint32_t(s0.pixelsHost.size());                   // (the share's pixel list: renderToDevice has just built it)
    if (np) {
      hipLaunchKernelGGL(k_copy_pixels, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, m.streams[0],
                         reinterpret_cast<const f4*>(m.requeueFrame.p), s0.pixels.p, np, W, reinterpret_cast<f4*>(s0.hdr.p));
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(m.streams[0]));
    }
    m.scenes[i]->tiles = s0.tiles; m.scenes[i]->tileRaysHost = s0.tileRaysHost;   // the share's blocks and their ray counts
    st[i] = extra;
    st[0].ms_device += extra.ms_device;                                   // (devices[0] did both: the slowest device's time grows)
    st[i].ms_device = 0;
  }
  if (requeued) { m.scenes[0]->tiles = ownTiles; m.scenes[0]->tileRaysHost = ownTileRays; }
  HIP_CHECK(hipSetDevice(m.devices[0]));
  HIP_CHECK(hipMemcpy(out_rgba, m.scenes[0]->hdr.p, words * sizeof(float), hipMemcpyDeviceToHost));
  if (stats) {
    YartStats total{};
    for (uint32_t i = 0; i < n; i++) {
      total.samples += st[i].samples; total.rays += st[i].rays; total.traversals += st[i].traversals;
      total.box_tests += st[i].box_tests; total.tri_tests += st[i].tri_tests; total.shaded_hits += st[i].shaded_hits;
      total.ms_device = std::max(total.ms_device, st[i].ms_device);       // the slowest device sets the frame time
      total.ms_extend = std::max(total.ms_extend, st[i].ms_extend); total.ms_shade = std::max(total.ms_shade, st[i].ms_shade);
      total.ms_connect = std::max(total.ms_connect, st[i].ms_connect); total.ms_gmon = std::max(total.ms_gmon, st[i].ms_gmon);
      total.ms_traverse = std::max(total.ms_traverse, st[i].ms_traverse);
      total.waves = st[i].waves; total.pipeline_flags = st[i].pipeline_flags;
    }
    total.ms_total = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    *stats = total;
  }
}


// The wave schedule of tile-renderer.hpp:264-289 over all devices: every wave is rendered by all of them (each its own blocks),
// merged, copied out and reported — Renderer::onRenderWaveComplete fires whatever the number of workers (:243-282) — and, with
// on_tile, every block of the frame is reported once per wave, in Morton order, with its own ray count (finishTile, :200-262;
// the devices finish their blocks concurrently, so the reports follow the wave's merge).
int renderMultiProgressive(YartMulti& m, const YartCameraDesc& cam, const YartRenderParams& params, float* out_rgba, YartStats* stats,
                           YartWaveCallback on_wave, YartTileCallback on_tile, void* user) {
  bool aborted = false;
  auto t0 = std::chrono::high_resolution_clock::now();
  const uint32_t n = uint32_t(m.scenes.size());
  const uint32_t stop = params.stop_sample ? params.stop_sample : params.samples;
  YartStats total{};
  for (WaveSchedule ws(params.samples, params.first_wave_samples, params.max_wave_samples); !aborted && ws.next();) {
    const uint32_t taken = uint32_t(ws.takenBefore);
    const uint64_t wave = ws.wave, waveSamples = ws.samples;
    if (taken >= params.start_sample && taken < stop) {
      YartRenderParams q = params;
      q.start_sample = taken; q.stop_sample = uint32_t(taken + waveSamples);
      YartStats st{};
      auto tw = std::chrono::high_resolution_clock::now();
      renderMulti(m, cam, q, out_rgba, &st, on_tile != nullptr);
      total.rays += st.rays; total.samples += st.samples; total.waves += 1; total.ms_device += st.ms_device;
      total.ms_extend += st.ms_extend; total.ms_shade += st.ms_shade; total.ms_connect += st.ms_connect; total.ms_gmon += st.ms_gmon;
      total.ms_traverse += st.ms_traverse; total.pipeline_flags = st.pipeline_flags;
      if (on_tile) {
        // block k of the frame (Morton order) is block k / n of device k % n (makePixelList deals them round-robin)
        size_t nTiles = 0;
        for (uint32_t i = 0; i < n; i++) nTiles += m.scenes[i]->tiles.size();
        for (size_t k = 0; k < nTiles && !aborted; k++) {
          const YartScene& s = *m.scenes[k % n];
          const size_t local = k / n;
          if (local >= s.tiles.size()) continue;
          const YartScene::TileRec& t = s.tiles[local];
          YartTileInfo ti{};
          ti.x = t.x; ti.y = t.y; ti.width = t.w; ti.height = t.h;
          ti.index = uint32_t(k + 1); ti.total = uint32_t(nTiles);
          ti.wave = uint32_t(wave); ti.wave_samples = uint32_t(waveSamples); ti.samples_taken = uint32_t(taken + waveSamples);
          ti.total_samples = params.samples;
          ti.rays = local < s.tileRaysHost.size() ? s.tileRaysHost[local] : 0;
          ti.ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - tw).count();
          if (on_tile(user, &ti) != 0) aborted = true;
        }
      }
      st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
      if (!aborted && on_wave && on_wave(user, &st, uint32_t(wave), uint32_t(waveSamples), uint32_t(taken + waveSamples), params.samples) != 0)
        aborted = true;
    }
  }
  total.ms_total = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
  if (stats) *stats = total;
  return aborted ? YART_ABORTED : YART_OK;
}

}  // namespace
