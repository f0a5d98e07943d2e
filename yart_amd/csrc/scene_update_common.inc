// scene_update_common.inc — what the yart_hip_scene_update* entries share (included by yart_hip.hip, unit 0, before their four
// drivers). An entry is updateEntry over three functions of its own: the checks of its arguments, the checks against the scene,
// and the run; the run's frame is an UpdateCall. DESIGN §3 says what a new entry supplies.
namespace {

// An entry's check: refuses with the entry's prefix in front of the text.
struct UpdateCheck {
  const char* prefix;
  void operator()(bool ok, const std::string& what) const { if (!ok) throw std::invalid_argument(prefix + what); }
};

bool finiteWords(const float* m, size_t n) {
  for (size_t k = 0; k < n; k++) if (!std::isfinite(m[k])) return false;
  return true;
}

// The flags of YartSceneUpdate / YartSceneMeshUpdate: how the top-level hierarchy follows, at most one of the two rebuilds
void checkUpdateFlags(const UpdateCheck& check, uint32_t flags) {
  check((flags & ~(YART_UPDATE_REBUILD_TOP | YART_UPDATE_REBUILD_TOP_DEVICE)) == 0u, "unknown flags");
  check((flags & YART_UPDATE_REBUILD_TOP) == 0u || (flags & YART_UPDATE_REBUILD_TOP_DEVICE) == 0u,
        "flags: YART_UPDATE_REBUILD_TOP and YART_UPDATE_REBUILD_TOP_DEVICE exclude each other");
}

// YART_UPDATE_REBUILD_TOP_DEVICE is checked against the handle as well, behind the entry's other argument checks and before the
// handle is read: the flag is new, and callers that probed "unknown flags" with its value on a pointer that is no scene got an
// error return for it; they still do (SceneRegistry: the scenes that exist). Flags 0 and 1 take the handle as they always did.
void checkDeviceRebuildHandle(const UpdateCheck& check, uint32_t flags, const void* scene) {
  check((flags & YART_UPDATE_REBUILD_TOP_DEVICE) == 0u || SceneRegistry::get().has(scene),
        "flags: YART_UPDATE_REBUILD_TOP_DEVICE on a handle that is not a live scene of this library");
}

// The fields of a light that no update may change
bool sameLightTopology(const YartLightDesc& a, const YartLightDesc& b) {
  return a.type == b.type && a.mesh == b.mesh && a.tri == b.tri && a.two_sided == b.two_sided && a.texture == b.texture;
}

// The light rules of the entries that take new light transforms (yart_hip_scene_update, yart_hip_scene_update_graph): the count,
// then — behind the entry's checks of its nodes — every record
void checkLightCount(const UpdateCheck& check, const HostImage& h, uint32_t nLights, const YartLightDesc* lights) {
  check(nLights == 0u || nLights == h.nLights, "n_lights is neither 0 nor the scene's light count " + std::to_string(h.nLights));
  check(nLights == 0u || lights != nullptr, "lights pointer is null");
}
void checkLightTransforms(const UpdateCheck& check, const HostImage& h, uint32_t nLights, const YartLightDesc* lights) {
  for (uint32_t i = 0; i < nLights; i++) {
    const YartLightDesc& a = lights[i]; const YartLightDesc& b = h.lightDesc[i];
    check(sameLightTopology(a, b) && std::memcmp(&a.radius, &b.radius, 4) == 0 && std::memcmp(a.emission, b.emission, 12) == 0,
          "light " + std::to_string(i) + ": a field other than fwd / inv differs from the scene's");
    check(finiteWords(a.fwd, 16) && finiteWords(a.inv, 16), "light " + std::to_string(i) + ": a matrix word is not finite");
  }
}

// The update chain folds the meshes' vertex boxes; listed: the meshes whose box the update replaces (nullptr: none)
void checkMeshBoxes(const UpdateCheck& check, const HostImage& h, const uint8_t* listed) {
  for (size_t m = 0; m < h.meshBox.size(); m++)
    check((listed && listed[m]) || (finiteWords(h.meshBox[m].mn, 3) && finiteWords(h.meshBox[m].mx, 3)),
          "mesh " + std::to_string(m) + ": its vertex box is not finite (such a scene is re-created, not updated)");
}

// The host's re-derived lights to the device (rederiveLights / luRederiveLights have run)
void uploadLights(YartScene& s, hipStream_t stream) {
  const HostImage& h = s.host;
  s.dev.totalPower = h.totalPower;
  HIP_CHECK(hipMemcpyAsync(s.lights.p, h.lights.data(), h.lights.size() * sizeof(LightDev), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemcpyAsync(s.areaPowerCdf.p, h.areaPowerCdf.data(), h.areaPowerCdf.size() * sizeof(float), hipMemcpyHostToDevice, stream));
}

// The frame of one update on one stream: the device, the two events around the stream work, the launch count, the closing
// synchronisation and the stats. If the function that runs the update unwinds before finish(), the destructor waits for the stream:
// a copy that is still in flight then ends before the host arrays it reads or writes do — the caller's, and the function's own that
// are declared BEFORE the frame (they are destroyed after it).
using WallClock = std::chrono::high_resolution_clock;
class UpdateCall {
 public:
  const hipStream_t stream;
  // wall0: when the update began (ms_total counts from it; the opening event is recorded here, ms_device counts from that)
  UpdateCall(WallClock::time_point wall0, int device, hipStream_t st) : stream(st), wall0_(wall0) {
    HIP_CHECK(hipSetDevice(device));
    tm_.emplace();                                             // (the events are the device's: only now)
    HIP_CHECK(hipEventRecord(tm_->a, stream));
  }
  ~UpdateCall() { if (!finished_) (void)hipStreamSynchronize(stream); }
  UpdateCall(const UpdateCall&) = delete;
  // after every hipLaunchKernelGGL of the update, and never otherwise
  void launched() { HIP_CHECK(hipGetLastError()); launches_++; }
  // the launches of a callee that checks and counts its own (devbvh::buildCore)
  void launchedBy(uint32_t n) { launches_ += n; }
  // The closing event, and the stream synchronised. Again after further work: ms_device then ends behind that.
  void close() {
    HIP_CHECK(hipEventRecord(tm_->b, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  // The update has succeeded and close() has run: the stats, as many bytes of them as the caller's struct_size has room for
  void finish(YartSceneUpdateStats* stats) {
    finished_ = true;
    if (!stats) return;
    YartSceneUpdateStats out{};
    out.struct_size = stats->struct_size;
    out.launches = launches_;
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, tm_->a, tm_->b));
    out.ms_device = ms;
    out.ms_total = std::chrono::duration<double, std::milli>(WallClock::now() - wall0_).count();
    std::memcpy(stats, &out, std::min<size_t>(stats->struct_size, sizeof(out)));
  }

 private:
  const WallClock::time_point wall0_;
  std::optional<Timer> tm_;
  uint32_t launches_ = 0;
  bool finished_ = false;
};

// The checks every entry begins with. Returns the update copied into a struct of this build's size.
template <class Update>
Update updateHead(const UpdateCheck& check, const char* structName, const YartScene* scene, const Update* update) {
  check(scene != nullptr, "scene pointer is null");
  check(update != nullptr, "update pointer is null");
  check(update->struct_size >= sizeof(Update), std::string("struct_size is smaller than ") + structName);
  return *update;
}

// The body of an entry. Nothing of the scene is read before its lock is held, nothing is written and no device call is made before
// every check has passed; the order of the checks is part of the interface (the first that fails is the error reported).
//   checkArguments(u)                 the entry's own checks of the update, without a look at the scene
//   checkAgainstScene(scene, u)       what compares the update with the scene
//   run(scene, u, stream, stats)      owns an UpdateCall; returns synchronised, the stats written by finish()
template <class Update, class CheckArguments, class CheckAgainstScene, class Run>
int updateEntry(const UpdateCheck& check, const char* structName, YartScene* scene, const Update* update, void* stream, YartSceneUpdateStats* stats,
                CheckArguments&& checkArguments, CheckAgainstScene&& checkAgainstScene, Run&& run) {
  return guarded([&] {
    const Update u = updateHead(check, structName, scene, update);
    checkArguments(u);
    check(!stats || stats->struct_size >= 8u, "stats: struct_size is smaller than its first two fields");
    std::lock_guard<std::mutex> lock(scene->mu);
    checkAgainstScene(*scene, u);
    run(*scene, u, static_cast<hipStream_t>(stream), stats);
  });
}

}  // namespace
