// yart_hip.hpp — C++ host-side mirror of the reference's renderer interface over the C ABI.
//
// The reference's seam is `yart::Renderer` (reference src/core/renderer.hpp:17-104) as
// implemented by `yart::cpu::TileRenderer<Sampler, Integrator>`
// (src/cpu/tile-renderer.hpp:22-310): public knobs, `render()` (async), `abort()`,
// `wait()`, `renderSync()` returning `RenderData{buffer, samplesTaken, totalSamples,
// totalRays, totalTime}`. `yart::hip::HipTileRenderer` keeps those names, argument
// meanings and the "null scene -> empty render" behaviour (src/cpu/integrator.cpp:6), and
// adds what a device boundary needs: error codes become exceptions (`yart::hip::Error`).
//
// Header-only; link against libyart_hip.so. INTEGRATION.md shows the adapter that plugs
// this into the reference's `main()` / frontend in place of TileRenderer.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <exception>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "yart_hip.h"

namespace yart::hip {

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* msg) : std::runtime_error(std::string("yart_hip: ") + msg), code(c) {}
};
inline void check(int rc) { if (rc != YART_OK) throw Error(rc, yart_hip_last_error()); }
// the loaded library must speak the ABI these wrappers were compiled against (struct layouts, flag values)
inline void requireAbi() {
  if (yart_hip_abi_version() != YART_HIP_ABI_VERSION) throw Error(YART_E_INVALID, "libyart_hip.so and yart_hip.h disagree on YART_HIP_ABI_VERSION");
}

// Owns a device-resident scene (flattened geometry, BVHs, materials, lights).
// The frame and the first-hit feature buffers of one render (YartAovBuffers): only the requested ones are sized.
struct AovFrame {
  uint32_t width = 0, height = 0, mask = 0;
  std::vector<float> rgba, albedo, normal, position, depth, coverage;   // 4 / 3 / 3 / 3 / 1 / 1 floats per pixel
  std::vector<int32_t> ids;                                             // node, mesh, material, triangle of sample 0 (-1: miss)
  std::vector<uint32_t> rays;                                           // rays of the pixel over the whole render
};

// ... plus the per-pixel sample moments of the same render (YartMomentBuffers): only the requested ones are sized.
struct MomentFrame : AovFrame {
  uint32_t momentMask = 0;
  std::vector<float> mean, variance;                                    // 3 / 1 floats per pixel
  std::vector<uint32_t> count;                                          // accepted samples
};

class DeviceScene {
 public:
  explicit DeviceScene(const YartSceneDesc& desc, int device = -1) { requireAbi(); check(yart_hip_scene_create(&desc, device, &h_)); }
  explicit DeviceScene(const std::string& yscnPath, int device = -1) { requireAbi(); check(yart_hip_scene_load(yscnPath.c_str(), device, &h_)); }
  // a glTF 2.0 / GLB asset, as gltf::load + the frontend's environment light (src/gltf/gltf.cpp:319-358, src/main.cpp:78-86)
  static DeviceScene fromGltf(const std::string& path, const std::string& envHdrPath = "", float envRadius = 100.0f, int device = -1) {
    YartImportOptions o{};
    o.env_hdr_path = envHdrPath.empty() ? nullptr : envHdrPath.c_str();
    o.env_radius = envRadius;
    YartScene* h = nullptr;
    requireAbi();
    check(yart_hip_scene_load_gltf(path.c_str(), &o, device, &h));
    return DeviceScene(h);
  }
  DeviceScene(DeviceScene&& other) noexcept : h_(other.h_) { other.h_ = nullptr; }
  DeviceScene(const DeviceScene&) = delete;
  DeviceScene& operator=(const DeviceScene&) = delete;
  ~DeviceScene() { yart_hip_scene_destroy(h_); }
  YartScene* handle() const { return h_; }
  // How an update leaves the top-level hierarchy: its boxes refitted, or the tree rebuilt on the host (YART_UPDATE_REBUILD_TOP) or on
  // the device, on the update's stream (YART_UPDATE_REBUILD_TOP_DEVICE)
  enum class TopLevel : uint32_t { Refit = 0u, RebuildHost = YART_UPDATE_REBUILD_TOP, RebuildDevice = YART_UPDATE_REBUILD_TOP_DEVICE };
  // yart_hip_scene_update: new transforms for the scene's nodes (parent / mesh as at create) and, if any are given, its lights
  // (every other field as at create); rebuildTop: YART_UPDATE_REBUILD_TOP, or `top` for any of the three. Returns the update's statistics.
  YartSceneUpdateStats update(const std::vector<YartNodeDesc>& nodes, const std::vector<YartLightDesc>& lights = {}, bool rebuildTop = false,
                              void* stream = nullptr) {
    YartSceneUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_nodes = uint32_t(nodes.size()); u.nodes = nodes.data();
    u.n_lights = uint32_t(lights.size()); u.lights = lights.empty() ? nullptr : lights.data();
    u.flags = rebuildTop ? YART_UPDATE_REBUILD_TOP : 0u;
    return updateWith(yart_hip_scene_update, u, stream);
  }
  YartSceneUpdateStats update(const std::vector<YartNodeDesc>& nodes, const std::vector<YartLightDesc>& lights, TopLevel top, void* stream = nullptr) {
    YartSceneUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_nodes = uint32_t(nodes.size()); u.nodes = nodes.data();
    u.n_lights = uint32_t(lights.size()); u.lights = lights.empty() ? nullptr : lights.data();
    u.flags = uint32_t(top);
    return updateWith(yart_hip_scene_update, u, stream);
  }
  // yart_hip_scene_update_graph: a new node list for the scene (pre-order, node 0 the root; count, parents, mesh indices and
  // transforms may all differ from the scene's) and, if any are given, its lights' transforms. The top-level hierarchy is built on
  // the device (RebuildDevice, the default; Refit is the same: the leaf set changed, there is nothing to refit) or on the host
  // (RebuildHost). Discards the frame keepPrevious kept. Returns the update's statistics.
  YartSceneUpdateStats updateGraph(const std::vector<YartNodeDesc>& nodes, const std::vector<YartLightDesc>& lights = {},
                                   TopLevel top = TopLevel::RebuildDevice, void* stream = nullptr) {
    YartSceneGraphUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_nodes = uint32_t(nodes.size()); u.nodes = nodes.data();
    u.n_lights = uint32_t(lights.size()); u.lights = lights.empty() ? nullptr : lights.data();
    u.flags = uint32_t(top);
    return updateWith(yart_hip_scene_update_graph, u, stream);
  }
  // yart_hip_scene_update_meshes: new vertices for the listed meshes (each at most once; vertex counts as at create; normals /
  // tangents NULL: kept); rebuildTop: YART_UPDATE_REBUILD_TOP, or `top` as for update. Returns the update's statistics.
  YartSceneUpdateStats updateMeshes(const std::vector<YartMeshUpdate>& meshes, bool rebuildTop = false, void* stream = nullptr) {
    YartSceneMeshUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_meshes = uint32_t(meshes.size()); u.meshes = meshes.data();
    u.flags = rebuildTop ? YART_UPDATE_REBUILD_TOP : 0u;
    return updateWith(yart_hip_scene_update_meshes, u, stream);
  }
  YartSceneUpdateStats updateMeshes(const std::vector<YartMeshUpdate>& meshes, TopLevel top, void* stream = nullptr) {
    YartSceneMeshUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_meshes = uint32_t(meshes.size()); u.meshes = meshes.data();
    u.flags = uint32_t(top);
    return updateWith(yart_hip_scene_update_meshes, u, stream);
  }
  // yart_hip_scene_replace_meshes: whole new meshes (each at most once; positions, normals, tangents, uvs and faces as for create,
  // with counts of their own; no lights on the mesh); rebuildTop: YART_UPDATE_REBUILD_TOP, or `top` as for update. Discards the
  // frame keepPrevious kept. Returns the update's statistics.
  YartSceneUpdateStats replaceMeshes(const std::vector<YartMeshReplace>& meshes, bool rebuildTop = false, void* stream = nullptr) {
    YartSceneMeshReplace u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_meshes = uint32_t(meshes.size()); u.meshes = meshes.data();
    u.flags = rebuildTop ? YART_UPDATE_REBUILD_TOP : 0u;
    return updateWith(yart_hip_scene_replace_meshes, u, stream);
  }
  YartSceneUpdateStats replaceMeshes(const std::vector<YartMeshReplace>& meshes, TopLevel top, void* stream = nullptr) {
    YartSceneMeshReplace u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_meshes = uint32_t(meshes.size()); u.meshes = meshes.data();
    u.flags = uint32_t(top);
    return updateWith(yart_hip_scene_replace_meshes, u, stream);
  }
  // yart_hip_scene_update_lighting: new material values (empty: untouched; else every material of the scene), new light emission /
  // radius / transforms (empty: untouched; else every light) and new texels for the maps of image lights (each texture at most
  // once; the size as at create). Returns the update's statistics.
  YartSceneUpdateStats updateLighting(const std::vector<YartMaterialDesc>& materials, const std::vector<YartLightDesc>& lights,
                                      const std::vector<YartEnvImageUpdate>& images, void* stream = nullptr) {
    YartSceneLightingUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_materials = uint32_t(materials.size()); u.materials = materials.empty() ? nullptr : materials.data();
    u.n_lights = uint32_t(lights.size()); u.lights = lights.empty() ? nullptr : lights.data();
    u.n_images = uint32_t(images.size()); u.images = images.empty() ? nullptr : images.data();
    return updateWith(yart_hip_scene_update_lighting, u, stream);
  }
  // yart_hip_scene_update_textures: new texels for 8-bit material textures (each texture at most once; size and channels as at create;
  // YART_TEXELS_ON_DEVICE in an entry's flags: its pixels are memory of the scene's device). Returns the update's statistics.
  YartSceneUpdateStats updateTextures(const std::vector<YartTextureUpdate>& textures, void* stream = nullptr) {
    YartSceneTextureUpdate u{};
    u.struct_size = uint32_t(sizeof(u));
    u.n_textures = uint32_t(textures.size()); u.textures = textures.empty() ? nullptr : textures.data();
    return updateWith(yart_hip_scene_update_textures, u, stream);
  }
  // yart_hip_scene_keep_previous: the scene remembers the frame it holds as its previous frame; once per frame, before its updates
  void keepPrevious(void* stream = nullptr) { check(yart_hip_scene_keep_previous(h_, stream)); }
  // yart_hip_scene_pixel_motion_host: the per-pixel motion records (8 floats per pixel) between the kept frame and the scene as it
  // is now, from the host feature buffers (position, normal, coverage, ids) of a frame rendered from the scene as it is now
  std::vector<float> pixelMotion(const YartAovBuffers& aovs, uint32_t width, uint32_t height) {
    std::vector<float> records(size_t(width) * height * 8);
    check(yart_hip_scene_pixel_motion_host(h_, &aovs, width, height, records.data()));
    return records;
  }
  // yart_hip_render_aovs: the frame plus the feature buffers of `mask` (YART_AOV_*), from the same camera samples. Several GPUs:
  // one call per device with params.rank / world_size, then add the buffers (ids: by max).
  AovFrame renderAovs(const YartCameraDesc& cam, const YartRenderParams& params, uint32_t mask = YART_AOV_ALL, YartStats* stats = nullptr) {
    AovFrame f;
    f.width = cam.width; f.height = cam.height; f.mask = mask;
    const size_t n = size_t(cam.width) * cam.height;
    f.rgba.resize(n * 4);
    YartAovBuffers b{};
    b.struct_size = uint32_t(sizeof(b)); b.mask = mask;
    if (mask & YART_AOV_ALBEDO) { f.albedo.resize(n * 3); b.albedo = f.albedo.data(); }
    if (mask & YART_AOV_NORMAL) { f.normal.resize(n * 3); b.normal = f.normal.data(); }
    if (mask & YART_AOV_POSITION) { f.position.resize(n * 3); b.position = f.position.data(); }
    if (mask & YART_AOV_DEPTH) { f.depth.resize(n); b.depth = f.depth.data(); }
    if (mask & YART_AOV_COVERAGE) { f.coverage.resize(n); b.coverage = f.coverage.data(); }
    if (mask & YART_AOV_IDS) { f.ids.resize(n * 4); b.ids = f.ids.data(); }
    if (mask & YART_AOV_RAYS) { f.rays.resize(n); b.rays = f.rays.data(); }
    check(yart_hip_render_aovs(h_, &cam, &params, f.rgba.data(), &b, stats));
    return f;
  }
  // yart_hip_render_moments: renderAovs plus the sample moments of `momentMask` (YART_MOMENT_*) of the frame's own samples
  MomentFrame renderMoments(const YartCameraDesc& cam, const YartRenderParams& params, uint32_t momentMask = YART_MOMENT_ALL,
                            uint32_t aovMask = 0, YartStats* stats = nullptr) {
    MomentFrame f;
    f.width = cam.width; f.height = cam.height; f.mask = aovMask; f.momentMask = momentMask;
    const size_t n = size_t(cam.width) * cam.height;
    f.rgba.resize(n * 4);
    YartAovBuffers b{};
    b.struct_size = uint32_t(sizeof(b)); b.mask = aovMask;
    if (aovMask & YART_AOV_ALBEDO) { f.albedo.resize(n * 3); b.albedo = f.albedo.data(); }
    if (aovMask & YART_AOV_NORMAL) { f.normal.resize(n * 3); b.normal = f.normal.data(); }
    if (aovMask & YART_AOV_POSITION) { f.position.resize(n * 3); b.position = f.position.data(); }
    if (aovMask & YART_AOV_DEPTH) { f.depth.resize(n); b.depth = f.depth.data(); }
    if (aovMask & YART_AOV_COVERAGE) { f.coverage.resize(n); b.coverage = f.coverage.data(); }
    if (aovMask & YART_AOV_IDS) { f.ids.resize(n * 4); b.ids = f.ids.data(); }
    if (aovMask & YART_AOV_RAYS) { f.rays.resize(n); b.rays = f.rays.data(); }
    YartMomentBuffers m{};
    m.struct_size = uint32_t(sizeof(m)); m.mask = momentMask;
    if (momentMask & YART_MOMENT_MEAN) { f.mean.resize(n * 3); m.mean = f.mean.data(); }
    if (momentMask & YART_MOMENT_VARIANCE) { f.variance.resize(n); m.variance = f.variance.data(); }
    if (momentMask & YART_MOMENT_COUNT) { f.count.resize(n); m.count = f.count.data(); }
    check(yart_hip_render_moments(h_, &cam, &params, f.rgba.data(), &b, &m, stats));
    return f;
  }

 private:
  explicit DeviceScene(YartScene* h) : h_(h) {}
  // one of the yart_hip_scene_update* entries on this scene -> the update's statistics
  template <class Update>
  YartSceneUpdateStats updateWith(int (*entry)(YartScene*, const Update*, void*, YartSceneUpdateStats*), const Update& u, void* stream) {
    YartSceneUpdateStats st{};
    st.struct_size = uint32_t(sizeof(st));
    check(entry(h_, &u, stream, &st));
    return st;
  }
  YartScene* h_ = nullptr;
};

// RGBA32F framebuffer, row-major, alpha = 1 (reference src/core/buffer.hpp:12-47)
class Buffer {
 public:
  Buffer(uint32_t w, uint32_t h) : w_(w), h_(h), data_(size_t(w) * h * 4, 0.0f) {}
  uint32_t width() const { return w_; }
  uint32_t height() const { return h_; }
  const float* operator()(size_t x, size_t y) const { return &data_[(y * w_ + x) * 4]; }
  float* data() { return data_.data(); }
  const float* data() const { return data_.data(); }

 private:
  uint32_t w_, h_;
  std::vector<float> data_;
};

// The à-trous filter between renderAovs and the tonemap (yart_hip_denoise_atrous_host): host vectors in, the filtered frame out.
// An empty guide vector means that guide is not used.
struct DenoiseGuides { std::vector<float> albedo, normal, depth; };       // 3 / 3 / 1 floats per pixel
inline YartDenoiseParams denoiseDefaults(bool demodulate = false) {
  YartDenoiseParams p{};
  p.struct_size = uint32_t(sizeof(p)); p.iterations = YART_DENOISE_DEFAULT_ITERATIONS;
  p.sigma_color = YART_DENOISE_DEFAULT_SIGMA_COLOR; p.sigma_normal = YART_DENOISE_DEFAULT_SIGMA_NORMAL;
  p.sigma_depth = YART_DENOISE_DEFAULT_SIGMA_DEPTH; p.flags = demodulate ? YART_DENOISE_DEMODULATE : 0u;
  return p;
}
inline std::vector<float> denoise(const std::vector<float>& rgba, uint32_t width, uint32_t height, const DenoiseGuides& guides,
                                  const YartDenoiseParams& params) {
  const size_t n = size_t(width) * height;
  if (rgba.size() != n * 4 || (!guides.albedo.empty() && guides.albedo.size() != n * 3) ||
      (!guides.normal.empty() && guides.normal.size() != n * 3) || (!guides.depth.empty() && guides.depth.size() != n))
    throw Error(YART_E_INVALID, "denoise: a buffer does not have width * height * channels floats");
  std::vector<float> out(rgba.size());
  check(yart_hip_denoise_atrous_host(rgba.data(), guides.albedo.empty() ? nullptr : guides.albedo.data(),
                                     guides.normal.empty() ? nullptr : guides.normal.data(),
                                     guides.depth.empty() ? nullptr : guides.depth.data(), width, height, &params, out.data()));
  return out;
}

// The variance-guided form (yart_hip_denoise_atrous_var_host): `variance` is MomentFrame::variance of the same render.
inline YartDenoiseVarParams denoiseVarDefaults(bool demodulate = false) {
  YartDenoiseVarParams p{};
  p.struct_size = uint32_t(sizeof(p)); p.iterations = YART_DENOISE_VAR_DEFAULT_ITERATIONS;
  p.sigma_luma = YART_DENOISE_VAR_DEFAULT_SIGMA_LUMA; p.sigma_normal = YART_DENOISE_VAR_DEFAULT_SIGMA_NORMAL;
  p.sigma_depth = YART_DENOISE_VAR_DEFAULT_SIGMA_DEPTH; p.flags = demodulate ? YART_DENOISE_DEMODULATE : 0u;
  return p;
}
inline std::vector<float> denoiseVar(const std::vector<float>& rgba, const std::vector<float>& variance, uint32_t width, uint32_t height,
                                     const DenoiseGuides& guides, const YartDenoiseVarParams& params) {
  const size_t n = size_t(width) * height;
  if (rgba.size() != n * 4 || variance.size() != n || (!guides.albedo.empty() && guides.albedo.size() != n * 3) ||
      (!guides.normal.empty() && guides.normal.size() != n * 3) || (!guides.depth.empty() && guides.depth.size() != n))
    throw Error(YART_E_INVALID, "denoiseVar: a buffer does not have width * height * channels floats");
  std::vector<float> out(rgba.size());
  check(yart_hip_denoise_atrous_var_host(rgba.data(), variance.data(), guides.albedo.empty() ? nullptr : guides.albedo.data(),
                                         guides.normal.empty() ? nullptr : guides.normal.data(),
                                         guides.depth.empty() ? nullptr : guides.depth.data(), width, height, &params, out.data()));
  return out;
}

// Temporal accumulation with camera reprojection for a sequence of frames of one scene (yart_hip_temporal_*): the stage between a
// render with moments and denoiseVar. The handle holds the history (96 bytes per pixel on the device; 128 in the moments form) and
// the last camera. accumulateMoments is the moments form (yart_hip_temporal_accumulate_moments_host): the variance estimated from
// the accumulated luminance moments, and from the neighbourhood where the history is short; one form per handle between resets.
inline YartTemporalParams temporalDefaults(bool demodulate = false) {
  YartTemporalParams p{};
  p.struct_size = uint32_t(sizeof(p)); p.alpha_min = YART_TEMPORAL_DEFAULT_ALPHA_MIN; p.max_history = YART_TEMPORAL_DEFAULT_MAX_HISTORY;
  p.normal_cos_min = YART_TEMPORAL_DEFAULT_NORMAL_COS_MIN; p.plane_tolerance = YART_TEMPORAL_DEFAULT_PLANE_TOLERANCE;
  p.flags = demodulate ? YART_TEMPORAL_DEMODULATE : 0u;
  return p;
}
inline YartTemporalMomentParams temporalMomentDefaults(bool demodulate = false) {
  YartTemporalMomentParams p{};
  p.struct_size = uint32_t(sizeof(p)); p.alpha_min = YART_TEMPORAL_DEFAULT_ALPHA_MIN; p.max_history = YART_TEMPORAL_DEFAULT_MAX_HISTORY;
  p.normal_cos_min = YART_TEMPORAL_DEFAULT_NORMAL_COS_MIN; p.plane_tolerance = YART_TEMPORAL_DEFAULT_PLANE_TOLERANCE;
  p.min_moment_history = YART_TEMPORAL_DEFAULT_MIN_MOMENT_HISTORY;
  p.flags = demodulate ? YART_TEMPORAL_DEMODULATE : 0u;
  return p;
}
inline YartTemporalClip temporalClipDefaults() {
  YartTemporalClip c{};
  c.struct_size = uint32_t(sizeof(c)); c.radius = YART_TEMPORAL_DEFAULT_CLIP_RADIUS; c.gamma = YART_TEMPORAL_DEFAULT_CLIP_GAMMA;
  return c;
}
struct TemporalFeatures {                   // the frame's feature buffers: 3 / 3 / 1 / 1 / 4 (/ 3) values per pixel
  std::vector<float> position, normal, depth, coverage;
  std::vector<int32_t> ids;
  std::vector<float> albedo;                // only with YART_TEMPORAL_DEMODULATE
};
struct TemporalFrame { std::vector<float> rgba, variance; std::vector<uint32_t> length; };
class Temporal {
 public:
  Temporal(uint32_t width, uint32_t height, int device = 0) : m_width(width), m_height(height) {
    check(yart_hip_temporal_create(width, height, device, &m_handle));
  }
  ~Temporal() { yart_hip_temporal_destroy(m_handle); }
  Temporal(const Temporal&) = delete;
  Temporal& operator=(const Temporal&) = delete;
  Temporal(Temporal&& o) noexcept : m_handle(o.m_handle), m_width(o.m_width), m_height(o.m_height) { o.m_handle = nullptr; }

  void reset() { check(yart_hip_temporal_reset(m_handle)); }
  // per-node motion for the next accumulate call (yart_hip_temporal_set_motion): 24 floats per scene node; empty: clear a pending one
  void setMotion(const std::vector<float>& records) {
    if (records.empty()) { check(yart_hip_temporal_set_motion(m_handle, nullptr)); return; }
    if (records.size() % 24 != 0) throw Error(YART_E_INVALID, "Temporal::setMotion: records are not 24 floats per node");
    YartTemporalMotion m{};
    m.struct_size = uint32_t(sizeof(m)); m.n_nodes = uint32_t(records.size() / 24); m.records = records.data();
    check(yart_hip_temporal_set_motion(m_handle, &m));
  }
  // per-pixel motion for the next accumulate call (yart_hip_temporal_set_pixel_motion): 8 floats per pixel, in the address space
  // of the call that consumes them (host for accumulate / accumulateMoments), NOT copied: valid until that call returns; null: clear
  void setPixelMotion(const float* records) {
    if (!records) { check(yart_hip_temporal_set_pixel_motion(m_handle, nullptr)); return; }
    YartTemporalPixelMotion m{};
    m.struct_size = uint32_t(sizeof(m)); m.records = records;
    check(yart_hip_temporal_set_pixel_motion(m_handle, &m));
  }
  // the clip of the history to the frame's neighbourhood (yart_hip_temporal_set_clip): it stays set, across reset too, until it is
  // set again; null: off
  void setClip(const YartTemporalClip* clip) { check(yart_hip_temporal_set_clip(m_handle, clip)); }
  void setClip(const YartTemporalClip& clip) { setClip(&clip); }
  // one frame, host buffers: the accumulated frame, its variance and the history length per pixel
  TemporalFrame accumulate(const YartCameraDesc& camera, const std::vector<float>& rgba, const std::vector<float>& variance,
                           const TemporalFeatures& f, const YartTemporalParams& params) {
    return run(yart_hip_temporal_accumulate_host, camera, rgba, variance, f, params);
  }
  // the same in the moments form
  TemporalFrame accumulateMoments(const YartCameraDesc& camera, const std::vector<float>& rgba, const std::vector<float>& variance,
                                  const TemporalFeatures& f, const YartTemporalMomentParams& params) {
    return run(yart_hip_temporal_accumulate_moments_host, camera, rgba, variance, f, params);
  }
  YartTemporal* handle() const { return m_handle; }

 private:
  template <class Fn, class Params>
  TemporalFrame run(Fn fn, const YartCameraDesc& camera, const std::vector<float>& rgba, const std::vector<float>& variance,
                    const TemporalFeatures& f, const Params& params) {
    const size_t n = size_t(m_width) * m_height;
    if (rgba.size() != n * 4 || variance.size() != n || f.position.size() != n * 3 || f.normal.size() != n * 3 || f.depth.size() != n ||
        f.coverage.size() != n || f.ids.size() != n * 4 || (!f.albedo.empty() && f.albedo.size() != n * 3))
      throw Error(YART_E_INVALID, "Temporal::accumulate: a buffer does not have width * height * channels values");
    YartAovBuffers a{};
    a.struct_size = uint32_t(sizeof(a));
    a.mask = YART_AOV_POSITION | YART_AOV_NORMAL | YART_AOV_DEPTH | YART_AOV_COVERAGE | YART_AOV_IDS | (f.albedo.empty() ? 0u : YART_AOV_ALBEDO);
    a.position = const_cast<float*>(f.position.data()); a.normal = const_cast<float*>(f.normal.data());
    a.depth = const_cast<float*>(f.depth.data()); a.coverage = const_cast<float*>(f.coverage.data());
    a.ids = const_cast<int32_t*>(f.ids.data()); a.albedo = f.albedo.empty() ? nullptr : const_cast<float*>(f.albedo.data());
    TemporalFrame out{std::vector<float>(n * 4), std::vector<float>(n), std::vector<uint32_t>(n)};
    check(fn(m_handle, &camera, rgba.data(), variance.data(), &a, &params, out.rgba.data(), out.variance.data(), out.length.data()));
    return out;
  }
  YartTemporal* m_handle = nullptr;
  uint32_t m_width, m_height;
};

// Auto-exposure for a sequence of frames (yart_hip_exposure_*), the stage after the denoiser: meter builds a log-luminance
// histogram of a linear-HDR frame on the device and steps the exposure by dt seconds; apply multiplies by the gain, tonemaps
// (AgX; look -1: none) and encodes to 8 bits in one kernel. The state stays on the device.
inline YartExposureParams exposureDefaults() {
  YartExposureParams p{};
  p.struct_size = uint32_t(sizeof(p)); p.ev_min = YART_EXPOSURE_DEFAULT_EV_MIN; p.ev_max = YART_EXPOSURE_DEFAULT_EV_MAX;
  p.trim_low = YART_EXPOSURE_DEFAULT_TRIM_LOW; p.trim_high = YART_EXPOSURE_DEFAULT_TRIM_HIGH; p.key = YART_EXPOSURE_DEFAULT_KEY;
  p.compensation_ev = YART_EXPOSURE_DEFAULT_COMPENSATION_EV; p.gain_ev_min = YART_EXPOSURE_DEFAULT_GAIN_EV_MIN;
  p.gain_ev_max = YART_EXPOSURE_DEFAULT_GAIN_EV_MAX; p.speed_up = YART_EXPOSURE_DEFAULT_SPEED_UP; p.speed_down = YART_EXPOSURE_DEFAULT_SPEED_DOWN;
  return p;                                 // x0 = y0 = x1 = y1 = 0: the whole frame
}
struct ExposedFrame { std::vector<float> ldr; std::vector<uint8_t> rgb8; };
class Exposure {
 public:
  explicit Exposure(int device = 0) { check(yart_hip_exposure_create(device, &m_handle)); }
  ~Exposure() { yart_hip_exposure_destroy(m_handle); }
  Exposure(const Exposure&) = delete;
  Exposure& operator=(const Exposure&) = delete;
  Exposure(Exposure&& o) noexcept : m_handle(o.m_handle) { o.m_handle = nullptr; }

  void reset() { check(yart_hip_exposure_reset(m_handle)); }
  // one frame, host buffer (width * height * 4 floats); dt: seconds since the previous frame
  YartExposureState meter(const std::vector<float>& rgba, uint32_t width, uint32_t height, const YartExposureParams& params, float dt) {
    if (rgba.size() != size_t(width) * height * 4) throw Error(YART_E_INVALID, "Exposure::meter: the frame does not have width * height * 4 values");
    check(yart_hip_exposure_meter_host(m_handle, rgba.data(), width, height, &params, dt));
    return state();
  }
  ExposedFrame apply(const std::vector<float>& rgba, uint32_t width, uint32_t height, int look) {
    const size_t n = size_t(width) * height;
    if (rgba.size() != n * 4) throw Error(YART_E_INVALID, "Exposure::apply: the frame does not have width * height * 4 values");
    ExposedFrame out{std::vector<float>(n * 4), std::vector<uint8_t>(n * 3)};
    check(yart_hip_exposure_apply_host(m_handle, rgba.data(), width, height, look, out.ldr.data(), out.rgb8.data()));
    return out;
  }
  // the state record; histogram (may be null): the 256 bins of the last meter call
  YartExposureState state(std::vector<uint32_t>* histogram = nullptr) {
    YartExposureState s{};
    s.struct_size = uint32_t(sizeof(s));
    if (histogram) histogram->assign(YART_EXPOSURE_BINS, 0u);
    check(yart_hip_exposure_get(m_handle, &s, histogram ? histogram->data() : nullptr));
    return s;
  }
  YartExposure* handle() const { return m_handle; }

 private:
  YartExposure* m_handle = nullptr;
};

// The scene replicated on several GPUs of this node (yart_hip_multi_*): TileRenderer's worker pool with a GPU per worker.
class MultiDeviceScene {
 public:
  MultiDeviceScene(const std::string& path, const std::vector<int>& devices, const std::string& envHdrPath = "", float envRadius = 100.0f) {
    YartImportOptions o{};
    o.env_hdr_path = envHdrPath.empty() ? nullptr : envHdrPath.c_str();
    o.env_radius = envRadius;
    check(yart_hip_multi_load(path.c_str(), &o, devices.data(), uint32_t(devices.size()), &h_));
  }
  MultiDeviceScene(const YartSceneDesc& desc, const std::vector<int>& devices) {
    check(yart_hip_multi_create(&desc, devices.data(), uint32_t(devices.size()), &h_));
  }
  MultiDeviceScene(const MultiDeviceScene&) = delete;
  MultiDeviceScene& operator=(const MultiDeviceScene&) = delete;
  ~MultiDeviceScene() { yart_hip_multi_destroy(h_); }
  YartMulti* handle() const { return h_; }
  int deviceCount() const { return yart_hip_multi_device_count(h_); }
  // replicas a device failure took out of service (their pixel blocks are rendered on the first device from then on); empty normally
  std::vector<int> failedReplicas() const {
    std::vector<int> out(64);
    const int n = yart_hip_multi_failed_devices(h_, out.data(), uint32_t(out.size()));
    out.resize(size_t(n < 64 ? n : 64));
    return out;
  }

 private:
  YartMulti* h_ = nullptr;
};

class HipTileRenderer {
 public:
  struct RenderData {                       // renderer.hpp:22-28
    const Buffer& buffer;
    size_t samplesTaken, totalSamples;
    uint64_t totalRays;
    std::chrono::milliseconds totalTime;
  };
  struct WaveData {                         // renderer.hpp:33-38
    size_t wave, waveSamples;
    uint64_t rays;
    std::chrono::milliseconds time;
  };
  struct TileData {                         // renderer.hpp:40-50 (rays: 0, the device counts rays per wave)
    uint32_t offset[2], size[2];
    size_t index, total;
    uint64_t rays;
    std::chrono::milliseconds time;
  };
  template <class... Ts> using RenderCallback = std::optional<std::function<void(Ts...)>>;

  // knobs of TileRenderer (tile-renderer.hpp:27-32) and Renderer (renderer.hpp:52-58)
  uint32_t samples = 64, firstWaveSamples = 64, maxWaveSamples = 128, tileSize = 64;
  uint32_t maxDepth = 30;                   // RayIntegrator::m_maxDepth (ray-integrator.hpp:14)
  float backgroundColor[3] = {0, 0, 0};
  uint32_t estimator = YART_ESTIMATOR_GMON; // core/estimator.hpp class (integrator.cpp:17-18 fixes it at compile time)
  int tonemapLook = -1;                     // TileRenderer::tonemapper: -1 none (linear HDR), 0 AgX none, 1 golden, 2 punchy
  uint32_t maxBatchPaths = 0;               // YartRenderParams.max_batch_paths: how many tiles finish together (0: a whole wave)
  const DeviceScene* scene = nullptr;
  const MultiDeviceScene* multiScene = nullptr;   // if set: all its devices render every wave of the frame (same callbacks)
  RenderCallback<RenderData> onRenderComplete, onRenderAborted;
  RenderCallback<RenderData, WaveData> onRenderWaveComplete;
  RenderCallback<RenderData, TileData> onRenderTileComplete;

  HipTileRenderer(Buffer&& buffer, const YartCameraDesc& camera) : camera_(camera), buffer_(std::move(buffer)) {
    camera_.width = buffer_.width(); camera_.height = buffer_.height();
  }
  ~HipTileRenderer() { if (worker_.joinable()) worker_.join(); }

  void render() {                           // async, notifies through the callbacks
    wait();
    aborted_ = false;
    failure_ = nullptr;
    worker_ = std::thread([this] {
      // an exception must not leave the thread function (std::terminate): it is kept and rethrown by wait(), and the
      // caller is told through onRenderAborted
      try {
        RenderData d = renderSync();
        auto& cb = aborted_ ? onRenderAborted : onRenderComplete;
        if (cb) (*cb)(d);
      } catch (...) {
        failure_ = std::current_exception();
        if (onRenderAborted) (*onRenderAborted)(RenderData{buffer_, taken_, samples, rays_, elapsed()});
      }
    });
  }
  void abort() { aborted_ = true; }         // takes effect after the batch in flight (a wave, or max_batch_paths of it)
  void wait() {                             // joins; rethrows what the render thread failed with
    if (worker_.joinable()) worker_.join();
    if (failure_) { auto e = failure_; failure_ = nullptr; std::rethrow_exception(e); }
  }

  RenderData renderSync() {
    t0_ = std::chrono::high_resolution_clock::now();
    taken_ = 0; rays_ = 0;
    YartStats st{};
    if (scene || multiScene) {              // integrator.cpp:6: "if (!scene) return;"
      YartRenderParams p{};
      p.samples = samples; p.first_wave_samples = firstWaveSamples < samples ? firstWaveSamples : samples;
      p.max_wave_samples = maxWaveSamples; p.tile_size = tileSize; p.max_depth = maxDepth;
      for (int i = 0; i < 3; i++) p.background[i] = backgroundColor[i];
      p.rank = 0; p.world_size = 1;
      p.estimator = estimator;
      p.max_batch_paths = maxBatchPaths;
      int rc;
      if (multiScene) {
        rc = yart_hip_multi_render_tiles(multiScene->handle(), &camera_, &p, buffer_.data(), &st, &HipTileRenderer::onWave,
                                         onRenderTileComplete ? &HipTileRenderer::onTile : nullptr, this);
      } else if (onRenderTileComplete) {
        rc = yart_hip_render_tiles(scene->handle(), &camera_, &p, buffer_.data(), &st, &HipTileRenderer::onWave, &HipTileRenderer::onTile, this);
      } else {
        rc = yart_hip_render_waves(scene->handle(), &camera_, &p, buffer_.data(), &st, &HipTileRenderer::onWave, this);
      }
      if (rc != YART_ABORTED) check(rc);
      if (tonemapLook >= 0)                   // tile-renderer.hpp:234-239, on the whole frame
        check(yart_hip_tonemap_host(buffer_.data(), buffer_.width(), buffer_.height(), tonemapLook, buffer_.data(), nullptr));
    }
    stats_ = st;
    return {buffer_, (scene || multiScene) ? taken_ : 0, samples, rays_, elapsed()};
  }
  const YartStats& stats() const { return stats_; }

 private:
  // per wave: the linear frame blended so far is in buffer_ (renderer.hpp:33-38); abort() stops after this wave.
  // RenderData.totalRays is cumulative, as the reference's m_totalRays (tile-renderer.hpp:213-214)
  static int onWave(void* user, const YartStats* st, uint32_t wave, uint32_t waveSamples, uint32_t taken, uint32_t total) {
    HipTileRenderer& r = *static_cast<HipTileRenderer*>(user);
    r.taken_ = taken; r.rays_ += st->rays;
    if (r.onRenderWaveComplete)
      (*r.onRenderWaveComplete)(RenderData{r.buffer_, taken, total, r.rays_, r.elapsed()},
                                WaveData{wave, waveSamples, st->rays, std::chrono::milliseconds(int64_t(st->ms_device))});
    return r.aborted_ ? 1 : 0;
  }
  static int onTile(void* user, const YartTileInfo* t) {
    HipTileRenderer& r = *static_cast<HipTileRenderer*>(user);
    if (r.onRenderTileComplete)
      (*r.onRenderTileComplete)(RenderData{r.buffer_, size_t(t->samples_taken - t->wave_samples), t->total_samples, r.rays_, r.elapsed()},
                                TileData{{t->x, t->y}, {t->width, t->height}, t->index, t->total, t->rays,
                                         std::chrono::milliseconds(int64_t(t->ms))});
    return r.aborted_ ? 1 : 0;
  }
  std::chrono::milliseconds elapsed() const {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::high_resolution_clock::now() - t0_);
  }
  size_t taken_ = 0;
  uint64_t rays_ = 0;
  std::chrono::high_resolution_clock::time_point t0_;
  YartCameraDesc camera_;
  Buffer buffer_;
  std::thread worker_;
  std::atomic<bool> aborted_{false};
  std::exception_ptr failure_;
  YartStats stats_{};
};

}  // namespace yart::hip
