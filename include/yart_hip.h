/* yart_hip.h — C ABI of the MI355X-native path-tracing integrator (libyart_hip.so).
 *
 * The reference (teofum/yart) has no plugin / FFI layer: its seam is the abstract
 * C++ class yart::Renderer (reference src/core/renderer.hpp:17-104) implemented by
 * yart::cpu::TileRenderer (src/cpu/tile-renderer.hpp:22-310). This header is what
 * a binding for that seam calls: plain C, POD structs, caller-owned buffers, no
 * C++/torch types. INTEGRATION.md shows the adapter class a maintainer of the
 * reference would add on top of it.
 *
 * Every entry point returns 0 on success or a negative YART_E_* code;
 * yart_hip_last_error() gives the message. There is NO CPU fallback: without a
 * HIP device every compute entry point fails with YART_E_NO_DEVICE.
 */
#ifndef YART_HIP_H
#define YART_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YART_HIP_ABI_VERSION 3

enum {
  YART_OK = 0,
  YART_E_INVALID = -1,    /* bad descriptor (null pointer, index out of range, ...) */
  YART_E_NO_DEVICE = -2,  /* no usable HIP device */
  YART_E_HIP = -3,        /* a HIP runtime call failed */
  YART_E_IO = -4,         /* scene file could not be read */
  YART_E_RCCL = -5,       /* an RCCL call of the multi-device merge failed */
  YART_ABORTED = 1        /* yart_hip_render_waves: the wave callback asked to stop (the frame holds the waves done) */
};

/* Texture as the reference holds it after load (src/core/texture.hpp:21-49):
 * u8 with 1-4 channels or float RGB; sRGB-typed data is gamma-2 encoded
 * (texture.hpp:78-84). type: 0 LinearRGB, 1 sRGB, 2 NonColor. */
typedef struct YartTextureDesc {
  uint32_t width, height, channels, is_float, type;
  const void* data;
} YartTextureDesc;

/* Constructor arguments of ParametricBSDF (src/bsdf/parametric.hpp:16-37);
 * tex_* are indices into YartSceneDesc.textures or -1. */
typedef struct YartMaterialDesc {
  float base[3];
  float emission[3];
  float metallic, roughness, transmission, ior;
  float anisotropic, aniso_rotation, clearcoat, clearcoat_roughness;
  float normal_scale;
  uint32_t thin_transmission;
  float volume_color[3];
  float volume_density;
  int32_t tex_base, tex_mr, tex_transmission, tex_normal, tex_clearcoat, tex_emission;
} YartMaterialDesc;

/* Arguments of Mesh(vertices, vertexData, faces) (src/core/mesh.hpp:54-61) plus the
 * per-triangle light index the loader assigns (src/gltf/gltf.cpp:299-309). */
typedef struct YartMeshDesc {
  uint32_t n_vertices, n_faces;
  const float* positions;   /* 3 per vertex */
  const float* normals;     /* 3 per vertex */
  const float* tangents;    /* 4 per vertex (xyz + handedness) */
  const float* uvs;         /* 2 per vertex */
  const uint32_t* faces;    /* 4 per face: i0, i1, i2, material */
  const int32_t* face_light;/* 1 per face: light index or -1 */
} YartMeshDesc;

/* Scene-graph node (src/core/scene.hpp:11-64), pre-order (a node's parent comes before it), node 0 = root.
 * fwd / inv: row-major 4x4 Transform matrices (src/math/transform.hpp).
 * There is no nesting limit (the reference's testNode recurses to any depth); a scene holds fewer than 2^20 nodes.
 * The glTF import instances a node shared by several parents once per path and refuses a cycle (YART_E_IO). */
typedef struct YartNodeDesc {
  int32_t parent, mesh;
  float fwd[16], inv[16];
} YartNodeDesc;

/* Light (src/core/light.hpp): type 0 AreaLight(tri of mesh, emission, transform),
 * 1 UniformInfiniteLight(radius, emission), 2 ImageInfiniteLight(radius, float RGB
 * octahedral texture) with its public `transform`. */
typedef struct YartLightDesc {
  uint32_t type;
  int32_t mesh;
  uint32_t tri, two_sided;
  int32_t texture;
  float radius;
  float emission[3];
  float fwd[16], inv[16];
} YartLightDesc;

typedef struct YartSceneDesc {
  uint32_t n_textures, n_materials, n_meshes, n_nodes, n_lights;
  const YartTextureDesc* textures;
  const YartMaterialDesc* materials;
  const YartMeshDesc* meshes;
  const YartNodeDesc* nodes;
  const YartLightDesc* lights;
} YartSceneDesc;

/* Camera(imageSize, focalLength, fNumber, sensorSize) + moveAndLookAt + exposure /
 * apertureSides (src/core/camera.hpp:62-130). */
typedef struct YartCameraDesc {
  uint32_t width, height;
  float focal_length, f_number;
  float sensor[2];
  float position[3], target[3], up[3];
  float exposure;
  uint32_t aperture_sides;
} YartCameraDesc;

/* TileRenderer knobs (src/cpu/tile-renderer.hpp:27-32), Renderer::backgroundColor
 * (src/core/renderer.hpp:52), RayIntegrator::m_maxDepth (src/cpu/ray-integrator.hpp:14).
 * rank/world_size: this process renders the pixel blocks b with b % world_size == rank (blocks of shard_tile,
 * by default tile_size, pixels numbered in Morton order) and leaves the other pixels 0. */
typedef struct YartRenderParams {
  uint32_t samples, first_wave_samples, max_wave_samples, tile_size, max_depth;
  float background[3];
  uint32_t rank, world_size;
  uint32_t flags;            /* YART_FLAG_* */
  /* Resumable accumulation (the reference keeps its blended m_hdrBuffer between waves, tile-renderer.hpp:93,
   * 220-232): render only the waves that cover samples [start_sample, stop_sample) of the schedule that
   * `samples / first_wave_samples / max_wave_samples` define; both must lie on wave boundaries of that
   * schedule (stop_sample 0 = samples). With start_sample > 0 the output buffer must hold the frame
   * accumulated so far and is blended into, exactly as an uninterrupted render would continue. */
  uint32_t start_sample, stop_sample;
  /* Per-pixel estimator (core/estimator.hpp): the reference's Integrator::render picks one at compile time
   * (cpu/integrator.cpp:17-18: GMoNEstimator(samples, 15) as shipped, MeanEstimator in the commented line);
   * MoN and GMoNb take the same (samples, 15). 0 keeps the shipped behaviour. */
  uint32_t estimator;        /* YART_ESTIMATOR_* */
  /* Edge of the square pixel blocks dealt to the ranks (Morton order, round-robin); 0 = tile_size, the
   * reference's unit of parallel work. Which process renders a pixel does not change it (the sampler only
   * knows tile_size), so a smaller block only evens out the load between GPUs. */
  uint32_t shard_tile;
  /* Upper bound on the (pixel, sample) paths per batch; 0 = 2^28 (a fixed number: the memory a render holds does not depend on
   * what happens to be free on the device; only a device that cannot hold the batch renders smaller ones). A wave is rendered
   * batch by batch over this rank's pixels in tile order, every batch through all bounces and the estimator: 251 bytes per path
   * of the batch (path state, queues, per-sample radiance, the compacted state of the late bounces; feature buffers, YartAovBuffers
   * below, add nothing to it in this pipeline and 48 bytes per path under YART_FLAG_MEGAKERNEL / YART_FLAG_PATH_POOL). A smaller batch means
   * finished tiles arrive earlier (yart_hip_render_tiles) and less memory is held, at ~10 ms per batch on an MI355X (the C3 frame
   * of 531 M paths: +1.4 % in 2 batches, +4.5 % in 4, +19 % in 16). The frame does not depend on it. */
  uint32_t max_batch_paths;
  /* ABI 3. With YART_FLAG_PATH_POOL: the path slots of the pool (0 = 2^25: 5.6 GB). The paths of a batch are started in these
   * slots, and whenever a path ends its slot takes the batch's next (pixel, sample) — path regeneration, as a worker of the
   * reference takes the next tile the moment it has finished one (tile-renderer.hpp:161-167) — so the path state is bounded
   * by the pool (168 bytes per slot) and only 16 bytes per path of the batch remain. The frame does not depend on it. */
  uint32_t pool_paths;
} YartRenderParams;
#define YART_ESTIMATOR_GMON 0u      /* core/estimator.hpp:148-198 */
#define YART_ESTIMATOR_MEAN 1u      /* :29-46 */
#define YART_ESTIMATOR_MON 2u       /* :53-92 */
#define YART_ESTIMATOR_GMONB 3u     /* :94-146 */

#define YART_FLAG_MEGAKERNEL 1u     /* single-kernel integrator instead of the wavefront pipeline */
#define YART_FLAG_NO_REFILL 16u     /* one-ray-per-lane lean kernels instead of the ones with in-wave ray
                                       replacement (csrc/trace_lean.hpp: traceLean) */
#define YART_FLAG_SHADE_SORT 2u     /* bucket each wave's 256 shade-queue entries by lobe class before shading them: the default
                                       since round 2 (measured: shade stage -8.4 % on the McLaren-class scene, -0.5 % on the
                                       Sponza-class one; round 1 bucketed by material index and lost 5 % there) */
#define YART_FLAG_NO_SHADE_SORT 64u /* shade the queue entries in queue order */
#define YART_FLAG_DIRECT_SAMPLER 8u /* evaluate every ZSobol index digit per draw (no per-render sampler tables) */
#define YART_FLAG_NO_COMPACTION 32u  /* keep every bounce on the batch-sized path state (no copy of the survivors into a dense one) */
#define YART_FLAG_NO_RESUME 128u    /* rays the lean traversal kernels hand to the general ones are traced again from the root instead of
                                       being taken up where the lean kernel stood (the default; same frame either way) */
#define YART_FLAG_GENERAL_TRACE 4u  /* general traversal kernels for every ray instead of lean kernels + retry */
/* value 256 (YART_FLAG_WIDE_TREES of rounds 4-5: 8-wide trees of the lean kernels' own, walked one ray per lane, then by eight lanes per
   ray) is retired and ignored: both forms were bit-identical and slower than the walk of the reference's tree
   (profiles/r4_ab_lean_tree.txt, profiles/r5_ab_coop_tree.txt) */
#define YART_FLAG_PATH_POOL 512u    /* ABI 3: run a batch through a pool of pool_paths path slots with path regeneration (a slot whose path has ended
                                       takes the batch's next path) instead of one slot per path of the batch. Same frame either way */
/* ABI history. 3: YART_FLAG_PATH_POOL (and the since-retired value 256); YartStats grew (wide_* fields at the end, now always 0); value 128 has meant NO_RESUME since the end of
 * ABI 2 (it selected a since-removed 4-wide re-layout before: an old client passing it gets the same frame, a little slower);
 * YartRenderParams grew (pool_paths); max_batch_paths = 0 now means a fixed 2^28 paths, no longer a share of the free device memory; value 1024 is retired and ignored; YartTileInfo.rays is a real count; yart_hip_multi_render_tiles was added.
 * Added to ABI 3 without a bump (new exports and structs only, no existing layout changed): yart_hip_scene_replace_meshes with
 * YartMeshReplace / YartSceneMeshReplace, yart_hip_probe_geometry with YartGeometryProbe. */

/* Renderer::RenderData counters (src/core/renderer.hpp:22-28) + per-stage device time. */
typedef struct YartStats {
  uint64_t samples;          /* pixel samples taken by this rank */
  uint64_t rays;             /* path segments + unoccluded shadow rays (mis-integrator.cpp:22,126) */
  double ms_total;           /* wall time of the call */
  double ms_device;          /* HIP-event time of all kernels */
  double ms_traverse;        /* HIP-event time of the traversal kernels (wavefront: extend + connect;
                                megakernel: the whole path kernel) */
  uint64_t traversals;       /* rays traced (closest-hit + shadow) */
  uint64_t box_tests, tri_tests;   /* exact counts when collected (instrumented build), else 0 */
  uint32_t waves;            /* progressive waves rendered */
  uint32_t launches_traverse;      /* launches summed into ms_traverse */
  uint64_t shaded_hits;      /* instrumented build only */
  double ms_extend, ms_shade, ms_connect, ms_gmon;   /* per-stage HIP-event time (wavefront pipeline) */
  uint32_t launches_extend, launches_connect;
  /* the lean closest-hit kernel (k_wf_extend_fast) alone: HIP-event time, launches, and its share
     of the exact test counters (instrumented build) — the roofline kernel of bench.py */
  double ms_extend_lean;
  uint64_t lean_traversals, lean_box_tests, lean_tri_tests;
  uint32_t launches_extend_lean, reserved0;
  /* the shade kernel (k_wf_shade) and the lean any-hit kernel (k_wf_shadow_lean) alone, as above */
  double ms_shade_kernel, ms_shadow_lean;
  uint32_t launches_shade_kernel, launches_shadow_lean;
  uint64_t shadow_lean_traversals, shadow_lean_box_tests, shadow_lean_tri_tests;
  uint64_t shade_entries;      /* instrumented build: queue entries the shade kernel processed (hits + misses) */
  uint64_t texture_tap_bytes;  /* instrumented build: 4 taps x channels x texel bytes summed over every texture lookup */
  uint32_t pipeline_flags;     /* the YART_FLAG_* set this render ran with, after the per-scene defaults */
  uint32_t reserved1;
  /* instrumented build: rays the lean kernels abandoned at an alpha-tested / transparent candidate and the general
     kernels traced again from the root (they are counted in lean_traversals / shadow_lean_traversals as well) */
  uint64_t retry_extend_traversals, retry_shadow_traversals;
  /* ABI 3: counters of the retired 8-wide walk (value 256 above); kept for the layout, always 0 */
  uint64_t wide_extend_nodes, wide_extend_tris, wide_shadow_nodes, wide_shadow_tris;
  uint64_t wide_extend_handed[4], wide_shadow_handed[4];
  /* ABI 3, batch-synchronous wavefront pipeline: paths of this rank that entered bounce b (b < 16; [0] = every path), summed over
     the batches: how the work of a rank decays with the depth (an imbalance between ranks shows here first) */
  uint64_t paths_at_bounce[16];
} YartStats;

typedef struct YartScene YartScene;

/* Build the device scene (BVH build per mesh — on the device, see yart_hip_scene_create_flags —, flattening, upload). device < 0: current.
 * desc->nodes: pre-order, any nesting depth, fewer than 2^20 nodes (YartNodeDesc).
 * Traversal stack: every mesh's BVH is measured here (inner levels on its deepest path = the stack entries a ray can hold at
 * once); the scene's maximum sizes the kernels' stack spill area — 64 entries, the reference's own stack, or more if a tree
 * needs more. A mesh whose tree is deeper than 192 levels is refused: YART_E_INVALID, and yart_hip_last_error() names the
 * mesh and its depth. Nothing is launched for such a scene. (The same holds for every other scene-creating entry point.) */
int yart_hip_scene_create(const YartSceneDesc* desc, int device, YartScene** out);
/* ... with options. The BVH of every mesh is built on the device (yart_hip_bvh_build_device: the same node array and index
 * permutation as the host build, so the same frames; a mesh the device build refuses is built on the host) unless
 * YART_SCENE_HOST_BVH — or the environment variable YART_HOST_BVH — asks for the host builder. YART_SCENE_DEVICE_BVH names the default. */
#define YART_SCENE_DEVICE_BVH 1u
#define YART_SCENE_HOST_BVH 2u
int yart_hip_scene_create_flags(const YartSceneDesc* desc, int device, uint32_t scene_flags, YartScene** out);
/* Same, from a .yscn container (yart_amd/yscn.py). */
int yart_hip_scene_load(const char* path, int device, YartScene** out);
void yart_hip_scene_destroy(YartScene* scene);

/* New node and light transforms for a scene that is on the device — the next frame of a rigid animation without
 * yart_hip_scene_destroy + yart_hip_scene_create. Re-derived, on the device unless noted: the nodes' transforms, identity flags and
 * children-inclusive boxes, their padded world boxes, the boxes of the top-level hierarchy (scenes of 64 nodes and more; refitted
 * in the tree the scene has; with YART_UPDATE_REBUILD_TOP rebuilt on the host by scene creation's code; with
 * YART_UPDATE_REBUILD_TOP_DEVICE rebuilt on the device, see below), and on the host the
 * lights' transforms, the area lights' area and power, the power CDF and the total power. The scene then renders the bits a scene
 * freshly created from the same description renders. Nothing else is rebuilt or uploaded: BVHs, vertex / leaf / texture arrays,
 * materials and environment tables stay. A scene graph of more than 64 levels is re-derived on the host and uploaded.
 * nodes: n_nodes records, parent and mesh as at create, fwd / inv the new transforms. lights: n_lights = 0 leaves the lights
 * untouched, else every record as at create except fwd / inv (a light that lies on a moved node moves only if its record does).
 * Returns after the work has completed on `stream`. Takes the scene's lock like a render: it must not be called from a wave or tile
 * callback of the same scene.
 * YART_E_INVALID, with the scene and the device exactly as they were (everything is checked before the first write): scene, update
 * or nodes NULL; struct_size too small; unknown flags; YART_UPDATE_REBUILD_TOP_DEVICE on a `scene` that is not a live handle of this
 * library (that flag alone is checked against the handle before it is read); n_nodes not the scene's; a node's parent or mesh changed; n_lights neither 0
 * nor the scene's; a light field other than fwd / inv changed; a matrix word of a node or light not finite; a mesh of the scene
 * whose vertex box is not finite; a `stats` whose struct_size is below 8 (its first two fields).
 * stats: the caller sets stats->struct_size = sizeof(YartSceneUpdateStats) before the call; that many bytes are written.
 * Any other failure (YART_E_HIP: a copy or a launch failed after the first write) leaves the device arrays and the library's host
 * copy in an unspecified state: the scene is unusable and is to be destroyed.
 * Stream order: the copies and kernels of the update are enqueued on `stream`; the caller orders them against renders of this
 * scene that are still running on OTHER streams (yart_hip_render*_device). A scene's first update (and the first refit after a
 * YART_UPDATE_REBUILD_TOP) also uploads its topology tables with blocking copies on the null stream.
 * The top-level hierarchy after an update. A refit (flags 0) keeps the tree the scene has and is the cheapest; the tree filters
 * poorly once instances have moved far from where it was built. YART_UPDATE_REBUILD_TOP synchronises the stream, rebuilds on the host
 * from the downloaded world boxes and uploads. YART_UPDATE_REBUILD_TOP_DEVICE rebuilds on `stream` from the world boxes the update's
 * own chain has just written (csrc/tlas_build_kernels.inc): no synchronisation and no host work between the world-box kernel and the
 * last build kernel, the finished tree is copied to the library's host image asynchronously, and the wait at the end of the call is
 * the only one. All three leave the bytes of a freshly created scene in the device's and the host's tree (a refit: its boxes). The
 * two rebuild flags exclude each other (YART_E_INVALID). A scene without a hierarchy (fewer than 64 nodes) takes either and builds
 * nothing. The device rebuild's first use uploads the tables of the scene's leaf count with blocking copies; its launches are counted
 * in stats->launches: per level that holds a range of more than 2048 mesh nodes 2 + the bitonic merge stages above 2048 keys, one
 * for all subtrees, one per level of the tree. Cost on an MI355X (profiles/top_rebuild.txt; refit / host rebuild / device rebuild of
 * one run): 0.26 / 1.10 / 0.61 ms for 4 096 instances, 0.41 / 4.41 / 0.82 ms for 16 000, 1.15 / 20.4 / 1.78 ms for 65 536.
 * Out of scope — re-create the scene: the replicas of a YartMulti. A changed topology (nodes added, removed, re-parented or
 * re-meshed) is refused here and taken by yart_hip_scene_update_graph below. Deforming meshes: yart_hip_scene_update_meshes below;
 * materials, light emission and environment images: yart_hip_scene_update_lighting below. */
#define YART_UPDATE_REBUILD_TOP 1u   /* rebuild the top-level hierarchy (host, create's own code) instead of refitting its boxes */
#define YART_UPDATE_REBUILD_TOP_DEVICE 2u   /* rebuild it on the device, on the caller's stream: the same bytes */
typedef struct YartSceneUpdate {
  uint32_t struct_size;              /* sizeof(YartSceneUpdate) */
  uint32_t n_nodes;                  /* the scene's node count */
  const YartNodeDesc* nodes;         /* parent and mesh as at create; fwd / inv: the new transforms */
  uint32_t n_lights;                 /* 0: lights untouched; else the scene's light count */
  const YartLightDesc* lights;       /* every field as at create except fwd / inv */
  uint32_t flags;                    /* YART_UPDATE_* */
} YartSceneUpdate;
/* launches: kernels launched; ms_total: wall time of the call; ms_device: from the first copy to the last on the stream */
typedef struct YartSceneUpdateStats { uint32_t struct_size, launches; double ms_total, ms_device; } YartSceneUpdateStats;
int yart_hip_scene_update(YartScene* scene, const YartSceneUpdate* update, void* stream, YartSceneUpdateStats* stats /* may be NULL */);

/* A new NODE LIST for a scene that is on the device — an object spawned or removed, one hidden (mesh = -1), a level of detail swapped
 * (a node's mesh index), an instance moved to another group — without yart_hip_scene_destroy + yart_hip_scene_create: no mesh BVH is
 * rebuilt and no texture uploaded. The contract is that of the other update entries: afterwards the scene holds, and renders in
 * every pipeline, the bits of a scene freshly created from the same description with the new node list, and the entry combines with
 * the other four in any order. Meshes, BVHs, vertex / leaf / texture arrays, materials and environment tables stay where they are.
 * Lights do not depend on the nodes (a YartLightDesc carries its own mesh, triangle and transform): they are touched only when
 * `lights` is given, exactly as in yart_hip_scene_update.
 * nodes: the whole new list, n_nodes records in pre-order, node 0 the root; the count, every parent, every mesh index and every
 * transform may differ from the scene's. Re-derived: on the host, in one integer pass over the list (csrc/graph_update.hpp), skip
 * links, depths, the topology words of the world boxes, identity flags, the level tables of the update chain and the leaf list of the
 * top-level hierarchy; on the device, on `stream`, from the staged descriptors and 16 bytes of topology per node: the node records'
 * topology fields (one kernel), then yart_hip_scene_update's own chain — transforms, children-inclusive boxes, world boxes — and the
 * top-level hierarchy, BUILT (there is no refit: the leaf set changed): on the device with flags 0 or YART_UPDATE_REBUILD_TOP_DEVICE,
 * on the host by scene creation's code with YART_UPDATE_REBUILD_TOP. A list of fewer than 64 nodes, or one without a mesh node,
 * leaves no hierarchy, and a render takes the forms a fresh scene of that size takes. A graph of more than 64 levels is re-derived on
 * the host and uploaded, as in yart_hip_scene_update. The traversal stack bound follows (the deepest mesh or the new hierarchy's height).
 * Memory: the node, world-box, hierarchy and staging arrays and the tables grow on demand — an array that has to hold n elements and
 * does not is re-allocated for n + n / 2 + 64 — and never shrink: an animation that appends a node per frame allocates on a vanishing
 * share of its frames. A grown array is a new allocation: the caller orders the update against renders still running on other streams,
 * as for every update. The tables of a changed leaf list are uploaded with blocking copies (an unchanged one: none).
 * The kept previous frame. A graph update discards what yart_hip_scene_keep_previous kept — the kept node array is another list's —:
 * until the next yart_hip_scene_keep_previous, yart_hip_scene_pixel_motion_* answers as on a scene that never kept a frame,
 * YART_E_INVALID ("yart_hip_scene_keep_previous was never called on this scene"). Per-pixel motion across a graph change is out of
 * scope. Node indices are the temporal accumulator's key (ids(p)[0]): a caller who wants history across a change keeps the surviving
 * nodes' indices stable — hide a node with mesh = -1 instead of removing it, and append new children of the root at the end of the
 * list, which pre-order allows. The accumulator does not remap indices.
 * Not kept current: the default pipeline's lobe-share heuristic stays as at create (every pipeline renders the same frame).
 * Locking, `stream`, `stats` and failures other than YART_E_INVALID as for yart_hip_scene_update; stats->launches counts the topology
 * kernel, the chain's launches and the device build's.
 * YART_E_INVALID, with the scene and the device exactly as they were (everything is checked before the first write): scene, update
 * or nodes NULL; struct_size too small; unknown flags or both rebuild flags; n_nodes 0 or 2^20 and more; node 0's parent not -1;
 * another node's parent negative or not below the node's index; with flags 0 or YART_UPDATE_REBUILD_TOP_DEVICE a `scene` that is
 * not a live handle of this library; a `stats` whose struct_size is below 8; n_lights neither 0 nor the scene's, or a light that
 * yart_hip_scene_update would refuse; a mesh index that is not below the scene's mesh count (any negative index: no mesh); a matrix
 * word of a node not finite; a mesh of the scene whose vertex box is not finite; a hierarchy higher than the 192 entries of the
 * traversal stack (its height depends on the number of mesh nodes only, so it is known before any write; below 2^20 nodes it is at
 * most 20).
 * Cost on an MI355X (profiles/graph_update.txt; 1 % of the instances appended, device build / host build / destroy + create of the
 * same run): 0.70 / 1.15 / 2.9 ms for 4 096 instances, 1.10 / 4.55 / 7.6 ms for 16 000, 2.79 / 20.4 / 27.3 ms for 65 536; the
 * transform update with a device rebuild on the same scenes: 0.62, 0.84 and 1.78 ms.
 * Out of scope — re-create the scene: face or vertex counts, uvs, texture assignments, lights added or removed, and the replicas of
 * a YartMulti. */
typedef struct YartSceneGraphUpdate {
  uint32_t struct_size;              /* sizeof(YartSceneGraphUpdate) */
  uint32_t n_nodes;                  /* the NEW node count: 1 .. 2^20 - 1 */
  const YartNodeDesc* nodes;         /* the new list, pre-order, node 0 the root (parent -1) */
  uint32_t n_lights;                 /* as YartSceneUpdate: 0 = untouched, else the scene's count */
  const YartLightDesc* lights;
  uint32_t flags;                    /* 0 or YART_UPDATE_REBUILD_TOP_DEVICE: the hierarchy built on the device;
                                        YART_UPDATE_REBUILD_TOP: on the host. There is no refit: the leaf set changed. */
} YartSceneGraphUpdate;
int yart_hip_scene_update_graph(YartScene* scene, const YartSceneGraphUpdate* update, void* stream, YartSceneUpdateStats* stats /* may be NULL */);

/* New vertices for meshes of a scene that is on the device — the next frame of a skinned character, a cloth or a morphing height
 * field without yart_hip_scene_destroy + yart_hip_scene_create: textures, footprint records, environment tables, materials and every
 * mesh that is not listed stay where they are. Per listed mesh the positions (and normals / tangents, if given) are uploaded and the
 * vertex arrays rewritten; the mesh's BVH is REBUILT on the device by the builder scene creation uses (not refitted: the contract is
 * the bits the reference renders, and its Mesh constructor builds the tree from the vertices it is given — a refitted tree changes
 * the traversal order, and with it the stochastic alpha-test draws and equal-t ties); leaf records, link words (alpha bit, span),
 * the mesh's alpha flag and, with normals / tangents, the shading records are re-derived on the device; the node array is repacked
 * when a tree's node count changed; the traversal stack bound is re-derived (it sizes the spill area of the next render, growing or
 * shrinking). On the host, from the caller's positions: the mesh's vertex box (exact in the sign of zeros) and area, power, power CDF
 * and total power of area lights on a listed mesh. Then the nodes' boxes, world boxes and the top-level hierarchy are re-derived by
 * yart_hip_scene_update's own chain with the scene's current transforms (flags: YART_UPDATE_REBUILD_TOP / _DEVICE as there). Afterwards the
 * scene holds, and renders, the bits of a scene freshly created from the same description; yart_hip_bvh_info / yart_hip_bvh_copy
 * return the new tree, a later yart_hip_scene_update starts from the new boxes. The two entries combine in either order for a frame
 * that moves nodes and deforms meshes. Faces, materials, uvs, face_light, the node list and the transforms are unchanged.
 * Locking, `stream` and `stats` as for yart_hip_scene_update (the build reads a few counter words back per tree level: `stream` is
 * synchronised that often). Scratch memory of the build is kept in the scene and grown on demand: an animation allocates nothing
 * per frame once its largest mesh has been built and a node count has changed twice.
 * YART_E_INVALID, with the scene and the device exactly as they were: scene, update or meshes NULL; struct_size too small; unknown
 * flags; n_meshes 0 or more than the scene's mesh count; a mesh index out of range or listed twice; n_vertices not the mesh's;
 * positions NULL; a position, normal or tangent word not finite; a rebuilt tree deeper than 192 levels (known only after the build:
 * every listed mesh is built into scratch first, the scene is written once all have built; the message names the mesh and its
 * depth, as scene creation's does); a mesh that is not listed whose vertex box is not finite; stats->struct_size below 8.
 * A mesh the device build refuses, and every mesh under the environment variable YART_HOST_BVH, is built and derived on the host
 * and uploaded: the same bytes.
 * Not kept current: the default pipeline's lobe-share heuristic stays as at create (every pipeline renders the same frame).
 * Changed faces or vertex counts, uvs, a face's material index: yart_hip_scene_replace_meshes below. Out of scope — re-create the
 * scene: the replicas of a YartMulti
 * (the materials' values, light emission and environment images: yart_hip_scene_update_lighting below).
 * Motion for the temporal accumulator: yart_hip_scene_keep_previous before the frame's updates and yart_hip_scene_pixel_motion_device
 * after its render (below) say per pixel where a deformed — or rigidly moved — surface point was in the previous frame. */
typedef struct YartMeshUpdate {
  uint32_t mesh;                     /* index into the scene's meshes */
  uint32_t n_vertices;               /* the mesh's vertex count, as at create */
  const float* positions;            /* HOST, 3 per vertex, required */
  const float* normals;              /* HOST, 3 per vertex, or NULL: kept */
  const float* tangents;             /* HOST, 4 per vertex, or NULL: kept */
} YartMeshUpdate;
typedef struct YartSceneMeshUpdate {
  uint32_t struct_size;              /* sizeof(YartSceneMeshUpdate) */
  uint32_t n_meshes;                 /* meshes listed: 1 .. the scene's mesh count */
  const YartMeshUpdate* meshes;      /* each mesh at most once */
  uint32_t flags;                    /* YART_UPDATE_REBUILD_TOP or YART_UPDATE_REBUILD_TOP_DEVICE */
} YartSceneMeshUpdate;
int yart_hip_scene_update_meshes(YartScene* scene, const YartSceneMeshUpdate* update, void* stream, YartSceneUpdateStats* stats /* may be NULL */);

/* Whole new meshes for a scene that is on the device — a fluid surface extracted every frame, a re-tessellated terrain, a level of
 * detail streamed in — without yart_hip_scene_destroy + yart_hip_scene_create: textures, footprint records, environment tables,
 * materials and the trees of every mesh that is not listed stay on the device. `desc` is what yart_hip_scene_create takes for a mesh:
 * positions, normals, tangents, uvs and faces (i0, i1, i2, material), all required; n_vertices and n_faces are free to differ from
 * the mesh's. Per listed mesh the arrays are uploaded, the BVH is built by the builder scene creation uses, and leaf records, link
 * words, the alpha flag, the shading records (normals, tangents, uvs, material, light -1) and the vertex arrays are derived on the
 * device into scratch. Then the pools that are indexed by triangle, by vertex and by BVH node — shadeTris, leafTris, triVerts,
 * triLight, vPos, vNormal, vTangent, vUV, bvhNodes — are repacked on the device into second arrays as scene creation lays them
 * out (triOffset, leafOffset and vertOffset running sums, odd nodeOffsets behind a zero pad record, two zero records behind the
 * last mesh; the ShadeTri index in the leaf records of every mesh that moves is shifted), and the arrays are swapped. If no listed
 * mesh changes its triangle, vertex or node count, nothing is repacked: the new records are copied into place. The stack bound, the
 * nodes' boxes, world boxes and the top-level hierarchy follow as for yart_hip_scene_update_meshes (flags: YART_UPDATE_REBUILD_TOP /
 * _DEVICE as there; the default is a refit — the leaf set of the top level does not change). Afterwards the scene holds, and renders
 * in every pipeline, the bits of a scene freshly created from the same description; the entry combines in any order with the five
 * yart_hip_scene_update* entries. Locking, `stream` and `stats` as for yart_hip_scene_update_meshes. The frame
 * yart_hip_scene_keep_previous kept is discarded (its vertex array is indexed by scene-wide vertex).
 * Memory: the second arrays are kept in the scene, each grown to one and a half times what a call needs when it is too small, so an
 * animation allocates nothing per frame once both arrays of every pool have held its largest frame — and holds up to twice the geometry pools it needs (per
 * triangle 128 + 48 + 16 + 4 bytes, per vertex 56 bytes, per BVH node 32 bytes), plus the scratch of the listed meshes.
 * YART_E_INVALID, with the scene and the device exactly as they were (counts are checked before any array is read): scene, update or
 * meshes NULL; struct_size too small; unknown flags or both rebuild flags; YART_UPDATE_REBUILD_TOP_DEVICE on a handle that is not a
 * live scene; n_meshes 0 or more than the scene's mesh count; a mesh index out of range or listed twice; n_faces 0 or 2^25 and
 * more; n_vertices 0; positions, normals, tangents, uvs or faces NULL; a vertex index >= n_vertices; a material index >= the scene's
 * material count; a position, normal, tangent or uv word not finite; a mesh that is not listed whose vertex box is not finite; a
 * rebuilt tree deeper than 192 levels (every listed mesh is built into scratch first, the scene is written once all have built);
 * stats->struct_size below 8; a listed mesh that a light of the scene names (YartLightDesc::mesh) or that was created with a
 * face_light entry other than -1; a face_light that is not NULL and has an entry other than -1.
 * Out of scope — re-create the scene: emissive meshes (a mesh with area lights changes the light list, which no entry does), the
 * replicas of a YartMulti. */
typedef struct YartMeshReplace {
  uint32_t mesh;                     /* index into the scene's meshes */
  YartMeshDesc desc;                 /* HOST arrays, as for yart_hip_scene_create; face_light NULL or all -1 */
} YartMeshReplace;
typedef struct YartSceneMeshReplace {
  uint32_t struct_size;              /* sizeof(YartSceneMeshReplace) */
  uint32_t n_meshes;                 /* meshes listed: 1 .. the scene's mesh count */
  const YartMeshReplace* meshes;     /* each mesh at most once */
  uint32_t flags;                    /* YART_UPDATE_REBUILD_TOP or YART_UPDATE_REBUILD_TOP_DEVICE */
} YartSceneMeshReplace;
int yart_hip_scene_replace_meshes(YartScene* scene, const YartSceneMeshReplace* update, void* stream, YartSceneUpdateStats* stats /* may be NULL */);

/* New materials, new light emission and new environment images for a scene that is on the device — a lamp that dims, a material
 * whose colour or roughness is keyed, a sky whose sun moves — without yart_hip_scene_destroy + yart_hip_scene_create: meshes, BVHs,
 * the scene graph, material textures and their footprint records stay where they are. Afterwards the scene holds, and renders in every
 * pipeline, the bits of a scene freshly created from the same description. The three update entries combine in any order.
 * materials (n_materials = 0: untouched; else the scene's material count, every record): every numeric field may change — base,
 * emission, metallic, roughness, transmission, ior, anisotropic, aniso_rotation, clearcoat, clearcoat_roughness, normal_scale,
 * volume_color, volume_density. The device records are re-derived on the host by scene creation's arithmetic and uploaded, with the
 * per-material lobe classes. The six texture slots stay where creation left them, the alpha-test flag stays (it depends on the texels),
 * the emission flag is re-derived.
 * lights (n_lights = 0: untouched; else the scene's light count, every record): emission, radius, fwd and inv may change. Re-derived on
 * the host by the functions creation uses: the area lights' area and power, the power CDF and the total power; a uniform infinite
 * light's power; an image light's power from its radius and its image's average radiance. The library does not couple a light's
 * emission to its material's: as at create the caller describes both.
 * images (n_images = 0: untouched; each texture at most once): new texels for the float RGB map of image lights, of the same size.
 * They are uploaded into the texture's place, its footprint records are rewritten where the scene has them, and for every image light
 * that uses the texture the sampling tables — function, conditional CDFs, row integrals, marginal CDF and integral, guide tables,
 * interleaved records — are rebuilt in place ON THE DEVICE; the image's average radiance (a sequential binary32 sum in row-major
 * order) is taken on the host meanwhile, and the lights' power follows it.
 * Locking, `stream`, `stats` and "returns after the work has completed on `stream`" as for yart_hip_scene_update.
 * YART_E_INVALID, with the scene and the device exactly as they were (everything is checked before the first write): scene or update
 * NULL; struct_size too small; flags other than 0; all three counts 0; a count that is neither 0 nor the scene's, or its pointer NULL;
 * a material's tex_* or thin_transmission changed; a change that would make a thin material's transmission positive or zero (the
 * transparency bit lives in the meshes' leaf records); a light's type, mesh, tri, two_sided or texture changed; a word of a material,
 * of a light's radius or emission or of a matrix that is not finite; a texture index that is out of range, listed twice, not float RGB
 * or not used by an image light; width or height not the texture's; pixels NULL; a texel word that is not finite or whose magnitude
 * exceeds 2^64 (stricter than creation, on purpose: no row sum, marginal sum or average can then overflow, and every CDF is finite
 * and nondecreasing); stats->struct_size below 8.
 * Any other failure (YART_E_HIP) leaves the scene unusable, as for the other update entries.
 * Not kept current: the default pipeline's lobe-share heuristic stays as at create (every pipeline renders the same frame), as for
 * yart_hip_scene_update_meshes.
 * Out of scope — re-create the scene: changed texture assignments, changes that flip a material's transparency or
 * thin_transmission, lights added or removed, face_light changes, a resized environment image, and the replicas of a YartMulti
 * (the texels of material textures: yart_hip_scene_update_textures below). */
typedef struct YartEnvImageUpdate {
  uint32_t texture;                  /* index into the scene's textures: a float RGB texture that at least one image light uses */
  uint32_t width, height;            /* the texture's, as at create */
  const float* pixels;               /* HOST, 3 floats per texel, row-major, required */
} YartEnvImageUpdate;
typedef struct YartSceneLightingUpdate {
  uint32_t struct_size;              /* sizeof(YartSceneLightingUpdate) */
  uint32_t n_materials;              /* 0: materials untouched; else the scene's material count */
  const YartMaterialDesc* materials; /* every record; tex_* and thin_transmission as at create */
  uint32_t n_lights;                 /* 0: lights untouched; else the scene's light count */
  const YartLightDesc* lights;       /* every record; type, mesh, tri, two_sided and texture as at create */
  uint32_t n_images;                 /* 0: environment images untouched */
  const YartEnvImageUpdate* images;  /* each texture at most once */
  uint32_t flags;                    /* none defined: must be 0 */
} YartSceneLightingUpdate;
int yart_hip_scene_update_lighting(YartScene* scene, const YartSceneLightingUpdate* update, void* stream, YartSceneUpdateStats* stats /* may be NULL */);

/* New texels for 8-bit material textures of a scene that is on the device — a video screen, a flip-book decal, an animated emission
 * or roughness map, a cut-out that grows or dissolves — without yart_hip_scene_destroy + yart_hip_scene_create. Afterwards the scene
 * holds, and renders in every pipeline, the bits of a scene freshly created from the same description. The four update entries combine
 * in any order. Per listed texture:
 * texels: the pixels are copied into the texture's place (from host memory, or with YART_TEXELS_ON_DEVICE from memory of the scene's
 * device: a decoded video frame, a procedural map); the neighbouring textures and the pad bytes behind a texture whose byte count is
 * no multiple of 4 are untouched. The library's host copy follows (one device-to-host copy for device pixels).
 * footprint records: rewritten where the scene has them, once per place that holds the texture — its own array, and every bundle of a
 * base-colour / normal / metal-rough triple it is a member of (several materials share a bundle).
 * alpha test: for a 4-channel texture that is some material's tex_base, "an alpha byte below 255" is decided anew by one pass over the
 * texels on the device. Only where a material's flag CHANGES, the chain that scene creation derives from it is re-derived on the
 * device, in place, for the meshes that have a face of such a material: the leaf records' alpha bit, the alpha bit of every BVH node's
 * link word and the mesh's alpha flag (the shadow rays' pruning reads them). New texels that leave every flag as it was launch nothing
 * beyond the copy, the footprint records and that one pass.
 * Locking, `stream`, `stats` and "returns after the work has completed on `stream`" as for yart_hip_scene_update_lighting (`stream` is
 * synchronised once more where a flag changed: the flags are read back before the chain is launched).
 * YART_E_INVALID, with the scene and the device exactly as they were (everything is checked before the first write): scene or update
 * NULL; struct_size too small; flags other than the defined ones; n_textures 0, or its pointer NULL; a texture index that is out of
 * range (the scene's textures as given at create: the entries behind them, which creation adds for bundles, count as out of range) or
 * listed twice; a float texture (image lights' maps: yart_hip_scene_update_lighting); a width, height or channel count that is not
 * the texture's; pixels NULL; stats->struct_size below 8.
 * Any other failure (YART_E_HIP) leaves the scene unusable, as for the other update entries.
 * Not kept current: the default pipeline's lobe-share heuristic, as for the other entries.
 * Out of scope — re-create the scene: changed texture assignments, resized textures, thin_transmission / transparency flips, and the
 * replicas of a YartMulti. */
#define YART_TEXELS_ON_DEVICE 1u     /* YartTextureUpdate::flags: pixels is device memory of the scene's device */
typedef struct YartTextureUpdate {
  uint32_t texture;                  /* index into the scene's textures as given at create */
  uint32_t width, height, channels;  /* the texture's, as at create */
  const void* pixels;                /* 8-bit texels, row-major, channels bytes per texel, required */
  uint32_t flags;                    /* YART_TEXELS_ON_DEVICE, else pixels is host memory */
} YartTextureUpdate;
typedef struct YartSceneTextureUpdate {
  uint32_t struct_size;              /* sizeof(YartSceneTextureUpdate) */
  uint32_t n_textures;               /* textures listed: at least 1 */
  const YartTextureUpdate* textures; /* each texture at most once */
  uint32_t flags;                    /* none defined: must be 0 */
} YartSceneTextureUpdate;
int yart_hip_scene_update_textures(YartScene* scene, const YartSceneTextureUpdate* update, void* stream, YartSceneUpdateStats* stats /* may be NULL */);

/* The scene remembers the frame it holds as its PREVIOUS frame: its node array and its vertex positions are copied into scene-owned
 * arrays — two device-to-device copies on `stream`; the call returns after they have completed. The arrays are allocated by the
 * first call: a scene that never calls it pays nothing. Called once per frame, BEFORE that frame's yart_hip_scene_update /
 * yart_hip_scene_update_meshes (which run in either order and do not change; yart_hip_scene_update_graph discards the kept frame:
 * keep again after it). Locking as for the update entries. The replicas of a
 * YartMulti are out of scope. YART_E_INVALID: a NULL scene; YART_E_HIP: the allocation or a copy failed. */
int yart_hip_scene_keep_previous(YartScene* scene, void* stream);

/* PER-PIXEL MOTION between the previous frame (yart_hip_scene_keep_previous) and the scene as it is now, from the feature buffers of
 * a frame rendered from the scene as it is now: per pixel where the surface point it shows was in the previous frame, P', and what
 * its normal was, n' — for nodes that moved rigidly and for meshes deformed by yart_hip_scene_update_meshes alike. The records are
 * what yart_hip_temporal_set_pixel_motion takes. d_aovs: position, normal, coverage and ids are required; buffers of other mask bits
 * are not touched. d_records: 8 floats per pixel, 16-byte aligned, read as two 16-byte words {P'.xyz, kind} and {n'.xyz, 0}; kind is
 * a uint32 stored as bits: 0 static (the record is all zero), 1 moved. DEVICE pointers on `stream`; returns after completion on it.
 * DEFINITION. Two kernels; csrc/scene_motion.hpp states them, yart_amd/scene_motion.py scene_motion_reference is the NumPy statement
 * the tests compare with, on bits.
 *   Per scene node, in binary64 (every operation individually rounded, no FMA contraction), by a walk from the node to the root over
 *   `parent`, for the current and for the previous node array, with the top three rows of fwd / inv as 3 x 4 matrices whose last
 *   row is (0, 0, 0, 1):   Wc = fwd_root · … · fwd_node,  Ac = inv_node · … · inv_root;  Wp, Ap the same of the previous array.
 *   The walk starts from the node's own matrix and multiplies a parent's on (W = fwd_parent · W, A = A · inv_parent); an element of a
 *   product is (x0 * y0 + x1 * y1) + x2 * y2, and + x3 (the word times 1) in the last column. The four matrices are rounded to
 *   binary32 at the end. changed = some fwd or inv word (all 16 of each) of a node on the chain differs between the two arrays.
 *   Per pixel p, in binary32 under the rules of the temporal definition below (dot, cross, individually rounded operations in the
 *   order written; sqrtf correctly rounded), with (node, ·, ·, tri) = ids(p), P = position(p), n = normal(p):
 *   STATIC — an all-zero record — if any of: coverage(p) != 1.0f; a component of P or n is not finite; uint32(node) >= the scene's
 *     node count; the node has no mesh; uint32(tri) >= the triangle count of the node's mesh (the scene's, not ids(p)[1]); the node
 *     is not changed and the x, y, z words of the triangle's three current vertex positions equal its three previous ones.
 *   Otherwise, with a, b, c the current and a', b', c' the previous positions of the triangle's vertices, M · x = (dot(M row i .xyz,
 *   x) + M row i .w) and M_lin^T · x = (dot(M column j of the 3 x 3 part, x)):
 *     po = Ac · P;   e1 = b - a;   e2 = c - a;   r = po - a
 *     d11 = dot(e1, e1);  d12 = dot(e1, e2);  d22 = dot(e2, e2);  r1 = dot(r, e1);  r2 = dot(r, e2);  det = d11 * d22 - d12 * d12
 *     u = (d22 * r1 - d12 * r2) / det;   v = (d11 * r2 - d12 * r1) / det
 *     f1 = b' - a';   f2 = c' - a';   p' = (a' + u * f1) + v * f2;   P' = Wp · p'
 *   — the affine map from the current triangle to the previous one, extended to the triangle's plane (position is an average over
 *   the samples and may lie beyond sample 0's triangle); the offset along the normal is dropped. The normal goes by the inverse
 *   transpose of the same map:
 *     no = Wc_lin^T · n;   g11, g12, g22, gdet from f1, f2 as d11, d12, d22, det from e1, e2
 *     D1 = (g22 * f1 - g12 * f2) / gdet;   D2 = (g11 * f2 - g12 * f1) / gdet;   N = cross(e1, e2);   N' = cross(f1, f2)
 *     gamma = dot(no, N) / sqrtf(dot(N, N) * dot(N', N'))
 *     n'o = (dot(no, e1) * D1 + dot(no, e2) * D2) + gamma * N';   n' = Ap_lin^T · n'o     (no renormalisation)
 *   — exact for per-triangle rigid motion; a strain changes |n'| only through the tangential part of a shading normal.
 *   kind = 1 with P' and n' as computed, finite or not: the accumulator refuses a non-finite record per pixel.
 * YART_E_INVALID, with a message and before any device work: a NULL scene, d_aovs or d_records; a required buffer missing from
 * d_aovs->mask (or NULL, or beyond its struct_size); 0 pixels or more than 2^28; a d_records that is not 16-byte aligned; a scene on
 * which yart_hip_scene_keep_previous was never called. Locking as for the update entries. */
struct YartAovBuffers;           /* (defined with the feature buffers below) */
int yart_hip_scene_pixel_motion_device(YartScene* scene, const struct YartAovBuffers* d_aovs, uint32_t width, uint32_t height,
                                       float* d_records, void* stream);
/* Same, HOST pointers (records needs no alignment): the buffers are copied to the scene's device and the records copied back. */
int yart_hip_scene_pixel_motion_host(YartScene* scene, const struct YartAovBuffers* aovs, uint32_t width, uint32_t height, float* records);

/* glTF 2.0 / GLB import — what `gltf::load(path)` (src/gltf/gltf.cpp:319-358) followed
 * by the frontend's environment set-up (src/main.cpp:78-86) gives the renderer: materials with the KHR
 * transmission / ior / anisotropy / clearcoat / volume / emissive_strength extensions (gltf.cpp:62-176),
 * gamma-2 re-encoded textures (core/texture.hpp:62-92), the primitives of each mesh merged (gltf.cpp:178-270),
 * the T*R*S node tree and one AreaLight per emissive triangle with per-node light indices (gltf.cpp:272-317).
 * Embedded PNG and JPEG (baseline / progressive Huffman) images are decoded to the bytes the reference's
 * stb_image call yields; arithmetic-coded / CMYK JPEG images and sparse accessors are refused (YART_E_IO, see yart_hip_last_error). opts may be NULL (asset only). env_hdr_path: octahedral-mapped Radiance .hdr wrapped
 * in ImageInfiniteLight(env_radius, texture) (core/texture.cpp:5-20); uniform_env != 0 adds
 * UniformInfiniteLight(env_radius, uniform_emission). env_radius <= 0 means 100 (main.cpp:82). */
typedef struct YartImportOptions {
  const char* env_hdr_path;
  float env_radius;
  uint32_t uniform_env;
  float uniform_emission[3];
  uint32_t reserved[4];
} YartImportOptions;
int yart_hip_scene_load_gltf(const char* path, const YartImportOptions* opts, int device, YartScene** out);
/* Host only (no device needed): the imported scene written as a .yscn container — the same bytes
 * yart_hip_scene_load reads, and what oracle/ takes to render the asset with the reference. */
int yart_hip_gltf_to_yscn(const char* gltf_path, const YartImportOptions* opts, const char* yscn_path);

/* Blocking render (Renderer::renderSync). out_rgba: caller-owned host buffer of
 * width*height*4 floats, linear HDR with exposure applied, alpha = 1 — the
 * reference's m_hdrBuffer (tile-renderer.hpp:93, tonemapper == nullptr). */
int yart_hip_render(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                    float* out_rgba, YartStats* stats);
/* Same, one wave of the schedule at a time (tile-renderer.hpp:264-289): after every wave out_rgba holds the frame
 * blended so far and on_wave is called — what Renderer::onRenderWaveComplete reports (renderer.hpp:33-38, 56) —
 * with that wave's statistics; a non-zero return stops the render after this wave, as Renderer::abort() does
 * between tiles, and the call returns YART_ABORTED. on_wave may be NULL. */
typedef int (*YartWaveCallback)(void* user, const YartStats* wave_stats, uint32_t wave, uint32_t wave_samples,
                                uint32_t samples_taken, uint32_t total_samples);
int yart_hip_render_waves(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                          float* out_rgba, YartStats* stats, YartWaveCallback on_wave, void* user);
/* Same, with tile granularity (Renderer::onRenderTileComplete, renderer.hpp:40-50, 58; fired by finishTile,
 * tile-renderer.hpp:243-262 — the frontend uploads each finished tile from it, frontend main.cpp:206). A wave is
 * rendered batch by batch over this rank's pixel blocks in Morton order (YartRenderParams.max_batch_paths bounds a
 * batch; blocks are tile_size, or shard_tile, pixels wide); when a batch ends, the blocks it completed are copied into
 * out_rgba — which then holds, for those pixels, the frame blended up to this wave — and on_tile is called once per
 * block. A non-zero return stops the render after the current batch (YART_ABORTED; out_rgba then holds whatever had
 * been blended). YartTileInfo.rays is the reference's TileData.rays: the rays (path segments + unoccluded NEE rays,
 * mis-integrator.cpp:22, 126) of the block's pixels in this wave — every finished path carries its own count, the blend
 * kernel sums them per pixel, a small kernel per block; the blocks' counts of a wave sum to that wave's YartStats.rays. */
typedef struct YartTileInfo {
  uint32_t x, y, width, height;     /* TileData.offset / size */
  uint32_t index, total;            /* TileData.index (1-based count of finished blocks of this wave) / total */
  uint32_t wave, wave_samples, samples_taken, total_samples;   /* samples_taken: after this wave */
  uint64_t rays;                    /* TileData.rays: this block's rays of this wave */
  double ms;                        /* since the wave started */
} YartTileInfo;
typedef int (*YartTileCallback)(void* user, const YartTileInfo* tile);
int yart_hip_render_tiles(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                          float* out_rgba, YartStats* stats, YartWaveCallback on_wave, YartTileCallback on_tile, void* user);
/* Same as yart_hip_render, writing a DEVICE buffer (e.g. a torch tensor's data_ptr) on `stream`
 * (hipStream_t, may be NULL); returns after the work has been enqueued and
 * completed on that stream. */
int yart_hip_render_device(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                           float* d_out_rgba, void* stream, YartStats* stats);

/* First-hit feature buffers ("AOVs"): what bounce 0 of every path of the frame knows about the surface it sees, from the SAME
 * camera samples as the frame — guides for a denoiser (albedo, normal), compositing (coverage, depth), picking (ids), and the
 * per-pixel ray count (where the time goes). The definition is the reference's Hit (cpu/hit.hpp) as testNode / testMesh leave it
 * (cpu/ray-integrator.cpp:20-82) for the camera ray of (pixel, sample): the candidate the stochastic alpha test accepted (the
 * path and the buffers see the same surface), n after BSDF::normal (normal-mapped, world space). For a pixel and its samples
 * s = 0 .. samples-1, misses contributing nothing:
 *   albedo, normal, position, depth   float32 sum over the hitting samples in ASCENDING s, then one division by float(samples);
 *                                     albedo = the base colour ParametricBSDF::fImpl starts from (parametric.cpp:75-78, 90-91)
 *                                     at Hit.uv, depth = Hit.t, position = Hit.p. The order is part of the contract: the result
 *                                     is a pure function of the per-sample values.
 *   coverage                          hitting samples / samples
 *   ids                               of sample 0's hit: node (index into YartSceneDesc.nodes), mesh, material, triangle (Hit.idx);
 *                                     all -1 when sample 0 misses
 *   rays                              the pixel's rays over the whole render (mis-integrator.cpp:22, 126); sums to YartStats.rays
 * Pixels of other ranks are left 0 (ids -1), as in out_rgba: the ranks' buffers add up to the unsharded ones (ids: by max).
 * The buffers do not depend on flags (megakernel and path pool included), max_batch_paths, the wave schedule or the estimator.
 * Memory: the default pipeline holds nothing more per path (the 48-byte feature record of a path lives in the shadow-ray arrays,
 * which are unused until bounce 0 is shaded: still 251 bytes per path); YART_FLAG_MEGAKERNEL and YART_FLAG_PATH_POOL hold 48 bytes
 * more per path of the batch (the batch clamp of max_batch_paths accounts for it); every pipeline 68 bytes per pixel of the rank.
 * start_sample / stop_sample other than the full range are refused (YART_E_INVALID). Several GPUs: yart_hip_multi_* has no feature
 * buffers; shard with rank / world_size, one call per device, and add the buffers. */
#define YART_AOV_ALBEDO   1u   /* 3 floats / pixel */
#define YART_AOV_NORMAL   2u   /* 3 floats */
#define YART_AOV_POSITION 4u   /* 3 floats */
#define YART_AOV_DEPTH    8u   /* 1 float  */
#define YART_AOV_COVERAGE 16u  /* 1 float  */
#define YART_AOV_IDS      32u  /* 4 x int32: node, mesh, material, triangle */
#define YART_AOV_RAYS     64u  /* 1 x uint32 */
#define YART_AOV_ALL      127u
typedef struct YartAovBuffers {
  uint32_t struct_size;        /* sizeof(YartAovBuffers): lets the struct grow without an ABI bump */
  uint32_t mask;               /* YART_AOV_* requested; a requested buffer must be non-NULL, the others are not touched */
  float *albedo, *normal, *position, *depth, *coverage;
  int32_t* ids;
  uint32_t* rays;
} YartAovBuffers;
/* yart_hip_render + feature buffers: host pointers, width * height * channels each, row-major like out_rgba. out_rgba and
 * YartStats.samples / rays are those of yart_hip_render with the same arguments, bit for bit; mask == 0 (or aovs == NULL) is
 * yart_hip_render. A NULL requested buffer, a struct_size that ends before a requested field, unknown mask bits and a partial
 * sample range return YART_E_INVALID before anything is launched. */
int yart_hip_render_aovs(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                         const YartAovBuffers* aovs, YartStats* stats);
/* yart_hip_render_device + feature buffers: DEVICE pointers (e.g. torch tensors' data_ptr) */
int yart_hip_render_aovs_device(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* d_out_rgba,
                                const YartAovBuffers* d_aovs, void* stream, YartStats* stats);

/* Per-pixel sample moments: how noisy a pixel of the frame is, from the frame's OWN samples — the per-(pixel, sample) radiance every
 * pipeline holds at the end of a batch, before the estimator collapses it. For a pixel and its samples s = 0 .. samples-1 over the
 * whole render, in ASCENDING s:
 *   w_s = L_s.xyz * exposureScale      per channel, binary32: the value the estimator is fed
 *   y_s = luma(w_s)                    (w.r * 0.2126f + w.g * 0.7152f) + w.b * 0.0722f, binary32 (csrc/estimator.hpp)
 *   accepted                           iff no component of w_s is NaN, none is negative, and y_s is finite. The rule is fixed: it does
 *                                      not follow params->estimator.
 *   state                              N (uint32) and five BINARY64 sums Sr, Sg, Sb, S1, S2: an accepted sample adds double(w.r),
 *                                      double(w.g), double(w.b), double(y) and double(y) * double(y) (exact); no FMA contraction
 *   finish, once after the last wave   mean.c   = float(S_c / double(N)); 0 when N == 0
 *                                      variance = 0 when N < 2, else v = ((S2 - (S1 * S1) / N) / (N - 1)) / N, every binary64
 *                                                 operation rounded in the order written, a negative v replaced by 0, then rounded
 *                                                 once to binary32: the variance of the pixel's MEAN luminance estimate
 *                                      count    = N
 * The order is part of the contract: the result is a pure function of the per-sample values. It does not depend on flags (megakernel
 * and path pool included), max_batch_paths, pool_paths, the wave schedule or the estimator. csrc/moments.hpp states the arithmetic,
 * yart_amd/moments.py moments_reference is the NumPy statement the tests compare with, on bits. (The sums are binary64 because a
 * pixel's samples arrive wave by wave — no second pass — and a binary32 S2 - S1 * S1 / N cancels on low-noise pixels.)
 * Pixels of other ranks are left 0: the ranks' buffers add up to the unsharded ones. Memory: nothing more per path in any pipeline
 * (only the per-sample radiance is read); 48 bytes per pixel of the rank (the 44 bytes of state, padded), which the batch clamp of
 * max_batch_paths takes off its budget. start_sample / stop_sample other than the full range are refused (YART_E_INVALID). Several
 * GPUs: yart_hip_multi_* does not carry the moments; shard with rank / world_size, one call per device, and add the buffers. */
#define YART_MOMENT_MEAN 1u      /* 3 floats / pixel */
#define YART_MOMENT_VARIANCE 2u  /* 1 float  */
#define YART_MOMENT_COUNT 4u     /* 1 uint32 */
#define YART_MOMENT_ALL 7u
typedef struct YartMomentBuffers {
  uint32_t struct_size;        /* sizeof(YartMomentBuffers): lets the struct grow without an ABI bump */
  uint32_t mask;               /* YART_MOMENT_* requested; a requested buffer must be non-NULL, the others are not touched */
  float *mean, *variance;
  uint32_t* count;
} YartMomentBuffers;
/* yart_hip_render_aovs + moments: host pointers, width * height * channels each, row-major like out_rgba. out_rgba, YartStats.samples /
 * rays and the feature buffers are those of yart_hip_render_aovs with the same arguments, bit for bit; an empty moment mask (or
 * moments == NULL) is yart_hip_render_aovs. aovs may be NULL. A NULL requested buffer, a struct_size that ends before a requested
 * field, unknown mask bits and a partial sample range return YART_E_INVALID before anything is launched. */
int yart_hip_render_moments(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                            const YartAovBuffers* aovs, const YartMomentBuffers* moments, YartStats* stats);
/* yart_hip_render_aovs_device + moments: DEVICE pointers (e.g. torch tensors' data_ptr) */
int yart_hip_render_moments_device(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, float* d_out_rgba,
                                   const YartAovBuffers* d_aovs, const YartMomentBuffers* d_moments, void* stream, YartStats* stats);
/* Diagnostic, no scene: the accumulate and finish kernels of the moments on caller-supplied per-sample records, on the current device.
 * L_rgba: n_pixels * spp records of 4 floats (host; pixel-major, samples ascending; the fourth float is not read). chunks: n_chunks
 * sample counts (each > 0) that sum to spp: one accumulate launch per chunk, as a render launches one per wave. mean (3 per pixel),
 * variance, count (1 per pixel): host, all required. */
int yart_hip_probe_moments(const float* L_rgba, uint32_t n_pixels, uint32_t spp, const uint32_t* chunks, uint32_t n_chunks,
                           float exposure_scale, float* mean, float* variance, uint32_t* count);
/* Diagnostic, no scene: the estimator kernel of the render (one launch, the render's launch geometry) on caller-supplied per-sample
 * records, on the current device. L_rgba: n_pixels * spp records {r, g, b, ray count as uint32 bits} (host; pixel-major, samples
 * ascending). kind: YART_ESTIMATOR_*. pixels: n_pixels distinct words x | y << 16 inside the width x height frame, or NULL: pixel i at
 * (i % width, i / width). hdr_inout (host, width * height * 4): read as the current frame and written back with the listed pixels set
 * to current * w_current + {estimate, 1} * w_wave; the others are not touched. pix_rays (host, n_pixels, or NULL): each pixel's
 * ray counts summed mod 2^32. A null L_rgba / hdr_inout, a zero n_pixels / spp / width / height, a width or height above 65536, a kind
 * outside 0..3, more than 2^26 records, n_pixels > width * height, a pixels[] entry outside the frame and a non-finite
 * exposure_scale / w_current / w_wave return YART_E_INVALID before any device is touched. */
int yart_hip_probe_estimator(const float* L_rgba, uint32_t n_pixels, uint32_t spp, int kind, float exposure_scale,
                             const uint32_t* pixels, uint32_t width, uint32_t height, float w_current, float w_wave,
                             float* hdr_inout, uint32_t* pix_rays);

/* Several GPUs of one node behind one handle — what the reference's worker pool is to CPU threads
 * (TileRenderer::renderImpl starts threadCount workers that pull tiles, tile-renderer.hpp:150-197; finishTile merges
 * each finished tile into the one m_hdrBuffer, :225-241). The scene is replicated on every listed device; device i of
 * N renders the pixel blocks b with b % N == i (blocks of shard_tile / tile_size pixels in Morton order — combined
 * with params->rank / world_size as device i of N of process rank r of R); one host thread per device drives its
 * launches; the merge sends each device's OWN pixels (a packed slab, 1/N of the frame) to devices[0] with RCCL
 * point-to-point calls over xGMI, where they are scattered into the frame, which is then copied to out_rgba.
 * RCCL failures return YART_E_RCCL. A device listed more than once (rehearsal on a one-GPU box) is served by a
 * device-to-device copy instead of RCCL, everything else being the same; bound max_batch_paths then, the replicas
 * share that device's memory. Blocking; the frame equals the single-device render bit for bit. */
typedef struct YartMulti YartMulti;
int yart_hip_multi_create(const YartSceneDesc* desc, const int* devices, uint32_t n_devices, YartMulti** out);
/* from a .yscn container or a .glb / .gltf asset (opts as for yart_hip_scene_load_gltf; ignored for .yscn) */
int yart_hip_multi_load(const char* path, const YartImportOptions* opts, const int* devices, uint32_t n_devices, YartMulti** out);
void yart_hip_multi_destroy(YartMulti* multi);
int yart_hip_multi_device_count(const YartMulti* multi);
/* Failure of a device (SURVEY §5 "failure detection"; the reference has none: a worker thread that dies takes the process along). A
 * HIP error on the host thread of a replica other than devices[0] takes THAT replica out of service for the rest of the handle's life:
 * the call still succeeds — the replica's pixel blocks are rendered on devices[0] after the merge (blocks are idempotent: which
 * device renders a pixel does not change it), in this and in every later render. This entry point reports the replicas out of service
 * (indices into the `devices` list, at most `capacity` written; returns their number) and leaves the first failure's message in
 * yart_hip_last_error(). A failure of devices[0] itself, where the frame is merged, is the call's error (YART_E_HIP). */
int yart_hip_multi_failed_devices(const YartMulti* multi, int* replicas_out, uint32_t capacity);
/* Diagnostic: the RCCL calls of the merge (ncclCommInitAll, one group of ncclSend + ncclRecv on a stream, ncclCommDestroy) on a
 * one-rank communicator of `device` — the rank sends a slab of n_floats to itself and compares. Shows on a one-GPU box that
 * RCCL is linked, initialises and moves a slab; YART_E_RCCL otherwise. */
int yart_hip_multi_rccl_selftest(int device, uint32_t n_floats);
/* stats: samples / rays / test counters summed over the devices, ms_* the slowest device's, ms_total the call's wall time */
int yart_hip_multi_render(YartMulti* multi, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                          YartStats* stats);
/* The progressive form of yart_hip_multi_render (what yart_hip_render_waves / _tiles are to yart_hip_render): one wave of the
 * schedule at a time on all devices, merged, copied to out_rgba and reported through on_wave (Renderer::onRenderWaveComplete
 * fires whatever the number of workers, tile-renderer.hpp:243-282); with on_tile every block of the frame is reported once per
 * wave after that wave's merge, in Morton order, with its own ray count. Either callback may be NULL; a non-zero return stops
 * the render after the current wave (YART_ABORTED). */
int yart_hip_multi_render_tiles(YartMulti* multi, const YartCameraDesc* cam, const YartRenderParams* params, float* out_rgba,
                                YartStats* stats, YartWaveCallback on_wave, YartTileCallback on_tile, void* user);

/* Diagnostics (device code paths, used by the parity tests):
 * per-sample radiance (before exposure) of n (x, y, sample) triples -> 3 floats each */
int yart_hip_probe_samples(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params,
                           uint32_t n, const uint32_t* xys, float* out_rgb, uint64_t* out_rays);
/* Diagnostic: the ZSobol / FastOwen sampler alone on the device (reference core/sampler.hpp:84-173, scrambler.hpp:57-65): for each
 * of n cases (pixel x, pixel y, sample index: 3 words) startPixelSample, then n_draws draws following `pattern` (1 = get1D, 2 = get2D);
 * out receives sum(pattern) floats per case. use_tables != 0: through the per-render sampler tables the wavefront kernels read. */
int yart_hip_probe_sampler(YartScene* scene, uint32_t spp, uint32_t tile, uint32_t n, const uint32_t* cases, uint32_t n_draws,
                           const uint8_t* pattern, int use_tables, float* out);
/* Diagnostic: one math function of the device code at a time, on device 0, without a scene: the inline functions the render
 * kernels call (csrc/ymath.hpp ysinf / ycosf / ysinf2pi / ycosf2pi / ylogf / yexpf, csrc/tonemap.hpp ylog2f / ypowf), the fp32
 * divide and square root as the kernels are compiled, and reverseBits32 (operand and result are raw 32-bit words in float slots).
 * Range form: fn at bit_cast<float>(first_bits + i), i < count (count <= 2^28, the range may not wrap); y is the exponent of
 * YART_MATH_POWF and ignored otherwise; YART_MATH_DIV has no range form. Pairs form: explicit operands a[i], b[i] (b may be
 * NULL for the one-operand functions; for YART_MATH_POWF b holds the exponents). out_host receives one float per input. */
enum YartMathFn {
  YART_MATH_SINF = 0, YART_MATH_COSF = 1, YART_MATH_SINF_2PI = 2, YART_MATH_COSF_2PI = 3, YART_MATH_LOGF = 4, YART_MATH_EXPF = 5,
  YART_MATH_LOG2F = 6, YART_MATH_POWF = 7, YART_MATH_DIV = 8, YART_MATH_SQRT = 9, YART_MATH_BREV = 10, YART_MATH_COUNT = 11
};
int yart_hip_probe_math(int fn, uint32_t first_bits, uint64_t count, float y, float* out_host);
int yart_hip_probe_math_pairs(int fn, uint64_t n, const float* a, const float* b, float* out_host);
/* closest hit of n world rays (ox,oy,oz,dx,dy,dz) -> 16 floats each:
 * hit, t, u, v, px,py,pz, nx,ny,nz, tx,ty,tz, triIdx, lightIdx, backSide */
int yart_hip_probe_hits(YartScene* scene, uint32_t n, const float* rays, float* out);
/* Diagnostic: one walk of the scene (csrc/traverse.hpp traverseScene, then finalizeHit) per caller-supplied ray, in the
 * instantiation `walk` selects: 0 TRAV_GENERAL, 1 TRAV_FAST, 2 TRAV_FAST | TRAV_IDENTITY (YART_E_INVALID unless every node
 * chain of the scene is the identity). The sampler is the one a render with `params` constructs (samples, tile_size).
 * rays: n records of 12 words: origin[3], direction[3], tMax (f32; +inf for a closest-hit ray), kind (0 closest hit, 1
 *   occlusion: the walk of MISIntegrator::unoccluded), x, y, s (the sampler is started on pixel (x, y), sample s before the
 *   walk, so stochastic alpha tests draw what a path's would; x, y < 65536, s < params->samples), one unused word. Every ray
 *   enters the walk with tMin = 0.001 and hit.t = tMax.
 * out: n records of 20 words: 0 hit / occluded, 1 mesh-local triangle, 2 light index (-1: none), 3 back side, 4 t, 5..7 p,
 *   8..10 n, 11..13 tangent (world space; closest-hit rays with a hit, otherwise 0), 14..16 the attenuation the walk
 *   accumulated (1, 1, 1 unless an occlusion ray passed transparent surfaces), 17 one get1D() drawn after the walk (pins the
 *   number of dimensions the walk consumed), 18 deferred, 19 zero. The fast walks set `deferred` and zero every other word for
 *   a ray they hand over to the general walk; for an occlusion ray they report words 0, 14..16 (unoccluded rays) and 17 only,
 *   which is all the shadow kernels take from them. */
int yart_hip_probe_rays(YartScene* scene, const YartRenderParams* params, uint32_t n, const uint32_t* rays, int walk, uint32_t* out);
/* Diagnostic: the shading code (csrc/bsdf.hpp, csrc/lights.hpp) one call at a time on caller-supplied operands, in the forms
 * only the device runs. cases: n records of 32 words, out: n records of 32 words; oracle/shaderec.hpp spells both out: word 0
 * the kind (0 the five GGX table lookups, 1 a texture fetch, 2 a material's alpha / base colour / shading normal /
 * attenuation, 3 a BSDF's f, pdf and sample, 4 a light's sample, pdf, Le and selection probability, 5 the light sampler's
 * choice), word 1 the texture / material / light index, word 2 bit 0 `regularized`, words 4..31 the float operands.
 * form is a bit set: 1 the functions receive the LDS copy of the glossy lobes' GGX tables that the shade kernel builds (the
 * first LutDev::glassE floats and, behind them, the tables' address for the glass lookups); 2 the material, texture, light,
 * environment and infinite-light tables are LDS copies where they fit the shade kernel's slots (kShade*Slots); 4 a BSDF case
 * goes through one matEvaluate and bsdfSampleImplE / bsdfFImplE / bsdfPdfImplE in the local frame, as the wavefront shade
 * stage calls them, instead of bsdfSample / bsdfF / bsdfPdf. Whether textures are read through 2x2 footprint records is a
 * property of the scene (YART_TEX_QUADS_MAX_MB at creation).
 * Everything is checked before a device is touched — YART_E_INVALID for a null pointer, an unknown kind or form bit, an index
 * at or above the scene's count, an operand that is not finite, a PICK case in a scene without lights or whose u lies outside [0, 1), a TEX case on a texture
 * that has no footprint records of its own in a scene that uses them, n above 2^20 — so that no case makes a lane read outside
 * the scene. */
int yart_hip_probe_shading(YartScene* scene, uint32_t n, const uint32_t* cases, uint32_t form, uint32_t* out);
/* Diagnostic: the camera ray of n (x, y, sample) triples -> 6 floats each (origin, direction), drawn exactly as bounce 0 of that
 * sample draws it: startPixelSample, the film and the lens draw (core/sampler.hpp), Camera::getRay (core/camera.hpp:138-164) */
int yart_hip_probe_camera_rays(YartScene* scene, const YartCameraDesc* cam, const YartRenderParams* params, uint32_t n,
                               const uint32_t* xys, float* out_rays);
/* the BVH the kernels traverse: nodes (8 x u32 each: bounds, left|first, span) and
 * the index permutation of mesh `mesh` */
/* the 32 device counter words of the last render on this scene ([0] rays, [1..4] exact
 * traversal tallies in the instrumented build, [8..] kernel-phase statistics in debug builds) */
int yart_hip_debug_counters(YartScene* scene, uint64_t* out32);
/* diagnostic read-back of what yart_hip_scene_update re-derives, from the device: the NodeDev records (176 bytes per node), the
 * nodeWorld pairs (8 floats per node), the TlasNode records (32 bytes each; *n_tlas_out of them, 0 for a scene of fewer than 64
 * nodes; room for 2 * nodes - 1). Any output pointer may be NULL. */
int yart_hip_probe_scene_graph(YartScene* scene, void* nodes_out, float* node_world_out, void* tlas_out, uint32_t* n_tlas_out);
/* diagnostic read-back of one mesh as the kernels see it, from the device (not from the library's host copy): its MeshDev record
 * (64 bytes: nodeOffset, leafOffset, triOffset, vertOffset, nTris, nVerts, nNodes, hasAlpha, 8 unused words), its nNodes BvhNode records
 * (32 bytes; the link words with alpha and span bits), its nTris LeafTri (48 bytes) and ShadeTri (128 bytes) records, its nVerts
 * vPos / vNormal / vTangent entries (4 floats each), and the scene's current traversal stack bound. Any output pointer may be NULL:
 * a first call with mesh_dev_out alone gives the counts the arrays need. */
int yart_hip_probe_mesh(YartScene* scene, uint32_t mesh, void* mesh_dev_out, void* nodes_out, void* leaf_out, void* shade_out, float* vpos_out,
                        float* vnormal_out, float* vtangent_out, uint32_t* stack_bound_out);
/* diagnostic read-back of what yart_hip_scene_update_lighting re-derives, from the device (not from the library's host copy). The
 * caller sets struct_size; the call fills in every count (elements of the arrays below, as the device holds them: padded to at least
 * one) and total_power, and copies into every array pointer that is not NULL — a first call with all of them NULL gives the sizes.
 * materials: MaterialDev records (176 bytes); mat_class: the lobe-class bytes (padded to a multiple of 4); lights: LightDev records
 * (176 bytes); envs: EnvDev records (48 bytes: w, h, funcOffset, cdfOffset, rowIntOffset, margCdfOffset, margIntegral, surfaceArea,
 * guideOffset, guideKw, guideKh, pairOffset); env_data / env_guide: the image lights' tables; area_power_cdf; tex_f32: the float
 * texels; tex_quads: the footprint-record array in bytes (n_tex_quad_bytes = 0 where the scene has none; bytes that belong to no
 * record are unspecified); textures: TexDev records (32 bytes: offset, width, height, channels, type, isFloat, quadOffset in 16-byte
 * units or 0xffffffff, quadStride), which say where a texture's texels and records lie. */
typedef struct YartLightingProbe {
  uint32_t struct_size;              /* sizeof(YartLightingProbe) */
  float total_power;
  uint64_t n_materials, n_mat_class, n_lights, n_envs, n_env_data, n_env_guide, n_area_power_cdf, n_tex_f32, n_tex_quad_bytes, n_textures;
  void* materials; uint8_t* mat_class; void* lights; void* envs; float* env_data; uint32_t* env_guide; float* area_power_cdf;
  float* tex_f32; uint8_t* tex_quads; void* textures;
} YartLightingProbe;
int yart_hip_probe_lighting(YartScene* scene, YartLightingProbe* probe);
/* the host part of an image replacement on its own (measurements): the three sequential binary32 sums over n_texels RGB texels in
 * row-major order, as scene creation and yart_hip_scene_update_lighting take them for an image light's average radiance */
int yart_hip_probe_texel_sum(const float* pixels, uint64_t n_texels, float* sum3_out);
/* diagnostic read-back of the 8-bit texels, from the device (not from the library's host copy), for yart_hip_scene_update_textures.
 * The caller sets struct_size; the call fills in both counts and copies into every array pointer that is not NULL — a first call with
 * both NULL gives the sizes. tex_u8: the byte array of all 8-bit textures (each padded to a multiple of 4 bytes; at least one
 * element); textures: TexDev records (32 bytes, as in YartLightingProbe), the entries creation adds for bundles included. */
typedef struct YartTexturesProbe {
  uint32_t struct_size;              /* sizeof(YartTexturesProbe) */
  uint64_t n_tex_u8, n_textures;
  uint8_t* tex_u8; void* textures;
} YartTexturesProbe;
int yart_hip_probe_textures(YartScene* scene, YartTexturesProbe* probe);
/* diagnostic read-back of the geometry pools as the kernels see them, from the device (not from the library's host copy), for
 * yart_hip_scene_replace_meshes. The caller sets struct_size; the call fills in stack_bound (the scene's current traversal stack
 * bound) and every count — from the meshes' layout, not from the capacity of a buffer — and copies into every array pointer that is
 * not NULL: a first call with all of them NULL gives the sizes. bvh_nodes: BvhNode records (32 bytes) of all meshes, the zero pad
 * records in front of the meshes and the two behind the last included; leaf_tris: LeafTri (48 bytes); shade_tris: ShadeTri (128
 * bytes); tri_verts: 4 words per triangle; tri_light: 1 word; vpos / vnormal / vtangent: 4 floats per vertex; vuv: 2 floats;
 * meshes: MeshDev records (64 bytes, as in yart_hip_probe_mesh). */
typedef struct YartGeometryProbe {
  uint32_t struct_size;              /* sizeof(YartGeometryProbe) */
  uint32_t stack_bound;
  uint64_t n_bvh_nodes, n_leaf_tris, n_shade_tris, n_tri_verts, n_tri_light, n_vpos, n_vnormal, n_vtangent, n_vuv, n_meshes;
  void* bvh_nodes; void* leaf_tris; void* shade_tris; uint32_t* tri_verts; int32_t* tri_light; float* vpos; float* vnormal;
  float* vtangent; float* vuv; void* meshes;
} YartGeometryProbe;
int yart_hip_probe_geometry(YartScene* scene, YartGeometryProbe* probe);
/* measurement builds (-DYART_SHADE_REGIONS=1, tools/shade_regions.py) only: wave cycles [0..15], visits [16..31] and
 * active lanes [32..47] per code region of the shade kernel since the last call; YART_E_INVALID in the product build */
int yart_hip_debug_shade_regions(uint64_t* out48);
int yart_hip_bvh_info(YartScene* scene, uint32_t mesh, uint32_t* n_nodes, uint32_t* n_tris);
/* The reference's binned-SAH build (core/bvh.hpp:41-184, 273-347) of one mesh, outside a scene: on the device
 * (csrc/bvh_build_device.inc: level by level, one workgroup per node, the sequential partition in closed form) and on
 * the host (csrc/bvh_build_host = csrc/bvh_build.hpp, `threads` workers, 0 = all). Both write the reference's node array
 * (8 words per node: bounds, left|first, span; room for 2 * n_faces nodes) and index permutation, byte for byte the
 * same. faces: n_faces x face_stride words, the first three of each the vertex indices. The device build refuses input
 * with NaN coordinates or a tree deeper than 192 levels (YART_E_INVALID): build those on the host. */
int yart_hip_bvh_build_device(int device, const float* positions, uint32_t n_verts, const uint32_t* faces, uint32_t face_stride,
                              uint32_t n_faces, uint32_t* nodes_out, uint32_t* indices_out, uint32_t* n_nodes, double* ms_device);
int yart_hip_bvh_build_host(const float* positions, uint32_t n_verts, const uint32_t* faces, uint32_t face_stride, uint32_t n_faces,
                            uint32_t threads, uint32_t* nodes_out, uint32_t* indices_out, uint32_t* n_nodes, double* ms_host);
int yart_hip_bvh_copy(YartScene* scene, uint32_t mesh, uint32_t* nodes_out, uint32_t* indices_out);
/* The top-level hierarchy of a node list, outside a scene: on the device (csrc/tlas_build_kernels.inc, what
 * YART_UPDATE_REBUILD_TOP_DEVICE runs) and on the host (host_scene.hpp::buildTopLevel, what scene creation runs); byte for byte the
 * same records. node_world: n_nodes x 8 floats, the nodes' padded world boxes as lo.xyz, -, hi.xyz, - (the fourth words are
 * ignored); mesh: per node, < 0 = not a mesh node. tlas_out: room for 2 L - 1 records of 32 bytes (lo[3], a, hi[3], b), L the number
 * of mesh nodes. n_nodes < 64 or L = 0 gives 0 records, as scene creation does. YART_E_INVALID: a NULL pointer, n_nodes >= 2^20.
 * Outside the contract: a bound that is a NaN, and a bound that is +0 on one mesh node and -0 on another.
 * yart_hip_tlas_build_launches: the kernel launches the device build makes for L mesh nodes. */
int yart_hip_tlas_build_device(int device, const float* node_world, const int32_t* mesh, uint32_t n_nodes, void* tlas_out,
                               uint32_t* n_tlas_out, uint32_t* height_out);
int yart_hip_tlas_build_host(const float* node_world, const int32_t* mesh, uint32_t n_nodes, void* tlas_out, uint32_t* n_tlas_out,
                             uint32_t* height_out);
int yart_hip_tlas_build_launches(uint32_t n_leaves);

/* The step after the path: AgX tonemap of the RGBA32F frame as
 * cpu/tile-renderer.hpp:234-237 applies it per tile (core/tonemapping.hpp:14-92; look 0 none, 1 golden,
 * 2 punchy; alpha = 1), and the 8-bit encoding of output/ppm.cpp:7-21 (gamma 1/2.2, * 255.999, truncated;
 * 3 bytes per pixel, row-major, no header). Device buffers; the calls return after completion on `stream`. */
int yart_hip_tonemap_agx(const float* d_hdr_rgba, uint32_t width, uint32_t height, int look, float* d_ldr_rgba,
                         void* stream);
int yart_hip_encode_rgb8(const float* d_rgba, uint32_t width, uint32_t height, uint8_t* d_rgb8, void* stream);
/* Host-buffer convenience: tonemap (look -1: none, as with a null tonemapper) + encode through the device;
 * ldr_rgba / rgb8 may be NULL. */
int yart_hip_tonemap_host(const float* hdr_rgba, uint32_t width, uint32_t height, int look, float* ldr_rgba,
                          uint8_t* rgb8);

/* The stage between yart_hip_render_aovs and yart_hip_tonemap_agx: an edge-avoiding à-trous wavelet filter (Dammertz, Sewtz,
 * Hanika, Lensch 2010) of the linear-HDR RGBA32F frame, guided by any subset of the albedo, normal and depth feature buffers
 * (3 / 3 / 1 floats per pixel, as YartAovBuffers holds them; NULL: that guide is not used), entirely on the device.
 * DEFINITION. Every operation is an individually rounded binary32 operation in the order written (no FMA contraction); expf and
 * logf have glibc's values (csrc/ymath.hpp yexpf / ylogf). csrc/denoise.hpp states it; yart_amd/denoise.py atrous_reference is
 * the NumPy statement the tests compare with, on bits.
 *   Prepare, once per pixel p:
 *     alb      = albedo(p) with YART_DENOISE_DEMODULATE, else (1, 1, 1) (the albedo buffer is not read at all then)
 *     d        = alb > 1e-3f ? alb : 1.0f                      per channel
 *     c_0(p)   = rgb(p) / d                                    per channel
 *     n(p)     = normal(p);  lz(p) = logf(depth(p) > 1e-30f ? depth(p) : 1e-30f)          (each only if that buffer is given)
 *     valid(p) = every component of c_0(p) is finite, and of albedo(p) when demodulating, and of normal(p) and depth(p) where given
 *   Iteration i = 0 .. iterations-1, step s = 1 << i, from image c_i to c_(i+1):
 *     acc = (0, 0, 0); wsum = 0
 *     for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner):  q = p + s * (dx, dy)
 *       q outside the image: skipped (no clamping, no mirroring);  !valid(q): skipped
 *       h  = k[|dy|] * k[|dx|],  k = {0.375f, 0.25f, 0.0625f}
 *       dc = (dr * dr + dg * dg) + db * db   over c_i(q) - c_i(p);   dn the same over n(q) - n(p);   dl = lz(q) - lz(p)
 *       e  = (dc * icol_i + dn * inrm) + (dl * dl) * idep
 *              icol_i = icol * float(1u << (2 * i)) (the colour sigma halves with every iteration); icol = 1.0f / (sigma_color *
 *              sigma_color), inrm and idep likewise from their sigmas, each formed once on the host in fp32.
 *              A term whose sigma is <= 0 or whose buffer is not given does not exist: e is the sum of the others, in this order
 *              and association (colour and depth only: dc * icol_i + (dl * dl) * idep); no term at all: e = 0.0f.
 *              !valid(p): e = 0.0f for every tap (the pixel is filled from its valid neighbours; it is no tap of anyone's, its
 *              own included, in any iteration).
 *       w  = h * expf(-e)
 *       acc.r = acc.r + w * c_i(q).r   (a multiply, then an add; g and b likewise);   wsum = wsum + w
 *     c_(i+1)(p) = acc / wsum per channel; (0, 0, 0) if wsum == 0
 *   Finish: out.rgb(p) = c_iterations(p) * d per channel, out.a(p) = in.a(p).
 * iterations == 0 copies the frame (no demodulation round trip). out may be the input frame; it may not overlap a guide buffer.
 * Memory: 48 bytes per pixel while the call runs — two working-colour images and the guide records {n, lz}, 16 bytes each, allocated
 * and freed by the library; d is not stored (the finish pass forms it again from the albedo buffer, which the call never writes).
 * The defaults are the sigmas with the smallest worst-case error over host renders of the two golden scenes, 16 spp filtered against
 * 1024 spp, all guides, demodulated (profiles/denoise_sigma_sweep.txt: RMSE 0.60 / 0.85 of the unfiltered frame's). */
#define YART_DENOISE_DEMODULATE 1u          /* divide the frame by the albedo before filtering, multiply after (needs albedo) */
#define YART_DENOISE_DEFAULT_ITERATIONS 5u
#define YART_DENOISE_DEFAULT_SIGMA_COLOR 0.5f
#define YART_DENOISE_DEFAULT_SIGMA_NORMAL 0.5f
#define YART_DENOISE_DEFAULT_SIGMA_DEPTH 0.3f
typedef struct YartDenoiseParams {
  uint32_t struct_size;        /* sizeof(YartDenoiseParams): lets the struct grow without an ABI bump */
  uint32_t iterations;         /* 0 .. 8 */
  float sigma_color, sigma_normal, sigma_depth;   /* finite; <= 0: that term is left out */
  uint32_t flags;              /* YART_DENOISE_* */
} YartDenoiseParams;
/* DEVICE pointers (e.g. torch tensors' data_ptr) on `stream` (hipStream_t, may be NULL); returns after completion on that stream.
 * YART_E_INVALID, with a message and before any device is touched: a NULL d_rgba, d_out_rgba or params; a struct_size smaller than
 * YartDenoiseParams; iterations > 8; a width or height of 0 (or more than 2^28 pixels); a sigma that is not finite; unknown flags
 * bits; YART_DENOISE_DEMODULATE without d_albedo. YART_E_NO_DEVICE without a HIP device. */
int yart_hip_denoise_atrous_device(const float* d_rgba, const float* d_albedo, const float* d_normal, const float* d_depth,
                                   uint32_t width, uint32_t height, const YartDenoiseParams* params, float* d_out_rgba,
                                   void* stream);
/* Same, HOST pointers: the buffers are copied to the current device, filtered there and the frame copied back. */
int yart_hip_denoise_atrous_host(const float* rgba, const float* albedo, const float* normal, const float* depth, uint32_t width,
                                 uint32_t height, const YartDenoiseParams* params, float* out_rgba);

/* The variance-guided form of the filter above — the spatial filter of SVGF (Schied, Kaplanyan, Wyman, Patney, Chaitanya, Burgess,
 * Liu, Dachsbacher, Lefohn, Salvi 2017) — with the per-pixel variance of yart_hip_render_moments (YART_MOMENT_VARIANCE) as a fourth
 * input: a colour difference is measured against the local standard deviation of the luminance instead of one global sigma_color, and
 * the variance is filtered along. It is the DEFINITION above with these changes and nothing else (csrc/denoise.hpp dnPrepare<true> /
 * dnFilterPixel<true> state it; yart_amd/denoise.py atrous_var_reference is the NumPy statement the tests compare with, on bits):
 *   Prepare:   v_0(p) = variance(p) / (ld * ld), ld = luma(d) = (d.r * 0.2126f + d.g * 0.7152f) + d.b * 0.0722f of the demodulation
 *              divisor d ((1, 1, 1) when not demodulating). valid(p) additionally requires variance(p) to be finite and >= 0.
 *   Iteration, once per centre pixel p:  g(p) = the 3 x 3 Gaussian of v_i around p, ALWAYS at distance 1: weights k3[|dy|] * k3[|dx|],
 *              k3 = {0.5f, 0.25f} (0.25f centre, 0.125f edge, 0.0625f corner), over the valid pixels inside the image, dy outer, dx
 *              inner: gv = gv + k * v_i(q), gk = gk + k; g = gv / gk, 0.0f if no tap counts.
 *   Colour term of e:  fabsf(ly(q) - ly(p)) / (sigma_luma * sqrtf(g(p)) + 1e-6f), ly = luma(c_i), in place of dc * icol_i: no 4^i
 *              scaling (the filtered variance shrinks instead). The normal and depth terms, their order, the association of e, the
 *              rule that a term whose sigma is <= 0 does not exist, and the handling of invalid pixels are unchanged.
 *   Variance:  vacc = vacc + (w * w) * v_i(q) next to acc; v_(i+1)(p) = vacc / (wsum * wsum), 0.0f if wsum == 0.
 *   Finish:    unchanged (the filtered variance is not returned).
 * Memory: 48 bytes per pixel while the call runs, as above: v_i lives in the fourth word of the working colour, where the plain
 * filter keeps the valid flag. The defaults are the minimiser of the worst case over the same two host renders
 * (profiles/denoise_var_sweep.txt: RMSE 0.42 / 0.64 of the unfiltered frame's, where the plain filter at its defaults reaches 0.60 / 0.85
 * on the same inputs). */
#define YART_DENOISE_VAR_DEFAULT_ITERATIONS 3u
#define YART_DENOISE_VAR_DEFAULT_SIGMA_LUMA 2.0f
#define YART_DENOISE_VAR_DEFAULT_SIGMA_NORMAL 0.25f
#define YART_DENOISE_VAR_DEFAULT_SIGMA_DEPTH 0.1f
typedef struct YartDenoiseVarParams {
  uint32_t struct_size;        /* sizeof(YartDenoiseVarParams) */
  uint32_t iterations;         /* 0 .. 8 */
  float sigma_luma, sigma_normal, sigma_depth;    /* finite; <= 0: that term is left out */
  uint32_t flags;              /* YART_DENOISE_* */
} YartDenoiseVarParams;
/* DEVICE pointers on `stream`; returns after completion on that stream. d_variance (width * height floats) is required; the other
 * argument errors are those of yart_hip_denoise_atrous_device: YART_E_INVALID with a message, before any device is touched. */
int yart_hip_denoise_atrous_var_device(const float* d_rgba, const float* d_variance, const float* d_albedo, const float* d_normal,
                                       const float* d_depth, uint32_t width, uint32_t height, const YartDenoiseVarParams* params,
                                       float* d_out_rgba, void* stream);
/* Same, HOST pointers */
int yart_hip_denoise_atrous_var_host(const float* rgba, const float* variance, const float* albedo, const float* normal,
                                     const float* depth, uint32_t width, uint32_t height, const YartDenoiseVarParams* params,
                                     float* out_rgba);

/* Temporal accumulation with camera reprojection — the temporal half of SVGF — for a SEQUENCE of frames of one scene: the stage
 * between yart_hip_render_moments and yart_hip_denoise_atrous_var_device. A scene is immutable after yart_hip_scene_create, so
 * between frames of ONE scene only the camera moves: the position buffer (world-space Hit.p) and the previous frame's
 * YartCameraDesc are a complete motion description, and no render kernel takes part. A caller who animates geometry re-creates the
 * scene per frame with other YartNodeDesc::fwd / inv and says how each node moved with yart_hip_temporal_set_motion (below, PER-NODE
 * MOTION). Per frame the accumulator takes the frame, its
 * variance (YART_MOMENT_VARIANCE), its feature buffers and its camera; it projects every pixel's surface point into the previous
 * frame's camera, fetches the accumulated history there with a validated bilinear tap set, blends, and returns the accumulated
 * frame, the variance of that estimate and the history length per pixel. Frame and variance are what the variance-guided filter takes.
 * The handle holds the history for one image size on one device: two images (the pass reads neighbours of one while it writes the
 * other) of three 16-byte records per pixel — {acc.rgb, variance}, {P.xyz, length}, {n.xyz, node} — 96 BYTES PER PIXEL, allocated
 * by the first accumulate call (yart_hip_temporal_create touches no device), and the YartCameraDesc of the last accumulated frame.
 * DEFINITION. Every operation is an individually rounded binary32 operation in the order written (no FMA contraction); dot(a, b) is
 * (a.x * b.x + a.y * b.y) + a.z * b.z, cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); only
 * + - * /, floorf and comparisons occur (and sqrtf, with a CLIP). csrc/temporal.hpp states it; yart_amd/temporal.py temporal_reference is the NumPy
 * statement the tests compare with, on bits.
 *   Current pixel p:
 *     d = alb > 1e-3f ? alb : 1.0f per channel with YART_TEMPORAL_DEMODULATE (the filters' rule), else (1, 1, 1) (albedo is not read)
 *     c = rgb(p) / d per channel;  ld = luma(d) = (d.r * 0.2126f + d.g * 0.7152f) + d.b * 0.0722f;  v = variance(p) / (ld * ld)
 *     usable(p)        every component of c is finite, and of albedo(p) when demodulating; variance(p) is finite and >= 0; v is finite
 *     reprojectable(p) usable(p), coverage(p) == 1.0f, and position(p), normal(p) and depth(p) are finite. (The feature buffers are
 *                      sums over the hitting samples divided by `samples`: position is a surface point only where every sample hit.)
 *     !usable(p): out_rgba(p) = rgba(p) and out_variance(p) = variance(p), the input bits; out_length(p) = 0; the pixel's history
 *                      record is all zero — length 0 — and is nobody's tap.
 *   Projection of P = position(p) through the PREVIOUS camera's lens centre onto its focus plane, with the derived quantities of
 *   Camera::calcDerivedProperties (position, topLeftPixel tl, pixelDeltaU dU, pixelDeltaV dV), formed as the renderer forms them:
 *     nrm = cross(dU, dV);  num = dot(tl - position, nrm);  rel = P - position;  s = num / dot(rel, nrm)
 *     in front of the camera iff s > 0.0f and s <= FLT_MAX (the denominator has num's sign and is not 0); else no tap counts
 *     X = (position + rel * s) - tl;  jx = dot(X, dU) / dot(dU, dU);  jy = dot(X, dV) / dot(dV, dV)
 *     (jx, jy) is in the units of Camera::getRay's jitter: pixel (px, py)'s centre is (float(px), float(py)), its gaussian jitter has mean 0.
 *     no tap counts unless -1.0f <= jx < float(width) and -1.0f <= jy < float(height)
 *     x0 = floorf(jx), y0 = floorf(jy);  fx = jx - x0, fy = jy - y0;  taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), in
 *     this order, with the bilinear weights w = (fx or 1.0f - fx) * (fy or 1.0f - fy)
 *   A tap q COUNTS iff it is inside the image; its history length is >= 1; its node equals ids(p)[0]; dot(n(p), n_hist(q)) >=
 *     normal_cos_min; fabsf(dot(n(p), P_hist(q) - P)) <= plane_tolerance * depth(p); and its weight w > 0.0f (a tap of weight 0
 *     contributes nothing, so it neither shortens the length nor leaves a sum of weights of 0).
 *   Blend, sums over the counting taps in tap order starting from 0.0f (acc = acc + w * value):
 *     h = sum(w * c_hist) / sum(w) per channel;  v_h = sum(w * v_hist) / sum(w), the same weights — conservative on purpose:
 *     neighbouring history pixels are correlated;  N_h = the smallest length of the counting taps
 *     N = min(N_h + 1, max_history);  a = max(1.0f / float(N), alpha_min);  acc = h + a * (c - h) per channel
 *     v_acc = (a * a) * v + ((1.0f - a) * (1.0f - a)) * v_h
 *     No counting tap, p not reprojectable, or an empty history (first frame, or the first after a reset): acc = c, v_acc = v, N = 1.
 *   Outputs: out_rgba(p) = (acc * d, rgba(p).a);  out_variance(p) = v_acc * (ld * ld);  out_length(p) = N.
 *   New history record of p: {acc, v_acc}, {P, N}, {n(p), ids(p)[0]} — colour and variance in the demodulated domain.
 * The defaults minimise the worst case, over 6-frame orbits of the two golden scenes rendered by the host path tracer at 4 spp, of
 * the last frame's error against 1024 spp relative to not accumulating (tools/temporal_sweep.py, profiles/temporal_sweep.txt: RMSE
 * 0.60 / 0.71 of the last frame's alone on cornell / material; followed by the variance-guided filter, 0.91 of that filter's alone).
 * PER-NODE MOTION (yart_hip_temporal_set_motion). Node indices are stable across re-created scenes and ids(p)[0] is the node index.
 * A motion is one record per scene node: the map from THIS frame's world space to the PREVIOUS frame's for points rigidly attached
 * to that node, 24 floats read as six 16-byte words — {M row 0}, {M row 1}, {M row 2}: the 3 x 4 point transform; {Nm row 0, kind},
 * {Nm row 1, 0}, {Nm row 2, 0}: the 3 x 3 normal transform, kind a uint32 in word 15: 0 static (the other 23 words are ignored), 1
 * moving. The definition above changes for a MOVING pixel p only — a motion is pending, uint32(ids(p)[0]) < n_nodes, and that record's
 * kind == 1; any other pixel runs exactly the operations above (nothing is multiplied by an identity: -0 stays -0):
 *     P' = (dot(M row i .xyz, P) + M row i .w), i = 0 .. 2;   n' = (dot(Nm row i, n(p))), i = 0 .. 2   — the rules and the dot above
 *     reprojectable(p) additionally needs P' and n' finite;  the projection uses P' in place of P: rel = P' - position
 *     a tap q counts iff ... dot(n', n_hist(q)) >= normal_cos_min; fabsf(dot(n', P_hist(q) - P')) <= plane_tolerance * depth(p) ...
 *   Node equality, the weights, the blend, N, a, the moments and the new history record — {P, N}, {n(p), node}, the CURRENT values —
 *   are unchanged, and so is pass 2 of the moments form, which works on the new records only.
 * PER-PIXEL MOTION (yart_hip_temporal_set_pixel_motion): one record of 8 floats per pixel, two 16-byte words {P'.xyz, kind} and
 * {n'.xyz, 0}, as yart_hip_scene_pixel_motion_* writes them — for deforming meshes, which no per-node record describes. The
 * definition changes for a pixel whose record has kind == 1 and for no other, exactly as for a MOVING pixel above with P' and n'
 * taken from the record: reprojectable(p) additionally needs them finite, the projection and the tap tests use them; node
 * equality, the weights, the blend, N, the moments, the new record with the CURRENT P and n, and pass 2 are untouched. A pixel
 * whose kind is not 1 runs the operations it ran before.
 * CLIP (yart_hip_temporal_set_clip): variance clipping of the history against ghosting. Geometry alone validates a tap, so a light
 * that moves or dims, or a shadow that crosses a static wall, leaves every tap valid and the stale colour in the blend. With a clip
 * set, the fetched history colour is clipped, per channel, to mean +- gamma * standard deviation of the current frame's
 * demodulated colour over the (2 radius + 1)^2 window around p: history the frame supports passes untouched, the rest is pulled to
 * the edge of what the frame supports. Under the rules above; sqrtf is the correctly rounded binary32 square root (the only
 * operation the clip adds to + - * /, floorf and comparisons). The definition changes for a usable pixel p WITH A COUNTING TAP SET,
 * after h (and h1, h2 in the moments form) is formed and before the blend; a pixel without a counting tap, a first frame and an
 * unusable pixel produce the bits they produce without a clip:
 *     window: dy = -radius .. radius outer, dx = -radius .. radius inner. A neighbour q COUNTS iff it is inside the image, every
 *     component of c(q) = rgb(q) / d(q) is finite, and, when demodulating, every component of albedo(q) is finite. (variance(q)
 *     plays no part; p itself is a neighbour like any other.)
 *     over the counting neighbours, from 0.0f and 0, per channel: s1 = s1 + c(q);  s2 = s2 + c(q) * c(q);  k = k + 1
 *     k < 2: nothing is clipped. Otherwise, per channel:
 *       mu = s1 / float(k);  e2 = s2 / float(k);  var = e2 - mu * mu;  var = var > 0.0f ? var : 0.0f;  sd = sqrtf(var)
 *       lo = mu - gamma * sd;  hi = mu + gamma * sd
 *       mu, e2 and sd all finite: h = h < lo ? lo : (h > hi ? hi : h);  otherwise the channel is left alone (an overflowing c * c
 *       would clip to infinity — or, where mu * mu overflows with it, var is NaN, sd 0, and it would clip to a huge mu)
 *     N, a, v_h, hw2, the history length and the tap tests are unchanged.
 *   The moments form, additionally: the same sums for y(q) = luma(c(q)) give mu_y, e2_y and sd_y; with all three finite, h1' = h1 clipped the
 *     same way, and if h1' != h1: h2 = h2 + (h1' * h1' - h1 * h1), then h1 = h1' — the history's luminance distribution is translated,
 *     so its temporal variance h2 - h1 * h1 is kept. Pass 2 is untouched.
 *   The defaults minimise, over radius 1 .. 3 x gamma {0.5, 1, 1.5, 2, 3}, the worst case over the 6-frame orbits of the two golden
 *   scenes, unchanged and with every emitter dimmed to a quarter from frame 4 on, of the last frame's error against 1024 spp relative
 *   to the better of unclipped accumulation and not accumulating (tools/temporal_clip_sweep.py, profiles/temporal_clip_sweep.txt:
 *   radius 1, gamma 0.5; 0.93 / 0.98 of the unclipped RMSE on the unchanged orbits of cornell / material, and after the dimming 1.08
 *   of the last frame's alone on cornell, where unclipped accumulation is at 4.4, and 0.75 on material).
 * Out of scope: screen-space motion-vector output, a wider search when all four taps fail, yart_hip_multi_*. */
#define YART_TEMPORAL_DEMODULATE 1u         /* accumulate rgb / d, return acc * d (needs YART_AOV_ALBEDO) */
#define YART_TEMPORAL_DEFAULT_ALPHA_MIN 0.1f
#define YART_TEMPORAL_DEFAULT_MAX_HISTORY 8u
#define YART_TEMPORAL_DEFAULT_NORMAL_COS_MIN 0.8f
#define YART_TEMPORAL_DEFAULT_PLANE_TOLERANCE 0.01f
typedef struct YartTemporalParams {
  uint32_t struct_size;        /* sizeof(YartTemporalParams): lets the struct grow without an ABI bump */
  float alpha_min;             /* 0 .. 1: the smallest weight of the new frame */
  uint32_t max_history;        /* >= 1: the cap of the history length */
  float normal_cos_min;        /* finite */
  float plane_tolerance;       /* finite; relative to the pixel's depth */
  uint32_t flags;              /* YART_TEMPORAL_* */
} YartTemporalParams;
typedef struct YartTemporal YartTemporal;
/* width, height > 0 (at most 2^28 pixels); device < 0: the device current at the first accumulate call. No device is touched. */
int yart_hip_temporal_create(uint32_t width, uint32_t height, int device, YartTemporal** out);
void yart_hip_temporal_destroy(YartTemporal* temporal);
/* Forget the history: the next frame is a first frame. A pending motion (per node or per pixel) is forgotten too. */
int yart_hip_temporal_reset(YartTemporal* temporal);
/* Per-node motion for the NEXT accumulate call on the handle (PER-NODE MOTION above). The records are copied into the handle and no
 * device is touched. The motion applies to the next accumulate call — either form, device or host entry — that passes its own
 * argument checks; that call uploads the records on its stream before its kernel and consumes the motion: the call after it runs
 * without one. motion == NULL clears a pending motion, as yart_hip_temporal_reset does.
 * YART_E_INVALID, with a message and nothing left pending: a NULL temporal; a struct_size smaller than YartTemporalMotion; n_nodes
 * of 0 or >= 2^20; NULL records; a kind other than 0 or 1; a word of a kind == 1 record that is not finite. */
typedef struct YartTemporalMotion {
  uint32_t struct_size;        /* sizeof(YartTemporalMotion) */
  uint32_t n_nodes;            /* 1 .. 2^20 - 1 */
  const float* records;        /* HOST, n_nodes * 24 floats */
} YartTemporalMotion;
int yart_hip_temporal_set_motion(YartTemporal* temporal, const YartTemporalMotion* motion);
/* Per-pixel motion for the NEXT accumulate call on the handle (PER-PIXEL MOTION above). records: width * height * 8 floats in the
 * address space of the accumulate call that consumes them — a DEVICE pointer (16-byte aligned; written on that call's stream or
 * complete before it) for the _device entries, a HOST pointer for the _host entries. They are NOT copied: they must stay valid until
 * that call returns. Pending and consumed exactly as yart_hip_temporal_set_motion's: the records apply to the next accumulate call
 * of either form that passes its checks (a _device call refuses misaligned records with YART_E_INVALID and leaves them pending);
 * motion == NULL clears; yart_hip_temporal_reset clears. ONE motion is pending at a time: each of the two setters replaces whatever
 * the other left. No device is touched.
 * YART_E_INVALID, with a message and nothing left pending: a NULL temporal; a struct_size smaller than YartTemporalPixelMotion; NULL
 * records. */
typedef struct YartTemporalPixelMotion {
  uint32_t struct_size;        /* sizeof(YartTemporalPixelMotion) */
  const float* records;        /* width * height * 8 floats, in the consuming call's address space */
} YartTemporalPixelMotion;
int yart_hip_temporal_set_pixel_motion(YartTemporal* temporal, const YartTemporalPixelMotion* motion);
/* The clip of the history to the frame's neighbourhood (CLIP above): a SETTING of the handle. It touches no device; it stays set
 * across accumulate calls — both forms, every motion, device and host entries — and across yart_hip_temporal_reset until it is set
 * again; clip == NULL turns it off. A new handle has no clip, and without one every call runs the code and produces the bits it
 * did before there was a clip. With a clip the kernel reads the neighbours' d_rgba, so a _device call whose d_out_rgba is d_rgba
 * first copies the frame, on the call's stream, into a staging buffer the handle owns (16 bytes per pixel, allocated on first need).
 * YART_E_INVALID, with a message and the previous setting kept: a NULL temporal; a struct_size smaller than YartTemporalClip; a
 * radius outside 1 .. 3; a gamma that is not finite or is negative. */
#define YART_TEMPORAL_DEFAULT_CLIP_RADIUS 1u
#define YART_TEMPORAL_DEFAULT_CLIP_GAMMA 0.5f
typedef struct YartTemporalClip {
  uint32_t struct_size;        /* sizeof(YartTemporalClip) */
  uint32_t radius;             /* 1 .. 3: the window is (2 radius + 1)^2 */
  float gamma;                 /* finite, >= 0 */
} YartTemporalClip;
int yart_hip_temporal_set_clip(YartTemporal* temporal, const YartTemporalClip* clip);
/* One frame. DEVICE pointers on `stream` (hipStream_t, may be NULL); returns after completion on that stream. d_rgba: width * height
 * * 4 floats; d_variance: width * height; d_aovs: position, normal, depth, coverage and ids are required (and albedo with
 * YART_TEMPORAL_DEMODULATE), as yart_hip_render_moments_device fills them; buffers of other mask bits are not touched.
 * d_out_variance (width * height floats) and d_out_length (width * height uint32) may each be NULL. d_out_rgba may be d_rgba and
 * d_out_variance may be d_variance; the outputs may not overlap any other input.
 * YART_E_INVALID, with a message and before any device is touched: a NULL temporal, cam, d_rgba, d_variance, d_aovs, params or
 * d_out_rgba; a struct_size smaller than YartTemporalParams; unknown flags bits; a parameter that is not finite; alpha_min outside
 * [0, 1]; max_history of 0; a camera whose width / height are not the handle's (or with a focal length <= 0); a required feature
 * buffer missing from d_aovs->mask (or NULL, or beyond its struct_size). YART_E_NO_DEVICE without a HIP device. */
int yart_hip_temporal_accumulate_device(YartTemporal* temporal, const YartCameraDesc* cam, const float* d_rgba, const float* d_variance,
                                        const YartAovBuffers* d_aovs, const YartTemporalParams* params, float* d_out_rgba,
                                        float* d_out_variance, uint32_t* d_out_length, void* stream);
/* Same, HOST pointers: the buffers are copied to the handle's device, accumulated there (the history stays on the device) and the
 * outputs copied back. */
int yart_hip_temporal_accumulate_host(YartTemporal* temporal, const YartCameraDesc* cam, const float* rgba, const float* variance,
                                      const YartAovBuffers* aovs, const YartTemporalParams* params, float* out_rgba,
                                      float* out_variance, uint32_t* out_length);

/* THE MOMENTS FORM of the temporal accumulation — SVGF's variance estimation (Schied et al. 2017, section 4.2) — on the same
 * YartTemporal handle. The variance the plain form propagates is the within-pixel sample variance of yart_hip_render_moments, which
 * is 0.0f by definition at 1 spp and has samples - 1 degrees of freedom otherwise. This form estimates the variance of the
 * accumulated colour's luminance from the frames themselves: per pixel it accumulates, next to the colour, the first and second
 * moment of the luminance and the sum of the squared frame weights (temporal estimate), and a pixel whose history is too short —
 * a disocclusion, the first frames after a reset — takes the variance of its 7 x 7 neighbourhood on the same surface (spatial
 * estimate). Frame and length are those of the plain form, bit for bit; only the variance differs.
 * A handle is in ONE FORM from its first accumulate after create or reset: calling the other form before yart_hip_temporal_reset is
 * YART_E_INVALID. In the moments form the history has a fourth plane of 16-byte records per image, rec3 = {m1, m2, w2, 0}: 128 BYTES
 * PER PIXEL, allocated by the first moments-form call; a plain-form handle still allocates 96.
 * DEFINITION, in the terms and under the rules of the plain form's (every operation an individually rounded binary32 operation in
 * the order written, no FMA contraction; only + - * /, floorf, comparisons and integer min / max: no libm). csrc/temporal.hpp
 * states it (tpAccumulatePixel<true>, tpSpatialVariance); yart_amd/temporal.py temporal_moments_reference is the NumPy statement.
 *   PASS 1, per pixel p: the plain form — usable / reprojectable, projection, tap set, tap validation, N, a, the colour blend and
 *   out_rgba / out_length are unchanged — and additionally, with y = luma(c) = (c.r * 0.2126f + c.g * 0.7152f) + c.b * 0.0722f:
 *     with a counting tap set: h1, h2, hw2 = sum(w * m1_hist) / sum(w), sum(w * m2_hist) / sum(w), sum(w * w2_hist) / sum(w), the
 *       weights, tap order and sum of weights of h;  m1 = h1 + a * (y - h1);  m2 = h2 + a * (y * y - h2);
 *       w2 = (a * a) * 1.0f + ((1.0f - a) * (1.0f - a)) * hw2
 *     without one: m1 = y, m2 = y * y, w2 = 1.0f.   A pixel that is not usable writes an all-zero rec3.
 *     w2 is the sum of the squared weights the frames have in acc: 1/N for an equal-weight history, and still right when the
 *     alpha_min floor or the max_history cap binds.
 *     vt = m2 - m1 * m1;  vt = vt > 0.0f ? vt : 0.0f
 *     N >= min_moment_history and w2 < 1.0f:  v_acc = vt * (w2 / (1.0f - w2)) — the unbiased weighted-sample estimate of the variance
 *       of acc's luminance, vt / (N - 1) for equal weights. The pixel is LONG.
 *     otherwise the pixel is SHORT, and pass 1 stores the plain form's v_acc = (a * a) * v + ((1.0f - a) * (1.0f - a)) * v_h (v
 *       without a counting tap) as a provisional value: d_variance is the last fallback.
 *   PASS 2, per SHORT pixel p, on the history image pass 1 wrote (a second kernel): over the 7 x 7 window around p, dy = -3 .. 3
 *   outer and dx = -3 .. 3 inner, a tap q COUNTS iff it is inside the image; its new length is >= 1; its node equals p's;
 *   dot(n(p), n(q)) >= normal_cos_min; fabsf(dot(n(p), P(q) - P(p))) <= plane_tolerance * depth(p) — the tap tests of pass 1, on
 *   the new records; the centre is a tap like any other. Over the counting taps, from 0.0f and 0: s1 = s1 + m1(q), s2 = s2 + m2(q),
 *   k = k + 1.
 *     k >= 2:  e1 = s1 / float(k);  e2 = s2 / float(k);  vs = e2 - e1 * e1;  vs = vs > 0.0f ? vs : 0.0f
 *              v_acc = (vs * (float(k) / float(k - 1))) * w2(p)
 *     k < 2:   the provisional value stays.
 *   out_variance(p) = v_acc * (ld * ld), and v_acc is the variance word of p's history record, in both passes.
 * min_moment_history is SVGF's 4; on the 6-frame orbits of the two golden scenes at 1 spp the moments form followed by the
 * variance-guided filter is closer to 1024 spp than the plain form followed by it (profiles/temporal_moments_sweep.txt). */
#define YART_TEMPORAL_DEFAULT_MIN_MOMENT_HISTORY 4u
typedef struct YartTemporalMomentParams {
  uint32_t struct_size;        /* sizeof(YartTemporalMomentParams) */
  float alpha_min;             /* the four of YartTemporalParams, with the same meaning and limits */
  uint32_t max_history;
  float normal_cos_min;
  float plane_tolerance;
  uint32_t min_moment_history; /* >= 2: below this history length the spatial estimate is used */
  uint32_t flags;              /* YART_TEMPORAL_DEMODULATE only */
} YartTemporalMomentParams;
/* One frame in the moments form. Arguments, aliasing rules and errors of yart_hip_temporal_accumulate_device (d_variance stays
 * required: the caller has it from yart_hip_render_moments), and YART_E_INVALID as well, before any device is touched, for a
 * struct_size smaller than YartTemporalMomentParams, a min_moment_history smaller than 2, and a handle whose history is in the plain
 * form (as the plain call refuses a handle whose history is in the moments form). */
int yart_hip_temporal_accumulate_moments_device(YartTemporal* temporal, const YartCameraDesc* cam, const float* d_rgba,
                                                const float* d_variance, const YartAovBuffers* d_aovs,
                                                const YartTemporalMomentParams* params, float* d_out_rgba, float* d_out_variance,
                                                uint32_t* d_out_length, void* stream);
/* Same, HOST pointers */
int yart_hip_temporal_accumulate_moments_host(YartTemporal* temporal, const YartCameraDesc* cam, const float* rgba, const float* variance,
                                              const YartAovBuffers* aovs, const YartTemporalMomentParams* params, float* out_rgba,
                                              float* out_variance, uint32_t* out_length);

/* The last stage of a sequence, after the denoiser: auto-exposure. A handle meters a linear-HDR RGBA32F frame on the device with a
 * log-luminance histogram, turns it into an exposure with eye-style temporal adaptation — the state stays on the device —, and
 * one kernel applies the gain, the AgX tonemap and the 8-bit encoding (what scale + yart_hip_tonemap_agx + yart_hip_encode_rgb8
 * do in three passes).
 * DEFINITION. Every operation is one individually rounded binary32 operation in the order written (no FMA contraction) unless it
 * says binary64; log2f and expf have glibc's values (csrc/tonemap.hpp ylog2f, csrc/ymath.hpp yexpf). csrc/exposure.hpp states
 * it; yart_amd/exposure.py exposure_reference / apply_reference are the NumPy statement the tests compare with, on bits. The
 * histogram has B = 256 bins, fixed.
 *   Formed once per call on the host:
 *     bins_per_ev = 256.0f / (ev_max - ev_min);   bin_width = (ev_max - ev_min) / 256.0f;   key_ev = log2f(key)
 *     a_up = 1.0f - expf(-(dt * speed_up));   a_down = 1.0f - expf(-(dt * speed_down))      dt: seconds since the previous frame
 *   Meter, for every pixel p of the metering window:
 *     Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b
 *     p is ignored (and counted in n_ignored) if r, g or b is not finite or if !(Y > 0); alpha is not read. Otherwise
 *     ev = log2f(Y);   t = (ev - ev_min) * bins_per_ev;   bin = t < 0 ? 0 : (t >= 256.0f ? 255 : uint32_t(t));   hist[bin] += 1
 *   Resolve:
 *     N = sum of hist;   lo = floor(double(trim_low) * N);   hi = N - floor(double(trim_high) * N)     (hi > lo whenever N >= 1)
 *     the bins in ascending order with a running count c:   k_b = |[c, c + hist[b]) n [lo, hi)|
 *       centre_b = ev_min + (float(b) + 0.5f) * bin_width;   S += double(k_b) * double(centre_b)      (binary64, ascending)
 *     K = hi - lo;   mean_ev = float(S / double(K))
 *     target = min(gain_ev_max, max(gain_ev_min, (key_ev - mean_ev) + compensation_ev))
 *   State (cur_ev, valid):
 *     N == 0:    cur_ev, target_ev, mean_ev, gain and frames stay as they are and YART_EXPOSURE_EMPTY is set in flags
 *     !valid (a new handle, or one after reset):   cur_ev = target, valid = 1
 *     otherwise: d = target - cur_ev;   cur_ev = cur_ev + d * (d > 0 ? a_up : a_down)
 *     then:      gain = expf(cur_ev * 0.6931472f);   frames += 1;   flags = 0
 *     n_counted = N and n_ignored are the last meter call's in every case.
 *   Apply, per pixel:  c = (r * gain, g * gain, b * gain);   look 0 .. 2: ldr = (AgX(c, look), 1);   look -1: ldr = (c, a);
 *     rgb8 = the 8-bit encoding (yart_hip_encode_rgb8's) of each ldr channel. gain is read from the handle's device record; a handle
 *     that has never metered (or was reset) applies gain 1.
 * The defaults below are conventions (a +-16 EV range, the middle 80 % of the counted pixels, the 18 % grey key, an eye that adapts
 * faster to light than to dark); nothing here is tuned.
 * Memory: per handle, on the device, the accumulating histogram and the last call's (1 KB each) and one 40-byte record, allocated by
 * the first call that needs a device. */
#define YART_EXPOSURE_EMPTY 1u              /* YartExposureState::flags: the last meter call counted no pixel */
#define YART_EXPOSURE_BINS 256u
#define YART_EXPOSURE_DEFAULT_EV_MIN (-16.0f)
#define YART_EXPOSURE_DEFAULT_EV_MAX 16.0f
#define YART_EXPOSURE_DEFAULT_TRIM_LOW 0.10f
#define YART_EXPOSURE_DEFAULT_TRIM_HIGH 0.10f
#define YART_EXPOSURE_DEFAULT_KEY 0.18f
#define YART_EXPOSURE_DEFAULT_COMPENSATION_EV 0.0f
#define YART_EXPOSURE_DEFAULT_GAIN_EV_MIN (-16.0f)
#define YART_EXPOSURE_DEFAULT_GAIN_EV_MAX 16.0f
#define YART_EXPOSURE_DEFAULT_SPEED_UP 3.0f
#define YART_EXPOSURE_DEFAULT_SPEED_DOWN 1.0f
typedef struct YartExposureParams {
  uint32_t struct_size;        /* sizeof(YartExposureParams) */
  float ev_min, ev_max;        /* the histogram's range: finite, ev_min < ev_max */
  float trim_low, trim_high;   /* the fractions of the counted pixels left out at either end: each in [0, 1), sum < 1 */
  float key;                   /* the luminance the mean is mapped to: finite, > 0 */
  float compensation_ev;       /* finite */
  float gain_ev_min, gain_ev_max;   /* the target's clamp: finite, min <= max */
  float speed_up, speed_down;  /* adaptation rates in 1/s towards a larger / smaller exposure: finite, >= 0 */
  uint32_t x0, y0, x1, y1;     /* the metering window, half open; all 0: the whole frame; else x0 < x1 <= width, y0 < y1 <= height */
} YartExposureParams;
typedef struct YartExposureState {
  uint32_t struct_size;        /* sizeof(YartExposureState), set by the caller */
  float cur_ev, target_ev, mean_ev, gain;
  uint32_t n_counted, n_ignored, frames, flags;   /* frames: the meter calls that counted a pixel since create / reset */
} YartExposureState;
typedef struct YartExposure YartExposure;
/* device < 0: the device current at the first call that needs one. No device is touched. */
int yart_hip_exposure_create(int device, YartExposure** out);
void yart_hip_exposure_destroy(YartExposure* exposure);
/* Back to a new handle: the next meter call snaps to its target, and until then apply uses gain 1. */
int yart_hip_exposure_reset(YartExposure* exposure);
/* Meter one frame (DEVICE pointer, 16-byte aligned) on `stream` (hipStream_t, may be NULL) and step the state by dt seconds; returns
 * after completion on that stream. YART_E_INVALID, with a message and before any device is touched: a NULL exposure, d_rgba or
 * params; a struct_size smaller than YartExposureParams; a width or height of 0 (or more than 2^28 pixels); a parameter outside the
 * limits given with the struct; a dt that is not finite or negative. YART_E_NO_DEVICE without a HIP device. */
int yart_hip_exposure_meter_device(YartExposure* exposure, const float* d_rgba, uint32_t width, uint32_t height,
                                   const YartExposureParams* params, float dt, void* stream);
/* Same, HOST pointer: the frame is copied to the handle's device and metered there. */
int yart_hip_exposure_meter_host(YartExposure* exposure, const float* rgba, uint32_t width, uint32_t height,
                                 const YartExposureParams* params, float dt);
/* Apply the handle's gain, the tonemap (look -1: none) and the encoding to a frame (DEVICE pointers; d_ldr_rgba, RGBA32F, or
 * d_rgb8, 3 bytes per pixel, may be NULL, not both; d_ldr_rgba may be d_rgba). YART_E_INVALID, before any device is touched: a NULL
 * exposure or d_rgba, both outputs NULL, a width or height of 0 (or more than 2^28 pixels), a look outside -1 .. 2. */
int yart_hip_exposure_apply_device(YartExposure* exposure, const float* d_rgba, uint32_t width, uint32_t height, int look,
                                   float* d_ldr_rgba /* may be NULL */, uint8_t* d_rgb8 /* may be NULL */, void* stream);
/* Same, HOST pointers */
int yart_hip_exposure_apply_host(YartExposure* exposure, const float* rgba, uint32_t width, uint32_t height, int look, float* ldr_rgba,
                                 uint8_t* rgb8);
/* The state record, and in hist256 (may be NULL) the 256 bins of the last meter call. */
int yart_hip_exposure_get(YartExposure* exposure, YartExposureState* state, uint32_t* hist256);
/* Diagnostics (tools/exposure_bench.py): the device time in ms per launch, over `repeats` launches between two events on the NULL
 * stream, of what = 0 / 1: the histogram kernel's two forms (per-wave counting / interleaved replicas), 2: the resolve kernel,
 * 3: the apply kernel with both outputs, 4: the kernels of yart_hip_tonemap_agx and yart_hip_encode_rgb8 one after the other.
 * DEVICE pointers; d_ldr_rgba and d_rgb8 are needed for 3 and 4. The handle's state may change; after 0 / 1 yart_hip_exposure_get
 * reports the sum of the `repeats` histograms (the tests compare both forms' counts with it). */
int yart_hip_debug_exposure_time(YartExposure* exposure, const float* d_rgba, uint32_t width, uint32_t height,
                                 const YartExposureParams* params, int what, uint32_t repeats, float* d_ldr_rgba, uint8_t* d_rgb8,
                                 float* ms_out);

const char* yart_hip_last_error(void);
int yart_hip_abi_version(void);
int yart_hip_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* YART_HIP_H */
