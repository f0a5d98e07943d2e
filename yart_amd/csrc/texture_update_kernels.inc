// texture_update_kernels.inc — yart_hip_scene_update_textures: new texels for 8-bit material textures of a scene that is on the device
// (included by yart_hip.hip, unit 0, behind lighting_update_kernels.inc). The arithmetic is csrc/texture_update.hpp's. Per listed
// texture, in stream order:
//
//   (copy)           the pixels into the texture's place in texU8, from host or device memory; the library's host copy follows
//   k_tex_quads      the footprint records, once per place that holds the texture (texture_update.hpp::tuPlaces: its own array, and one
//                    launch per bundle it is a member of — through a clone entry's quadOffset / quadStride, so that only the member's
//                    16 bytes of every 64-byte record are rewritten). The per-member form is the one kept: a fused kernel that
//                    rewrites a bundle's whole records was not measured (profiles/texture_update.txt)
//   k_tu_alpha       (a 4-channel texture that is some material's tex_base) "an alpha byte below 255": one streaming pass over the
//                    RGBA words just written, 16 bytes per lane and step, one atomic per workgroup that found one
//
// The flags are read back with the synchronisation that ends the update. Only where a material's MAT_HAS_ALPHA CHANGED the chain
// scene creation derives from it is re-derived, in place, for every mesh that has a face of such a material:
//
//   (copy)           the material records (flags)
//   k_tu_leaves      one lane per leaf record: the alpha bit of matFlags from the record's material (one word of each 48-byte record)
//   k_mu_alpha_scan  (the mesh still has an alpha-tested material) mesh_update_kernels.inc's prefix sum over the leaf order
//   k_tu_links       one lane per node of the FINAL node array: the range of the leaf order below it (a walk to its left-most and its
//                    right-most leaf), the alpha bit of its link word from the prefix sum, the mesh's alpha flag from the root
//
// and the stream is synchronised once more. MeshUpdateState::meshAlpha of those meshes is forgotten: it caches "a face has an
// alpha-tested material".
namespace {

// words: the texture's first RGBA word (4-byte aligned: every texture of texU8 starts at a multiple of 4); out: set to 1, never cleared
__global__ void __launch_bounds__(kBlock) k_tu_alpha(const uint32_t* words, uint32_t n, uint32_t* out) {
  // 16-byte loads over the aligned middle; the at most 3 words before it and 3 behind it go to the first lanes of workgroup 0
  const uint32_t misaligned = uint32_t((16u - (reinterpret_cast<uintptr_t>(words) & 15u)) & 15u) / 4u;
  const uint32_t head = misaligned < n ? misaligned : n;
  const uint32_t nVec = (n - head) / 4u;
  const uint4* vec = reinterpret_cast<const uint4*>(words + head);
  bool any = false;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nVec; i += gridDim.x * blockDim.x) {
    const uint4 v = vec[i];
    any = any || tuWordHasAlpha(v.x) || tuWordHasAlpha(v.y) || tuWordHasAlpha(v.z) || tuWordHasAlpha(v.w);
  }
  if (blockIdx.x == 0u && threadIdx.x < 6u) {
    const uint32_t i = threadIdx.x < 3u ? threadIdx.x : head + nVec * 4u + (threadIdx.x - 3u);
    if (threadIdx.x < 3u ? i < head : i < n) any |= tuWordHasAlpha(words[i]);
  }
  if (__syncthreads_or(any ? 1 : 0) && threadIdx.x == 0u) atomicOr(out, 1u);
}

__global__ void __launch_bounds__(kBlock) k_tu_leaves(LeafTri* leaf, const MaterialDev* materials, uint32_t n, uint32_t nMaterials) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = leaf[i].material;
  if (m < nMaterials) leaf[i].matFlags = tuLeafFlags(leaf[i].matFlags, materials[m].flags);
}

// prefix: k_mu_alpha_scan's over the mesh's leaf records, or nullptr: no record has the bit. A lane writes its own node's link word
// while others read it on their walks: they read its index and span bits, which every write leaves as they are.
struct TuLinkArgs { BvhNode* nodes; const LeafTri* leaves; const uint32_t* prefix; MeshDev* mesh; uint32_t* error; uint32_t nNodes, nTris; };
__global__ void __launch_bounds__(kBlock) k_tu_links(TuLinkArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nNodes) return;
  bool alpha = false;
  if (a.prefix) {
    uint32_t first = 0, end = 0;
    if (!tuNodeRange(a.nodes, a.nNodes, a.leaves, a.nTris, i, first, end)) { *a.error = 1u; return; }
    alpha = a.prefix[end] != a.prefix[first];
  }
  a.nodes[i].leftFirst = tuLinkWord(a.nodes[i].leftFirst, alpha);
  if (i == 0u) a.mesh->hasAlpha = alpha ? 1u : 0u;
}

constexpr UpdateCheck tuCheck{"scene_update_textures: "};

// Everything that can refuse an update before the scene is looked at (behind updateHead's checks)
void tuValidateArguments(const YartSceneTextureUpdate& u) {
  tuCheck(u.flags == 0u, "unknown flags (none are defined)");
  tuCheck(u.n_textures >= 1u, "n_textures is 0");
  tuCheck(u.textures != nullptr, "textures pointer is null");
}
// ... and what compares it with the scene
void tuValidateAgainstScene(const YartScene& scene, const YartSceneTextureUpdate& u) {
  const HostImage& h = scene.host;
  std::vector<uint8_t> listed(h.textures.size(), 0);
  for (uint32_t k = 0; k < u.n_textures; k++) {
    const YartTextureUpdate& tu = u.textures[k];
    const std::string name = "entry " + std::to_string(k) + " (texture " + std::to_string(tu.texture) + ")";
    tuCheck((tu.flags & ~YART_TEXELS_ON_DEVICE) == 0u, name + ": unknown flags");
    tuCheck(tu.texture < h.textures.size() && h.textures[tu.texture].width != 0u && !tuIsClone(h.textures[tu.texture]),
            name + ": texture index out of range (the scene's textures as given at create)");
    tuCheck(!listed[tu.texture], name + ": the texture is listed twice");
    listed[tu.texture] = 1;
    const TexDev& t = h.textures[tu.texture];
    tuCheck(!t.isFloat, name + ": a float texture (the maps of image lights: yart_hip_scene_update_lighting)");
    tuCheck(tu.width == t.width && tu.height == t.height && tu.channels == t.channels,
            name + ": " + std::to_string(tu.width) + " x " + std::to_string(tu.height) + " x " + std::to_string(tu.channels) + ", the texture is " +
                std::to_string(t.width) + " x " + std::to_string(t.height) + " x " + std::to_string(t.channels) + " (size and channels cannot change)");
    tuCheck(tu.pixels != nullptr, name + ": pixels pointer is null");
    tuCheck(size_t(t.offset) % 4u == 0u && size_t(t.offset) + size_t(t.width) * t.height * t.channels <= h.texU8.size(),
            "internal: the texture lies outside the scene's 8-bit texels");
  }
}

void tuUpdate(YartScene& s, const YartSceneTextureUpdate& u, hipStream_t stream, YartSceneUpdateStats* stats) {
  std::vector<uint32_t> result;                              // (copies write the two: before the frame)
  uint32_t error = 0;
  UpdateCall call(WallClock::now(), s.device, stream);
  HostImage& h = s.host;
  TextureUpdateState& tu = s.texUp;
  const std::vector<YartMaterialDesc>& desc = s.lightUp.materialDesc;     // (tex_base as the caller gave it: h.materials hold clone indices)
  // result words: one per listed texture ("an alpha byte below 255"), then the chain's error word
  tu.result.ensure(size_t(u.n_textures) + 1u);
  HIP_CHECK(hipMemsetAsync(tu.result.p, 0, (size_t(u.n_textures) + 1u) * 4u, stream));
  std::vector<uint8_t> reduced(u.n_textures, 0);
  for (uint32_t k = 0; k < u.n_textures; k++) {
    const YartTextureUpdate& e = u.textures[k];
    const TexDev& t = h.textures[e.texture];
    const size_t nTexels = size_t(t.width) * t.height, bytes = nTexels * t.channels;
    const bool onDevice = (e.flags & YART_TEXELS_ON_DEVICE) != 0u;
    HIP_CHECK(hipMemcpyAsync(s.texU8.p + t.offset, e.pixels, bytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (onDevice) HIP_CHECK(hipMemcpyAsync(h.texU8.data() + t.offset, e.pixels, bytes, hipMemcpyDeviceToHost, stream));
    if (s.texQuadsOn)
      for (uint32_t place : tuPlaces(h.textures, e.texture)) {
        const TexDev& p = h.textures[place];
        TexQuadArgs qa{s.texU8.p, s.texF32.p, p, s.texQuads.p + size_t(p.quadOffset) * 16u};
        hipLaunchKernelGGL(k_tex_quads, dim3(luGrid(nTexels)), dim3(kBlock), 0, stream, qa);
        call.launched();
      }
    bool isBase = false;
    for (const YartMaterialDesc& m : desc) isBase |= m.tex_base == int32_t(e.texture);
    if (isBase && t.channels == 4u) {
      const uint32_t grid = uint32_t(std::min<size_t>((nTexels / 4u + kBlock - 1u) / kBlock + 1u, 2048u));
      hipLaunchKernelGGL(k_tu_alpha, dim3(grid), dim3(kBlock), 0, stream, reinterpret_cast<const uint32_t*>(s.texU8.p + t.offset), uint32_t(nTexels), tu.result.p + k);
      call.launched();
      reduced[k] = 1;
    }
    if (!onDevice) std::memcpy(h.texU8.data() + t.offset, e.pixels, bytes);   // (while the device works)
  }
  result.assign(size_t(u.n_textures) + 1u, 0u);
  HIP_CHECK(hipMemcpyAsync(result.data(), tu.result.p, result.size() * 4u, hipMemcpyDeviceToHost, stream));
  call.close();

  // ---- the materials whose flag changed, and the meshes with a face of one of them
  std::vector<uint8_t> flipped(h.nMaterials, 0);
  bool anyFlip = false;
  for (uint32_t k = 0; k < u.n_textures; k++) {
    if (!reduced[k]) continue;
    const uint32_t now = result[k] ? uint32_t(MAT_HAS_ALPHA) : 0u;
    for (uint32_t i = 0; i < h.nMaterials && i < desc.size(); i++) {
      if (desc[i].tex_base != int32_t(u.textures[k].texture) || (h.materials[i].flags & MAT_HAS_ALPHA) == now) continue;
      h.materials[i].flags = (h.materials[i].flags & ~uint32_t(MAT_HAS_ALPHA)) | now;
      flipped[i] = 1; anyFlip = true;
    }
  }
  if (anyFlip) {
    HIP_CHECK(hipMemcpyAsync(s.materials.p, h.materials.data(), h.materials.size() * sizeof(MaterialDev), hipMemcpyHostToDevice, stream));
    if (tu.meshMaterials.size() != h.meshes.size()) {        // per mesh the materials of its faces (kept until yart_hip_scene_replace_meshes changes faces: it clears the table)
      tu.meshMaterials.assign(h.meshes.size(), {});
      for (size_t mi = 0; mi < h.meshes.size(); mi++) {
        std::vector<uint32_t>& mm = tu.meshMaterials[mi];
        for (uint32_t f = 0; f < h.meshes[mi].nTris; f++) mm.push_back(h.triVerts[h.meshes[mi].triOffset + f].w);
        std::sort(mm.begin(), mm.end());
        mm.erase(std::unique(mm.begin(), mm.end()), mm.end());
      }
    }
    MeshUpdateState& mu = s.meshUp;
    for (size_t mi = 0; mi < h.meshes.size(); mi++) {
      bool affected = false, alpha = false;
      for (uint32_t m : tu.meshMaterials[mi]) {
        if (m >= h.nMaterials) continue;
        affected |= flipped[m] != 0; alpha |= (h.materials[m].flags & MAT_HAS_ALPHA) != 0u;
      }
      if (!affected) continue;
      MeshDev& md = h.meshes[mi];
      LeafTri* leaves = s.leafTris.p + md.leafOffset;
      hipLaunchKernelGGL(k_tu_leaves, dim3((md.nTris + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, leaves, s.materials.p, md.nTris, h.nMaterials);
      call.launched();
      if (alpha) {
        mu.prefix.ensure(size_t(md.nTris) + 1u);
        hipLaunchKernelGGL(k_mu_alpha_scan, dim3(1), dim3(kMuScanBlock), 0, stream, leaves, mu.prefix.p, md.nTris);
        call.launched();
      }
      TuLinkArgs la{s.bvhNodes.p + md.nodeOffset, leaves, alpha ? mu.prefix.p : nullptr, s.meshes.p + mi, tu.result.p + u.n_textures, md.nNodes, md.nTris};
      hipLaunchKernelGGL(k_tu_links, dim3((md.nNodes + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, la);
      call.launched();
      md.hasAlpha = alpha ? 1u : 0u;
      if (mi < mu.meshAlpha.size()) mu.meshAlpha[mi] = int8_t(-1);
    }
    HIP_CHECK(hipMemcpyAsync(&error, tu.result.p + u.n_textures, 4, hipMemcpyDeviceToHost, stream));
    call.close();                                            // (a second time: ms_device ends behind the chain)
    if (error) throw HipError("scene_update_textures: the node array of a mesh is not a tree of its leaf order");
  }
  call.finish(stats);
}

}  // namespace

extern "C" {

int yart_hip_scene_update_textures(YartScene* scene, const YartSceneTextureUpdate* update, void* stream, YartSceneUpdateStats* stats) {
  return updateEntry(tuCheck, "YartSceneTextureUpdate", scene, update, stream, stats, tuValidateArguments, tuValidateAgainstScene, tuUpdate);
}

int yart_hip_probe_textures(YartScene* scene, YartTexturesProbe* p) {
  return guarded([&] {
    require(scene, "probe_textures: scene pointer is null");
    require(p && p->struct_size >= sizeof(YartTexturesProbe), "probe_textures: probe pointer is null or its struct_size too small");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    const HostImage& h = s.host;
    HIP_CHECK(hipSetDevice(s.device));
    p->n_tex_u8 = uint64_t(std::max<size_t>(h.texU8.size(), 1));
    p->n_textures = uint64_t(h.textures.size());
    if (p->tex_u8) {
      p->tex_u8[0] = 0;                                      // (a scene without 8-bit texels: the one element is the buffer's minimum size)
      if (!h.texU8.empty()) HIP_CHECK(hipMemcpy(p->tex_u8, s.texU8.p, h.texU8.size(), hipMemcpyDeviceToHost));
    }
    if (p->textures && !h.textures.empty()) HIP_CHECK(hipMemcpy(p->textures, s.textures.p, h.textures.size() * sizeof(TexDev), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
