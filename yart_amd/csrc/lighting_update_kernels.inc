// lighting_update_kernels.inc — yart_hip_scene_update_lighting: new materials, new light emission / radius / transforms and new
// texels for the maps of image lights of a scene that is on the device (included by yart_hip.hip, unit 0, behind
// mesh_update_kernels.inc). The arithmetic is csrc/lighting_update.hpp's. Materials and lights are re-derived on the host by the
// expressions scene creation uses and uploaded (a few KB). A replaced map is uploaded into its place in texF32, its footprint records
// are rewritten by k_tex_quads, and for every image light that uses it the sampling tables are rebuilt IN PLACE on the device (the
// size is unchanged: every offset of its EnvDev stays):
//
//   k_lu_func      one lane per texel: func = |mean(rgb) * sin(theta_row)|
//   k_lu_rows      the rows' running sums cdf[k] = cdf[k-1] + func[k-1] / w: strictly sequential per row, so one lane per row, 64 rows
//                  per wave; the rows' 64 x 64 tiles go through LDS, so that global loads and stores are 256-byte row segments and
//                  not a stride-w gather. Leaves the unnormalised sums in the CDF's place and |integral| in rowInt
//   k_lu_norm      one lane per CDF entry: the divide by the row's integral (k / w where it is 0), and the row's {cdf, func} records
//   k_lu_marginal  one workgroup: lane 0 runs the marginal chain over |rowInt| (h terms), then every lane normalises entries and
//                  writes the marginal {margCdf, rowInt, cdf_k[1], 0} records; margIntegral into the EnvDev record
//   k_lu_guide     one lane per guide entry: a lower-bound search from index 1 (lighting_update.hpp::luGuideEntry)
//
// The image's texel sum (Lavg: a sequential binary32 sum whose order is part of the bits) is taken on the host from the caller's
// pixels while the device works. The library's host copy keeps what it reads after create current — materials, lights, lightDesc,
// envs (margIntegral is read back), areaPowerCdf, totalPower, texF32; envData and envGuide are the device's alone after an image
// update, and dominantLobeShare stays as at create (a default-pipeline heuristic: every pipeline renders the same frame).
namespace {

struct LuEnvArgs { const float* tex; float* data; uint32_t* guide; EnvDev* envOut; EnvDev e; };   // tex: the map's first texel; data / guide: envData / envGuide

__global__ void __launch_bounds__(kBlock) k_lu_func(LuEnvArgs a) {
  const size_t n = size_t(a.e.w) * a.e.h;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    const uint32_t y = uint32_t(i / a.e.w);
    a.data[a.e.funcOffset + i] = luFunc(a.tex + i * 3u, luSinTheta(y, a.e.h));
  }
}

constexpr uint32_t kLuTile = 64;
__global__ void __launch_bounds__(64) k_lu_rows(LuEnvArgs a) {
  __shared__ float tile[kLuTile][kLuTile + 1u];              // (+1: lane r walks row r, the lanes' words lie in 64 different banks)
  const uint32_t w = a.e.w, h = a.e.h, lane = threadIdx.x;
  const uint32_t row0 = blockIdx.x * kLuTile;
  const uint32_t rows = h - row0 < kLuTile ? h - row0 : kLuTile;
  const float* func = a.data + a.e.funcOffset;
  float* cdf = a.data + a.e.cdfOffset;
  float acc = 0.0f;
  if (lane < rows) cdf[size_t(row0 + lane) * (w + 1u)] = 0.0f;
  for (uint32_t c0 = 0; c0 < w; c0 += kLuTile) {
    const uint32_t cols = w - c0 < kLuTile ? w - c0 : kLuTile;
    for (uint32_t r = 0; r < rows; r++)
      if (lane < cols) tile[r][lane] = func[size_t(row0 + r) * w + c0 + lane];
    __syncthreads();
    if (lane < rows)
      for (uint32_t c = 0; c < cols; c++) { acc = luChainStep(acc, tile[lane][c], w); tile[lane][c] = acc; }
    __syncthreads();
    for (uint32_t r = 0; r < rows; r++)
      if (lane < cols) cdf[size_t(row0 + r) * (w + 1u) + 1u + c0 + lane] = tile[r][lane];
    __syncthreads();
  }
  if (lane < rows) a.data[a.e.rowIntOffset + row0 + lane] = fabsf(acc);
}

__global__ void __launch_bounds__(kBlock) k_lu_norm(LuEnvArgs a) {
  const uint32_t w = a.e.w, h = a.e.h;
  const size_t n = size_t(w + 1u) * h;
  float* rowPairs = a.data + a.e.pairOffset + size_t(h + 1u) * 4u;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    const uint32_t y = uint32_t(i / (w + 1u)), k = uint32_t(i % (w + 1u));
    float v = 0.0f;
    if (k) {
      // (the chain's terms are >= 0, so the integral is: |integral| is the integral, and the row's last sum)
      v = luNormalised(a.data[a.e.cdfOffset + i], k, w, a.data[a.e.rowIntOffset + y]);
      a.data[a.e.cdfOffset + i] = v;
    }
    luRowPair(rowPairs + i * 2u, k, w, v, a.data + a.e.funcOffset + size_t(y) * w);
  }
}

__global__ void __launch_bounds__(kBlock) k_lu_marginal(LuEnvArgs a) {
  __shared__ float integral;
  const uint32_t w = a.e.w, h = a.e.h;
  const float* rowInt = a.data + a.e.rowIntOffset;
  float* marg = a.data + a.e.margCdfOffset;
  if (threadIdx.x == 0) {
    float acc = 0.0f;
    marg[0] = 0.0f;
    for (uint32_t k = 1; k <= h; k++) { acc = luChainStep(acc, fabsf(rowInt[k - 1u]), h); marg[k] = acc; }
    integral = acc;
    a.envOut->margIntegral = acc;
  }
  __syncthreads();
  const float in = integral;
  for (uint32_t k = threadIdx.x; k <= h; k += blockDim.x) {
    const float v = k ? luNormalised(marg[k], k, h, in) : 0.0f;
    marg[k] = v;
    luMargPair(a.data + a.e.pairOffset + size_t(k) * 4u, k, h, v, rowInt, a.data + a.e.cdfOffset, w);
  }
}

__global__ void __launch_bounds__(kBlock) k_lu_guide(LuEnvArgs a) {
  const uint32_t w = a.e.w, h = a.e.h, Kw = a.e.guideKw, Kh = a.e.guideKh;
  const size_t first = size_t(Kh) + 1u, n = first + size_t(h) * (Kw + 1u);
  uint32_t* g = a.guide + a.e.guideOffset;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    if (i < first) { g[i] = luGuideEntry(a.data + a.e.margCdfOffset, h, uint32_t(i), Kh); continue; }
    const uint32_t y = uint32_t((i - first) / (Kw + 1u)), j = uint32_t((i - first) % (Kw + 1u));
    g[i] = luGuideEntry(a.data + a.e.cdfOffset + size_t(y) * (w + 1u), w, j, Kw);
  }
}

constexpr UpdateCheck luCheck{"scene_update_lighting: "};

// Everything that can refuse an update before the scene is looked at (behind updateHead's checks)
void luValidateArguments(const YartSceneLightingUpdate& u) {
  luCheck(u.flags == 0u, "unknown flags (none are defined)");
  luCheck(u.n_materials || u.n_lights || u.n_images, "n_materials, n_lights and n_images are all 0");
  luCheck(!u.n_materials || u.materials != nullptr, "materials pointer is null");
  luCheck(!u.n_lights || u.lights != nullptr, "lights pointer is null");
  luCheck(!u.n_images || u.images != nullptr, "images pointer is null");
}
// ... and what compares it with the scene
void luValidateAgainstScene(const YartScene& scene, const YartSceneLightingUpdate& u) {
  const HostImage& h = scene.host;
  const LightingUpdateState& lu = scene.lightUp;
  if (u.n_materials) {
    luCheck(u.n_materials == h.nMaterials, "n_materials is neither 0 nor the scene's material count " + std::to_string(h.nMaterials));
    luCheck(lu.materialDesc.size() == h.nMaterials, "internal: the scene does not hold its material descriptors");
    for (uint32_t i = 0; i < u.n_materials; i++) {
      const YartMaterialDesc& a = u.materials[i]; const YartMaterialDesc& b = lu.materialDesc[i];
      const std::string name = "material " + std::to_string(i);
      luCheck(a.tex_base == b.tex_base && a.tex_mr == b.tex_mr && a.tex_transmission == b.tex_transmission && a.tex_normal == b.tex_normal &&
              a.tex_clearcoat == b.tex_clearcoat && a.tex_emission == b.tex_emission, name + ": a texture slot differs from the scene's");
      luCheck((a.thin_transmission != 0u) == (b.thin_transmission != 0u), name + ": thin_transmission differs from the scene's");
      luCheck(finiteWords(a.base, 3) && finiteWords(a.emission, 3) && finiteWords(&a.metallic, 9) && finiteWords(a.volume_color, 3) &&
              finiteWords(&a.volume_density, 1), name + ": a word is not finite");
      luCheck(luTransparent(a) == ((h.materials[i].flags & MAT_TRANSPARENT) != 0u),
              name + ": the change would make a thin material transparent or opaque (transmission > 0: the leaf records carry that bit; such a scene is re-created)");
    }
  }
  if (u.n_lights) {
    luCheck(u.n_lights == h.nLights, "n_lights is neither 0 nor the scene's light count " + std::to_string(h.nLights));
    for (uint32_t i = 0; i < u.n_lights; i++) {
      const YartLightDesc& a = u.lights[i]; const YartLightDesc& b = h.lightDesc[i];
      const std::string name = "light " + std::to_string(i);
      luCheck(sameLightTopology(a, b), name + ": type, mesh, tri, two_sided or texture differ from the scene's");
      luCheck(finiteWords(&a.radius, 1) && finiteWords(a.emission, 3), name + ": radius or an emission word is not finite");
      luCheck(finiteWords(a.fwd, 16) && finiteWords(a.inv, 16), name + ": a matrix word is not finite");
    }
  }
  std::vector<uint8_t> listed(h.textures.size(), 0);
  for (uint32_t k = 0; k < u.n_images; k++) {
    const YartEnvImageUpdate& im = u.images[k];
    const std::string name = "image " + std::to_string(k) + " (texture " + std::to_string(im.texture) + ")";
    luCheck(im.texture < h.textures.size() && h.textures[im.texture].width != 0u, name + ": texture index out of range");
    luCheck(!listed[im.texture], name + ": the texture is listed twice");
    listed[im.texture] = 1;
    const TexDev& t = h.textures[im.texture];
    luCheck(t.isFloat && t.channels == 3u, name + ": not a float RGB texture");
    bool used = false;
    for (uint32_t i = 0; i < h.nLights; i++) used |= h.lights[i].type == LIGHT_IMAGE_INF && h.lights[i].texture == int32_t(im.texture);
    luCheck(used, name + ": no image light uses the texture");
    luCheck(im.width == t.width && im.height == t.height, name + ": " + std::to_string(im.width) + " x " + std::to_string(im.height) + ", the texture is " +
                                                            std::to_string(t.width) + " x " + std::to_string(t.height) + " (the size cannot change)");
    luCheck(im.pixels != nullptr, name + ": pixels pointer is null");
    const size_t n = size_t(t.width) * t.height * 3u;
    luCheck(size_t(t.offset) + n <= h.texF32.size(), "internal: the texture lies outside the scene's float texels");
    bool ok = true;
    for (size_t i = 0; i < n && ok; i++) ok = luTexelWordOk(im.pixels[i]);
    luCheck(ok, name + ": a texel word is not finite or larger than 2^64 in magnitude");
  }
}

uint32_t luGrid(size_t n) { return uint32_t(std::min<size_t>((n + kBlock - 1u) / kBlock, 65535u)); }

// the tables of one image light from the texels that are in texF32 (in stream order)
void luRebuildEnv(YartScene& s, uint32_t env, const TexDev& t, UpdateCall& call) {
  const hipStream_t stream = call.stream;
  const EnvDev& e = s.host.envs[env];
  const uint32_t w = e.w, h = e.h;
  // (what the kernels index: the record is create's, checked all the same before anything is launched from it)
  const size_t dataEnd = size_t(e.pairOffset) + size_t(h + 1u) * 4u + size_t(h) * (w + 1u) * 2u;
  const size_t guideEnd = size_t(e.guideOffset) + size_t(e.guideKh) + 1u + size_t(h) * (size_t(e.guideKw) + 1u);
  if (w != t.width || h != t.height || w == 0u || h == 0u || dataEnd > s.envData.n || guideEnd > s.envGuide.n ||
      size_t(e.funcOffset) + size_t(w) * h > e.cdfOffset || size_t(e.cdfOffset) + size_t(w + 1u) * h > e.rowIntOffset ||
      size_t(e.rowIntOffset) + h > e.margCdfOffset || size_t(e.margCdfOffset) + h + 1u > e.pairOffset || env >= s.envs.n)
    throw HipError("scene_update_lighting: the tables of image light table " + std::to_string(env) + " do not have create's layout");
  LuEnvArgs a{s.texF32.p + t.offset, s.envData.p, s.envGuide.p, s.envs.p + env, e};
  hipLaunchKernelGGL(k_lu_func, dim3(luGrid(size_t(w) * h)), dim3(kBlock), 0, stream, a);
  call.launched();
  hipLaunchKernelGGL(k_lu_rows, dim3((h + kLuTile - 1u) / kLuTile), dim3(64), 0, stream, a);
  call.launched();
  hipLaunchKernelGGL(k_lu_norm, dim3(luGrid(size_t(w + 1u) * h)), dim3(kBlock), 0, stream, a);
  call.launched();
  hipLaunchKernelGGL(k_lu_marginal, dim3(1), dim3(kBlock), 0, stream, a);
  call.launched();
  hipLaunchKernelGGL(k_lu_guide, dim3(luGrid(size_t(e.guideKh) + 1u + size_t(h) * (size_t(e.guideKw) + 1u))), dim3(kBlock), 0, stream, a);
  call.launched();
}

void luUpdate(YartScene& s, const YartSceneLightingUpdate& u, hipStream_t stream, YartSceneUpdateStats* stats) {
  std::vector<uint8_t> cls;                                  // the lobe classes, and the one word of an EnvDev record that the device
  std::vector<float> margIntegral;                           // derives (copies read / write the two: before the frame)
  UpdateCall call(WallClock::now(), s.device, stream);
  HostImage& h = s.host;
  LightingUpdateState& lu = s.lightUp;
  if (lu.envSumKnown.size() != h.envs.size()) { lu.envSumKnown.assign(h.envs.size(), 0); lu.envSum.assign(h.envs.size(), LuSum{0.0f, 0.0f, 0.0f}); }
  std::vector<uint32_t> touched;                             // the EnvDev records whose margIntegral the device rewrites
  for (uint32_t k = 0; k < u.n_images; k++) {
    const YartEnvImageUpdate& im = u.images[k];
    const TexDev& t = h.textures[im.texture];
    const size_t n = size_t(t.width) * t.height * 3u;
    HIP_CHECK(hipMemcpyAsync(s.texF32.p + t.offset, im.pixels, n * 4u, hipMemcpyHostToDevice, stream));
    if (s.texQuadsOn && t.quadOffset != kNoTexQuads) {
      TexQuadArgs qa{s.texU8.p, s.texF32.p, t, s.texQuads.p + size_t(t.quadOffset) * 16u};
      hipLaunchKernelGGL(k_tex_quads, dim3(luGrid(n / 3u)), dim3(kBlock), 0, stream, qa);
      call.launched();
    }
    for (uint32_t i = 0; i < h.nLights; i++)
      if (h.lights[i].type == LIGHT_IMAGE_INF && h.lights[i].texture == int32_t(im.texture)) {
        luRebuildEnv(s, h.lights[i].envOffset, t, call);
        touched.push_back(h.lights[i].envOffset);
      }
    // on the host while the device works: the host's copy of the texels and their sum (its order is part of the bits)
    std::memcpy(h.texF32.data() + t.offset, im.pixels, n * 4u);
    const LuSum sum = luTexelSum(im.pixels, n / 3u);
    for (uint32_t i = 0; i < h.nLights; i++)
      if (h.lights[i].type == LIGHT_IMAGE_INF && h.lights[i].texture == int32_t(im.texture)) {
        lu.envSum[h.lights[i].envOffset] = sum; lu.envSumKnown[h.lights[i].envOffset] = 1;
      }
  }
  if (u.n_materials) {
    for (uint32_t i = 0; i < u.n_materials; i++) { luMaterial(h.materials[i], u.materials[i]); lu.materialDesc[i] = u.materials[i]; }
    cls = luLobeClasses(h.materials);
    HIP_CHECK(hipMemcpyAsync(s.materials.p, h.materials.data(), h.materials.size() * sizeof(MaterialDev), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(s.matClass.p, cls.data(), cls.size(), hipMemcpyHostToDevice, stream));
  }
  margIntegral.resize(touched.size());
  for (size_t k = 0; k < touched.size(); k++)
    HIP_CHECK(hipMemcpyAsync(&margIntegral[k], &s.envs.p[touched[k]].margIntegral, 4, hipMemcpyDeviceToHost, stream));
  if (u.n_lights || u.n_images) {                            // (an image light's power follows its map's Lavg)
    for (uint32_t i = 0; i < h.nLights; i++) {
      const LightDev& ld = h.lights[i];
      if (ld.type != LIGHT_IMAGE_INF || lu.envSumKnown[ld.envOffset]) continue;
      const TexDev& t = h.textures[ld.texture];              // a map that was never replaced: the sum create took, over the same texels
      lu.envSum[ld.envOffset] = luTexelSum(h.texF32.data() + t.offset, size_t(t.width) * t.height);
      lu.envSumKnown[ld.envOffset] = 1;
    }
    const std::vector<YartLightDesc> desc = u.n_lights ? std::vector<YartLightDesc>(u.lights, u.lights + u.n_lights) : h.lightDesc;
    luRederiveLights(h, desc.data(), h.nLights, lu.envSum.data());
    uploadLights(s, stream);
  }
  call.close();
  for (size_t k = 0; k < touched.size(); k++) h.envs[touched[k]].margIntegral = margIntegral[k];
  call.finish(stats);
}

}  // namespace

extern "C" {

int yart_hip_scene_update_lighting(YartScene* scene, const YartSceneLightingUpdate* update, void* stream, YartSceneUpdateStats* stats) {
  return updateEntry(luCheck, "YartSceneLightingUpdate", scene, update, stream, stats, luValidateArguments, luValidateAgainstScene, luUpdate);
}

int yart_hip_probe_lighting(YartScene* scene, YartLightingProbe* p) {
  return guarded([&] {
    require(scene, "probe_lighting: scene pointer is null");
    require(p && p->struct_size >= sizeof(YartLightingProbe), "probe_lighting: probe pointer is null or its struct_size too small");
    std::lock_guard<std::mutex> lock(scene->mu);
    YartScene& s = *scene;
    const HostImage& h = s.host;
    HIP_CHECK(hipSetDevice(s.device));
    p->n_materials = uint64_t(h.materials.size()); p->n_mat_class = uint64_t((h.materials.size() + 3u) / 4u * 4u);
    p->n_lights = uint64_t(h.lights.size()); p->n_envs = uint64_t(h.envs.size());
    p->n_env_data = uint64_t(h.envData.size()); p->n_env_guide = uint64_t(h.envGuide.size());
    p->n_area_power_cdf = uint64_t(h.areaPowerCdf.size()); p->n_tex_f32 = uint64_t(h.texF32.size());
    p->n_tex_quad_bytes = s.texQuadsOn ? uint64_t(h.texQuadUnits) * 16u : 0u;
    p->n_textures = uint64_t(h.textures.size());
    p->total_power = s.dev.totalPower;
    auto copy = [&](void* out, const void* dev, size_t bytes) { if (out && bytes) HIP_CHECK(hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost)); };
    copy(p->materials, s.materials.p, h.materials.size() * sizeof(MaterialDev));
    copy(p->mat_class, s.matClass.p, size_t(p->n_mat_class));
    copy(p->lights, s.lights.p, h.lights.size() * sizeof(LightDev));
    copy(p->envs, s.envs.p, h.envs.size() * sizeof(EnvDev));
    copy(p->env_data, s.envData.p, h.envData.size() * 4u);
    copy(p->env_guide, s.envGuide.p, h.envGuide.size() * 4u);
    copy(p->area_power_cdf, s.areaPowerCdf.p, h.areaPowerCdf.size() * 4u);
    copy(p->tex_f32, s.texF32.p, h.texF32.size() * 4u);
    copy(p->tex_quads, s.texQuads.p, size_t(p->n_tex_quad_bytes));
    copy(p->textures, s.textures.p, h.textures.size() * sizeof(TexDev));
  });
}

int yart_hip_probe_texel_sum(const float* pixels, uint64_t n_texels, float* sum3_out) {
  return guarded([&] {
    require(pixels && sum3_out, "probe_texel_sum: a pointer is null");
    const LuSum s = luTexelSum(pixels, size_t(n_texels));
    sum3_out[0] = s.r; sum3_out[1] = s.g; sum3_out[2] = s.b;
  });
}

}  // extern "C"
