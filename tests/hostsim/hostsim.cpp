// hostsim.cpp — TEST INFRASTRUCTURE, never part of libyart_hip.so.
//
// Compiles the product's device headers (yart_amd/csrc/*.hpp) as plain host C++
// (YART_HD expands to `inline`) and evaluates the known-answer-test program of
// oracle/kat_common.hpp with them, so that every device function can be compared
// bit for bit with the compiled reference (oracle/_ref/yart_ref kat) in the
// GPU-less build container. It also renders small images on CPU threads with the
// same per-sample code, which lets `pytest -m "not gpu"` bound the difference
// between the kernel source and the reference before a GPU is involved.
// It is not a fallback: the C ABI has no path to this code (tests/test_no_fallback.py
// checks that the library fails without a device).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <memory>
#include <mutex>
#include <thread>

// stackcheck: what the traversal stack of every ray reaches. The device headers call YART_STACK_PROBE at a ray's start (0), at
// every push (1, entries after the push) and where the fast walk hands a ray over (2, entries held); only this host build
// defines it — in the kernels the macro is empty.
struct StackProbe {
  uint32_t rayMax = 0; bool open = false;
  uint64_t rays = 0, rayHist[65] = {0}, handHist[65] = {0}; uint32_t maxIndex = 0;
  void flush() { if (open) { rayHist[rayMax < 64u ? rayMax : 64u]++; rays++; if (rayMax > maxIndex) maxIndex = rayMax; } open = false; rayMax = 0; }
  void event(int what, uint32_t k) {
    if (what == 0) { flush(); open = true; }
    else if (what == 1) { if (k > rayMax) rayMax = k; }
    else handHist[k < 64u ? k : 64u]++;
  }
};
static thread_local StackProbe* t_stackProbe = nullptr;
#define YART_STACK_PROBE(what, k) do { if (t_stackProbe) t_stackProbe->event((what), (k)); } while (0)

#include "../../oracle/kat_common.hpp"
#include "../../oracle/params.hpp"
#include "../../oracle/rayrec.hpp"
#include "../../oracle/shaderec.hpp"
#include "../../yart_amd/csrc/estimator.hpp"
#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/tonemap.hpp"
#include "../../yart_amd/csrc/integrator.hpp"
#include "../../yart_amd/csrc/probe_record.hpp"
#include "../../yart_amd/csrc/shade_record.hpp"
#include "../../yart_amd/csrc/scene_file.hpp"

using namespace yart_hip;

static YartCameraDesc cameraDesc(const params::Params& p) {
  YartCameraDesc c{};
  c.width = p.width; c.height = p.height; c.focal_length = p.focal; c.f_number = p.fnumber;
  c.sensor[0] = p.sensor[0]; c.sensor[1] = p.sensor[1];
  for (int i = 0; i < 3; i++) { c.position[i] = p.eye[i]; c.target[i] = p.target[i]; c.up[i] = p.up[i]; }
  c.exposure = p.exposure; c.aperture_sides = p.apertureSides;
  return c;
}

struct Ctx {
  HostImage im;
  SceneDev sc;
  CameraDev cam;
  RenderConst rc;
};

// The traversal stacks of `lanes` threads, laid out as the kernels lay them out: the first `split` entries of a lane in one
// block ("LDS"), the rest in another ("spill"), both lane-interleaved (entry k of lane t at block[k * stride + t], stride > 1).
// The blocks are heap allocations of exactly split * stride and (bound - split) * stride words, so that under
// AddressSanitizer an index past either one is a report. bound = the scene's stack bound (host_scene.hpp), at least the
// reference's 64. YART_HOSTSIM_LDS_STACK (read here only) sets the split; without it every entry is in the first block, as before.
// YART_HOSTSIM_STACK_BOUND overrides the bound (tests: the area sized one entry short must be reported).
struct StackMem {
  uint32_t split, bound, stride;
  std::unique_ptr<uint64_t[]> lds, spill;
  StackMem(const Ctx& c, unsigned lanes) {
    bound = std::max(kRefStackDepth, c.im.stackBound);
    if (const char* e = std::getenv("YART_HOSTSIM_STACK_BOUND")) bound = uint32_t(std::atoi(e));
    split = bound;
    if (const char* e = std::getenv("YART_HOSTSIM_LDS_STACK")) split = std::min(bound, uint32_t(std::max(1, std::atoi(e))));
    stride = std::max(2u, lanes);
    lds.reset(new uint64_t[size_t(split) * stride]);
    spill.reset(new uint64_t[size_t(bound - split) * stride]);
  }
};

static PathCtx pathCtx(const Ctx& c, const StackMem& m, unsigned lane) {
  PathCtx px;
  px.sc = &c.sc;
  px.sobol = reinterpret_cast<const uint32_t*>(c.sc.lut + LutDev::sobol);
  px.stk.lds = m.lds.get() + lane; px.stk.ldsStride = m.stride; px.stk.ldsDepth = m.split;
  px.stk.spill = m.spill.get() + lane; px.stk.spillStride = m.stride;
  px.rc = c.rc;
  return px;
}

// The shading inputs of the KAT program (oracle/kat_common.hpp) as case records (oracle/shaderec.hpp): the LUT grid, per material
// bsdfCasesPerMaterial x (one BSDF case, one MAT case), per light of kat::lightSubset four LIGHT cases, then 32 PICK cases where
// the scene has lights. `kat` below evaluates exactly these records and `shade-kat-cases` writes them out (the device probe is fed
// them and compared with the committed .kat.json), so the two cannot drift.
static shaderec::Case shadeCase(uint32_t kind, uint32_t index, uint32_t flags = 0) {
  shaderec::Case c{};
  c.kind = kind; c.index = index; c.flags = flags;
  return c;
}
static std::vector<shaderec::Case> katShadeCases(size_t nMaterials, size_t nLights) {
  std::vector<shaderec::Case> v;
  for (const auto& q : kat::lutInputs()) {
    shaderec::Case c = shadeCase(SHADE_LUT, 0);
    c.f[0] = q.c; c.f[1] = q.r; c.f[2] = q.f0; c.f[3] = q.ior;
    v.push_back(c);
  }
  for (size_t m = 0; m < nMaterials; m++) {
    kat::Lcg rng(1000 + uint32_t(m));
    for (int k = 0; k < kat::bsdfCasesPerMaterial; k++) {
      float r[12];
      for (int q = 0; q < 6; q++) r[q] = rng.sym();
      for (int q = 6; q < 12; q++) r[q] = rng.next();
      const f3 wo = normalized(mk3(r[0], r[1], r[2])), wi = normalized(mk3(r[3], r[4], r[5]));
      const f2 uv = mk2(r[6] * 3.0f - 1.0f, r[7] * 3.0f - 1.0f);
      shaderec::Case b = shadeCase(SHADE_BSDF, uint32_t(m), uint32_t(k & 1));
      const float fb[18] = {wo.x, wo.y, wo.z, wi.x, wi.y, wi.z, 0, 0, 1, 1, 0, 0, uv.x, uv.y, r[8], r[9], r[10], r[11]};
      for (int q = 0; q < 18; q++) b.f[q] = fb[q];
      v.push_back(b);
      shaderec::Case a = shadeCase(SHADE_MAT, uint32_t(m));
      const float fa[10] = {uv.x, uv.y, 0, 0, 1, 1, 0, 0, 1, r[10] * 4.0f};
      for (int q = 0; q < 10; q++) a.f[q] = fa[q];
      v.push_back(a);
    }
  }
  kat::Lcg rng(4242);
  for (size_t li : kat::lightSubset(nLights))
    for (int k = 0; k < 4; k++) {
      float r0 = rng.sym(), r1 = rng.next(), r2 = rng.sym(), r3 = rng.next(), r4 = rng.next();
      float w0 = rng.sym(), w1 = rng.sym(), w2 = rng.sym();
      const f3 wi = normalized(mk3(w0, w1, w2));
      shaderec::Case c = shadeCase(SHADE_LIGHT, uint32_t(li));
      const float fl[8] = {r0 * 4.0f, r1 * 8.0f, r2 * 4.0f, r3, r4, wi.x, wi.y, wi.z};
      for (int q = 0; q < 8; q++) c.f[q] = fl[q];
      v.push_back(c);
    }
  if (nLights > 0)
    for (int k = 0; k < 32; k++) {
      shaderec::Case c = shadeCase(SHADE_PICK, 0);
      c.f[0] = rng.next();
      v.push_back(c);
    }
  return v;
}

static int doKat(Ctx& c, const params::Params& p, const std::string& outPath) {
  kat::Writer w(outPath);
  const std::vector<shaderec::Case> shadeCases = katShadeCases(c.im.nMaterials, c.sc.nLights);
  {
    std::vector<uint64_t> h, mb, mo;
    std::vector<int64_t> l2;
    for (uint32_t d = 0; d < 48; d++) h.push_back(hashDim(d));
    for (uint64_t v : kat::mixInputs()) mb.push_back(mixBits(v));
    for (auto xy : kat::mortonInputs()) mo.push_back(encodeMorton2(xy.first, xy.second));
    for (float v : kat::log2Inputs()) l2.push_back(log2IntHost(v));
    w.u64("hash32", h); w.u64("mixbits", mb); w.u64("morton", mo); w.i64("log2int", l2);
  }
  const uint32_t* sobol = reinterpret_cast<const uint32_t*>(c.sc.lut + LutDev::sobol);
  {
    std::vector<float> out;
    for (const auto& k : kat::samplerCases()) {
      SamplerConfig cfg = makeSamplerConfig(k.spp, k.tile);
      Sampler s;
      startPixelSample(s, cfg, k.px, k.py, k.sample);
      for (int q : kat::samplerPattern()) {
        if (q == 2) { f2 v = get2D(s, cfg, sobol); out.push_back(v.x); out.push_back(v.y); }
        else out.push_back(get1D(s, cfg));
      }
    }
    w.f32("sampler", out);
  }
  {
    std::vector<float> e, ea, be, bea, ge, gea;
    const float* lut = c.sc.lut;
    for (const shaderec::Case& q : shadeCases) {
      if (q.kind != SHADE_LUT) continue;
      const float c = q.f[0], r = q.f[1], f0 = q.f[2], ior = q.f[3];
      e.push_back(ggxE(lut, c, r));
      ea.push_back(ggxEavg(lut, r));
      be.push_back(ggxBaseE(lut, f0, r, c));
      bea.push_back(ggxBaseEavg(lut, f0, r));
      ge.push_back(ggxGlassE(lut, ior, r, std::fabs(c)));
      gea.push_back(0.0f);   // ggxGlassEavg is not on the path (unused by parametric.cpp)
    }
    w.f32("ggxE", e); w.f32("ggxEavg", ea); w.f32("ggxBaseE", be);
    w.f32("ggxBaseEavg", bea); w.f32("ggxGlassE", ge); w.f32("ggxGlassEavg", gea);
  }
  {
    std::vector<float> out;
    kat::Lcg rng(7);
    for (size_t i = 0; i + 1 < p.probePixels.size(); i += 2) {
      for (int k = 0; k < 4; k++) {
        f2 uf = mk2(0, 0), ul = mk2(0, 0);
        uf.x = rng.next(); uf.y = rng.next(); ul.x = rng.next(); ul.y = rng.next();
        f3 o, d;
        cameraRay(c.cam, p.probePixels[i], p.probePixels[i + 1], uf, ul, o, d);
        out.push_back(o.x); out.push_back(o.y); out.push_back(o.z);
        out.push_back(d.x); out.push_back(d.y); out.push_back(d.z);
      }
    }
    w.f32("camera_rays", out);
  }
  {
    std::vector<uint64_t> out;
    for (size_t m = 0; m < c.im.meshes.size(); m++) {
      const MeshDev& md = c.im.meshes[m];
      out.push_back(md.nNodes);
      std::vector<BvhNode> plain(c.im.bvhNodes.begin() + md.nodeOffset, c.im.bvhNodes.begin() + md.nodeOffset + md.nNodes);
      for (auto& n : plain) n.leftFirst &= kLinkIndexMask;       // the device image carries an extra flag bit
      out.push_back(kat::fnv1a(plain.data(), size_t(md.nNodes) * 32));
      out.push_back(kat::fnv1a(c.im.bvhIndices[m].data(), c.im.bvhIndices[m].size() * 4));
    }
    w.u64("bvh", out);
  }
  StackMem stackMem(c, 1);
  PathCtx px = pathCtx(c, stackMem, 0);
  {
    std::vector<float> fo, ro6;
    std::vector<int64_t> io;
    // the reference's probe integrator holds ONE sampler, constructed and never started on a pixel (ref_driver.cpp: pixel 0,
    // sample 0, dimension 0): stochastic alpha tests of the probe rays draw from it one after the other
    Sampler dummy; dummy.dim = 0; dummy.morton = 0; dummy.pix = 0;
    for (size_t i = 0; i + 1 < p.probePixels.size(); i += 2) {
      f3 o, d;
      cameraRay(c.cam, p.probePixels[i], p.probePixels[i + 1], mk2(0.5f, 0.5f), mk2(0.5f, 0.5f), o, d);
      ro6.push_back(o.x); ro6.push_back(o.y); ro6.push_back(o.z); ro6.push_back(d.x); ro6.push_back(d.y); ro6.push_back(d.z);
      HitRec hr; hr.t = kInf; hr.u = hr.v = 0; hr.tri = 0; hr.node = 0; hr.backSide = 0;
      f3 att = mk3(1.0f);
      AlphaCtx ac; ac.sampler = &dummy; ac.cfg = c.rc.sampler;
      bool hit = traverseScene<false>(c.sc, o, d, 0.001f, hr, att, px.stk, ac);
      io.push_back(hit);
      if (!hit) { io.push_back(-1); io.push_back(-1); io.push_back(0); for (int k = 0; k < 12; k++) fo.push_back(0); continue; }
      Hit h = finalizeHit(c.sc, hr, o, d);
      io.push_back(localTri(c.sc, hr)); io.push_back(h.lightIdx); io.push_back(h.backSide);
      fo.push_back(h.t); fo.push_back(h.uv.x); fo.push_back(h.uv.y);
      fo.push_back(h.p.x); fo.push_back(h.p.y); fo.push_back(h.p.z);
      fo.push_back(h.n.x); fo.push_back(h.n.y); fo.push_back(h.n.z);
      fo.push_back(h.tg.x); fo.push_back(h.tg.y); fo.push_back(h.tg.z);
    }
    w.i64("hits_i", io); w.f32("hits_f", fo); w.f32("hit_rays", ro6);
  }
  {
    std::vector<float> fo;
    std::vector<int64_t> io;
    for (size_t k = 0; k < shadeCases.size(); k++) {
      const shaderec::Case& q = shadeCases[k];
      if (q.kind != SHADE_BSDF) continue;
      const shaderec::Case& a = shadeCases[k + 1];          // the MAT case of the same draw
      const MaterialDev& mt = c.im.materials[q.index];
      const f3 wo = mk3(q.f[0], q.f[1], q.f[2]), wi = mk3(q.f[3], q.f[4], q.f[5]), n = mk3(q.f[6], q.f[7], q.f[8]), t = mk3(q.f[9], q.f[10], q.f[11]);
      const f2 uv = mk2(q.f[12], q.f[13]), u = mk2(q.f[14], q.f[15]);
      const float uc = q.f[16], uc2 = q.f[17];
      const bool reg = q.flags & 1u;
      f3 f = bsdfF(c.sc, mt, wo, wi, n, t, uv);
      float pdf = bsdfPdf(c.sc, mt, wo, wi, n, t, uv);
      BsdfSample s = bsdfSample(c.sc, mt, wo, n, t, uv, u, uc, uc2, reg);
      fo.push_back(f.x); fo.push_back(f.y); fo.push_back(f.z);
      fo.push_back(pdf);
      io.push_back(s.scatter);
      fo.push_back(s.f.x); fo.push_back(s.f.y); fo.push_back(s.f.z);
      fo.push_back(s.Le.x); fo.push_back(s.Le.y); fo.push_back(s.Le.z);
      fo.push_back(s.wi.x); fo.push_back(s.wi.y); fo.push_back(s.wi.z);
      fo.push_back(s.pdf); fo.push_back(s.roughness);
      const f2 auv = mk2(a.f[0], a.f[1]);
      fo.push_back(matAlpha(c.sc, mt, auv));
      f3 base = matBase(c.sc, mt, auv);
      fo.push_back(base.x); fo.push_back(base.y); fo.push_back(base.z);
      f4 t4; t4.x = a.f[5]; t4.y = a.f[6]; t4.z = a.f[7]; t4.w = a.f[8];
      f3 sn = bsdfNormal(c.sc, mt, mk3(a.f[2], a.f[3], a.f[4]), t4, auv);
      fo.push_back(sn.x); fo.push_back(sn.y); fo.push_back(sn.z);
      f3 att = matAttenuation(mt, a.f[9]);
      fo.push_back(att.x); fo.push_back(att.y); fo.push_back(att.z);
      const bool lastOfMaterial = k + 2 >= shadeCases.size() || shadeCases[k + 2].kind != SHADE_BSDF || shadeCases[k + 2].index != q.index;
      if (lastOfMaterial) io.push_back((mt.flags & MAT_TRANSPARENT) ? 1 : 0);
    }
    w.i64("bsdf_i", io); w.f32("bsdf_f", fo);
  }
  {
    std::vector<float> fo;
    std::vector<int64_t> io;
    for (size_t k = 0; k < shadeCases.size(); k++) {
      const shaderec::Case& q = shadeCases[k];
      if (q.kind == SHADE_LIGHT) {
        const LightDev& l = c.sc.lights[q.index];
        if (shadeCases[k - 1].kind != SHADE_LIGHT || shadeCases[k - 1].index != q.index) fo.push_back(l.power);
        LightSample s = lightSample(c.sc, l, mk3(q.f[0], q.f[1], q.f[2]), mk2(q.f[3], q.f[4]));
        fo.push_back(s.Li.x); fo.push_back(s.Li.y); fo.push_back(s.Li.z);
        fo.push_back(s.wi.x); fo.push_back(s.wi.y); fo.push_back(s.wi.z);
        fo.push_back(s.p.x); fo.push_back(s.p.y); fo.push_back(s.p.z);
        fo.push_back(s.n.x); fo.push_back(s.n.y); fo.push_back(s.n.z);
        fo.push_back(s.pdf);
        const f3 wi = mk3(q.f[5], q.f[6], q.f[7]);
        fo.push_back(lightPdf(c.sc, l, wi));
        f3 le = lightLe(c.sc, l, octahedralUV(wi));
        fo.push_back(le.x); fo.push_back(le.y); fo.push_back(le.z);
        if (k + 1 >= shadeCases.size() || shadeCases[k + 1].kind != SHADE_LIGHT || shadeCases[k + 1].index != q.index)
          fo.push_back(lightSamplerP(c.sc, q.index));
      } else if (q.kind == SHADE_PICK) {
        float pl;
        uint32_t which = lightSamplerSample(c.sc, q.f[0], pl);
        io.push_back(which);
        fo.push_back(pl);
      }
    }
    w.i64("lights_i", io); w.f32("lights_f", fo);
  }
  {
    std::vector<float> rad, pix;
    uint32_t rays = 0;
    for (size_t i = 0; i + 1 < p.probePixels.size(); i += 2) {
      int m = gmonBuckets(int32_t(p.spp));
      f3 acc[kGmonMax]; uint32_t cnt[kGmonMax];
      for (int b = 0; b < kGmonMax; b++) { acc[b] = mk3(0); cnt[b] = 0; }
      for (uint32_t s = 0; s < p.spp; s++) {
        f3 L = samplePixel(px, c.cam, p.probePixels[i], p.probePixels[i + 1], s, rays);
        rad.push_back(L.x); rad.push_back(L.y); rad.push_back(L.z);
        f3 v = L * c.cam.exposureScale;
        int b = int(s % uint32_t(m));
        if (gmonAccepts(v)) { acc[b] += v; cnt[b]++; }
      }
      f3 v = gmonFinish(acc, cnt, m);
      pix.push_back(v.x); pix.push_back(v.y); pix.push_back(v.z);
    }
    w.f32("radiance", rad); w.f32("gmon", pix);
    std::vector<uint64_t> rc{rays};
    w.u64("probe_rays", rc);
  }
  w.close();
  return 0;
}

// hits: one record per ray of a ray file (oracle/rayrec.hpp) through csrc/probe_record.hpp — the function k_probe_rays runs:
// traverseScene + finalizeHit, the sampler started on the ray's (x, y, s) first and one get1D() drawn after the walk. walk: 0 the general walk (what the reference's records are
// compared with), 1 TRAV_FAST, 2 TRAV_FAST | TRAV_IDENTITY (refused unless every chain is the identity) — the record a fast
// walk gives is what yart_hip_probe_rays gives for it (include/yart_hip.h). The hostsim_lean build walks every ray with
// TRAV_FAST first, as its path tracer does, and reports on stderr every ray that walk keeps whose result differs from the
// general walk's; its records are the general walk's.
template <int MODE>
static rayrec::Rec hitRecord(const Ctx& c, const PathCtx& px, const rayrec::Ray& q) {
  rayrec::Rec r;
  probeRayRecord<MODE>(c.sc, c.rc.sampler, px.stk, reinterpret_cast<const uint32_t*>(&q), reinterpret_cast<uint32_t*>(&r));
  return r;
}
static int doHits(Ctx& c, const std::string& raysPath, const std::string& outPath, int walk) {
  if (walk < 0 || walk > 2 || (walk == 2 && !c.im.allIdentity)) { std::fprintf(stderr, "hits: walk %d is not available for this scene\n", walk); return 2; }
  StackMem stackMem(c, 1);
  PathCtx px = pathCtx(c, stackMem, 0);
  std::vector<rayrec::Rec> out;
  size_t k = 0, differ = 0;
  for (const rayrec::Ray& q : rayrec::load(raysPath)) {
    const rayrec::Rec r = walk == 0 ? hitRecord<TRAV_GENERAL>(c, px, q) : walk == 1 ? hitRecord<TRAV_FAST>(c, px, q)
                                                                                   : hitRecord<TRAV_FAST | TRAV_IDENTITY>(c, px, q);
#if defined(YART_EMULATE_LEAN_HANDOVER)
    if (walk == 0)
      for (int fast = 1; fast <= (c.im.allIdentity ? 2 : 1); fast++) {
        const rayrec::Rec f = fast == 1 ? hitRecord<TRAV_FAST>(c, px, q) : hitRecord<TRAV_FAST | TRAV_IDENTITY>(c, px, q);
        if (f.deferred) continue;
        bool same = f.hit == r.hit && f.draw == r.draw;
        if (q.kind) same = same && (f.hit || std::memcmp(f.att, r.att, 12) == 0);
        else same = same && std::memcmp(&f, &r, sizeof(f)) == 0;
        if (!same) {
          differ++;
          std::fprintf(stderr, "HITS differs: ray %zu kind %u walk %d: kept hit %u t %.9g tri %u | general hit %u t %.9g tri %u\n", k, q.kind, fast,
                       f.hit, f.t, f.tri, r.hit, r.t, r.tri);
        }
      }
#endif
    out.push_back(r);
    k++;
  }
  rayrec::save(outPath, out);
  std::printf("{\"hits\": \"ok\", \"rays\": %zu, \"walk\": %d, \"kept_rays_that_differ\": %zu}\n", k, walk, differ);
  return 0;
}

// shade: one record per case of a case file (oracle/shaderec.hpp) through csrc/shade_record.hpp — the function k_probe_shading
// runs. entries: 0 the plain entries (bsdfF / bsdfPdf / bsdfSample, what the KAT goes through), 1 one matEvaluate and the *ImplE
// entries in the local frame, as wfShade calls them.
static int doShade(Ctx& c, const std::string& casesPath, const std::string& outPath, int entries) {
  if (entries < 0 || entries > 1) { std::fprintf(stderr, "shade: entries must be 0 (plain) or 1 (matEvaluate + *ImplE)\n"); return 2; }
  std::vector<uint32_t> dims;
  for (uint32_t t = 0; t < c.sc.nTextures; t++) { dims.push_back(c.sc.textures[t].width); dims.push_back(c.sc.textures[t].height); }
  std::vector<shaderec::Rec> out;
  const auto cases = shaderec::load(casesPath);
  for (size_t k = 0; k < cases.size(); k++) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(&cases[k]);
    if (const char* why = shadeCaseProblem(q, uint32_t(c.im.nMaterials), c.sc.nTextures, c.sc.nLights, dims.data())) {
      std::fprintf(stderr, "shade: case %zu: %s\n", k, why);
      return 2;
    }
    shaderec::Rec r;
    shadeCaseRecord(c.sc, q, entries == 1, r.w);
    out.push_back(r);
  }
  shaderec::save(outPath, out);
  std::printf("{\"shade\": \"ok\", \"cases\": %zu, \"entries\": %d}\n", cases.size(), entries);
  return 0;
}

// need(leaf) = 0, need(inner) = 1 + max(need(left), need(right)) of every mesh, through the function scene creation uses
static std::string meshNeedsJson(const Ctx& c) {
  std::string s = "[";
  for (size_t m = 0; m < c.im.meshes.size(); m++) {
    const MeshDev& md = c.im.meshes[m];
    s += (m ? ", " : "") + std::to_string(bvhStackNeed(c.im.bvhNodes.data() + md.nodeOffset, md.nNodes));
  }
  return s + "]";
}

static int doRender(Ctx& c, const params::Params& p, const std::string& outPath, bool stackcheck = false) {
  const uint32_t W = p.width, H = p.height;
  std::vector<float> img(size_t(W) * H * 4, 0.0f);
  std::atomic<uint32_t> nextRow{0};
  std::atomic<uint64_t> totalRays{0};
  unsigned nt = p.threads ? p.threads : std::thread::hardware_concurrency();
  auto t0 = std::chrono::high_resolution_clock::now();
  StackMem stackMem(c, nt);
  StackProbe total;
  std::mutex totalLock;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      PathCtx px = pathCtx(c, stackMem, t);
      StackProbe probe;
      if (stackcheck) t_stackProbe = &probe;
      uint32_t rays = 0;
      int m = gmonBuckets(int32_t(p.spp));
      for (;;) {
        uint32_t y = nextRow++;
        if (y >= H) break;
        for (uint32_t x = 0; x < W; x++) {
          f3 acc[kGmonMax]; uint32_t cnt[kGmonMax];
          for (int b = 0; b < kGmonMax; b++) { acc[b] = mk3(0); cnt[b] = 0; }
          for (uint32_t s = 0; s < p.spp; s++) {
            f3 v = samplePixel(px, c.cam, x, y, s, rays) * c.cam.exposureScale;
            int b = int(s % uint32_t(m));
            if (gmonAccepts(v)) { acc[b] += v; cnt[b]++; }
          }
          f3 v = gmonFinish(acc, cnt, m);
          float* o = &img[(size_t(y) * W + x) * 4];
          // single wave: hdr = hdr*0 + wave*1 (tile-renderer.hpp:220-232)
          o[0] = 0.0f * 0.0f + v.x * 1.0f; o[1] = 0.0f * 0.0f + v.y * 1.0f; o[2] = 0.0f * 0.0f + v.z * 1.0f;
          o[3] = 1.0f;
        }
      }
      totalRays += rays;
      if (stackcheck) {
        t_stackProbe = nullptr;
        probe.flush();
        std::lock_guard<std::mutex> g(totalLock);
        total.rays += probe.rays; total.maxIndex = std::max(total.maxIndex, probe.maxIndex);
        for (int k = 0; k < 65; k++) { total.rayHist[k] += probe.rayHist[k]; total.handHist[k] += probe.handHist[k]; }
      }
    });
  for (auto& t : th) t.join();
  double sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
  FILE* f = std::fopen(outPath.c_str(), "wb");
  if (!f) return 2;
  std::fwrite(img.data(), 4, img.size(), f);
  std::fclose(f);
  if (stackcheck) {
    auto hist = [](const uint64_t* h) {
      std::string s = "[";
      for (int k = 0; k < 65; k++) s += (k ? ", " : "") + std::to_string(h[k]);
      return s + "]";
    };
    std::printf("{\"stackcheck\": \"ok\", \"mesh_need\": %s, \"tlas_height\": %u, \"stack_bound\": %u, \"lds_entries\": %u, \"spill_entries\": %u, "
                "\"traversals\": %llu, \"max_stack_index\": %u, \"ray_max_hist\": %s, \"handover_hist\": %s, \"rays\": %llu}\n",
                meshNeedsJson(c).c_str(), c.im.tlasHeight, c.im.stackBound, stackMem.split, stackMem.bound - stackMem.split,
                (unsigned long long) total.rays, total.maxIndex, hist(total.rayHist).c_str(), hist(total.handHist).c_str(),
                (unsigned long long) totalRays.load());
    return 0;
  }
  std::printf("{\"rays\": %llu, \"seconds\": %.6f, \"msamples_per_s\": %.6f, \"threads\": %u}\n",
              (unsigned long long) totalRays.load(), sec, double(W) * H * p.spp / sec * 1e-6, nt);
  return 0;
}

// stackbound: the stack bound of scene creation (host_scene.hpp: bvhStackNeed + checkStackBound) on a synthetic node array — a
// chain of `levels` inner nodes, each with a leaf and the next inner node as children. Finite f32 geometry does not drive the
// reference's builder far past the limit, a node array does.
static int doStackBound(unsigned levels) {
  std::vector<BvhNode> nodes(size_t(levels) * 2 + 1, BvhNode{});
  for (unsigned k = 0; k < levels; k++) {
    nodes[2 * k].leftFirst = 2 * k + 1; nodes[2 * k].span = 0;       // children at 2k + 1 (leaf), 2k + 2 (the chain goes on)
    nodes[2 * k + 1].leftFirst = k; nodes[2 * k + 1].span = 1;
  }
  nodes[2 * size_t(levels)].leftFirst = levels; nodes[2 * size_t(levels)].span = 1;
  const uint32_t need = bvhStackNeed(nodes.data(), nodes.size());
  std::string msg;
  try { checkStackBound(need, 0); } catch (const std::invalid_argument& e) { msg = e.what(); }
  std::printf("{\"stackbound\": \"ok\", \"levels\": %u, \"need\": %u, \"cap\": %u, \"refused\": %s, \"message\": \"%s\"}\n",
              levels, need, kMaxStackBound, msg.empty() ? "false" : "true", msg.c_str());
  return 0;
}

// stackops: stackPush / Pop / Peek / Poke of csrc/traverse.hpp on three interleaved lanes with `split` entries in one heap block
// and bound - split in another (exact sizes: an index past either is an AddressSanitizer report), against a plain array.
static int doStackOps(unsigned split, unsigned bound) {
  const unsigned lanes = 3;
  std::unique_ptr<uint64_t[]> lds(new uint64_t[size_t(split) * lanes]), spill(new uint64_t[size_t(bound - split) * lanes]);
  for (size_t k = 0; k < size_t(split) * lanes; k++) lds[k] = ~0ull;
  for (size_t k = 0; k < size_t(bound - split) * lanes; k++) spill[k] = ~0ull;
  TravStack st[lanes];
  for (unsigned l = 0; l < lanes; l++) {
    st[l].lds = lds.get() + l; st[l].ldsStride = lanes; st[l].ldsDepth = split;
    st[l].spill = spill.get() + l; st[l].spillStride = lanes;
  }
  auto node = [](unsigned l, unsigned k, unsigned gen) { return (l + 1u) * 100000u + k * 7u + gen; };
  auto dist = [](unsigned l, unsigned k, unsigned gen) { return float(l) * 1000.0f + float(k) + 0.25f * float(gen); };
  auto word = [&](unsigned l, unsigned k, unsigned gen) {
    return uint64_t(node(l, k, gen)) | (uint64_t(__builtin_bit_cast(uint32_t, dist(l, k, gen))) << 32);
  };
  auto fail = [&](const char* what, unsigned l, unsigned k) { std::fprintf(stderr, "stackops: %s, lane %u entry %u (split %u)\n", what, l, k, split); return 3; };
  for (unsigned k = 0; k < bound; k++)
    for (unsigned l = 0; l < lanes; l++) stackPush(st[l], k, node(l, k, 0), dist(l, k, 0));
  for (unsigned l = 0; l < lanes; l++)
    for (unsigned k = 0; k < bound; k++) if (stackPeek(st[l], k) != word(l, k, 0)) return fail("peek after push", l, k);
  for (unsigned k = 0; k < bound; k++)
    for (unsigned l = 0; l < lanes; l++) if ((k + l) % 2u) stackPoke(st[l], k, word(l, k, 1));
  for (unsigned l = 0; l < lanes; l++)
    for (unsigned k = bound; k-- > 0;) {
      uint32_t n; float d;
      stackPop(st[l], k, n, d);
      const unsigned gen = (k + l) % 2u;
      if (n != node(l, k, gen) || d != dist(l, k, gen)) return fail("pop after poke", l, k);
      if (stackPeek(st[l], k) != word(l, k, gen)) return fail("peek after poke", l, k);
    }
  std::printf("{\"stackops\": \"ok\", \"split\": %u, \"bound\": %u}\n", split, bound);
  return 0;
}

// selftest: the table-driven forms of the device headers against their direct forms, on the host.
//  * ZSobol index: SamplerTables entry + remaining digits == the reference's digit loop, for every
//    log2spp / tile size combination, random pixels, dimensions and samples;
//  * Sobol' dimension-1 byte tables == the bit loop;
//  * CDF search with a guide table == the plain lower-bound search, on random and degenerate CDFs.
static int doSelfTest() {
  struct { uint64_t s = 0x5eed5eedull; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return uint32_t(s >> 32); } } rng;
  uint64_t checked = 0;
  std::vector<uint32_t> matrix52(52);
  for (uint32_t k = 0; k < 52; k++) matrix52[k] = sobolDim1Column(k);
  std::vector<uint32_t> byteTab(8 * 256);
  for (uint32_t k = 0; k < 8 * 256; k++) {
    uint32_t b = k >> 8, v = k & 255u, x = 0;
    for (uint32_t j = 0; j < 8; j++) if (((v >> j) & 1u) && 8 * b + j < 52) x ^= matrix52[8 * b + j];
    byteTab[k] = x;
  }
  for (uint32_t spp : {1u, 2u, 3u, 4u, 8u, 12u, 16u, 32u, 48u, 64u, 128u, 256u, 512u, 1024u, 2048u}) {
    for (uint32_t tile : {8u, 64u, 100u, 512u, 4096u}) {
      SamplerConfig cfg = makeSamplerConfig(spp, tile);
      if (uint64_t(spp) > (1ull << cfg.log2spp)) continue;      // the renderer disables the tables here
      const uint32_t dims = 40, nPix = 24;
      std::vector<uint32_t> px(nPix), py(nPix);
      std::vector<uint64_t> entries(size_t(dims) * nPix), hash(dims + 3);
      for (uint32_t i = 0; i < nPix; i++) { px[i] = rng.next() % 4000u; py[i] = rng.next() % 3000u; }
      for (uint32_t d = 0; d < dims; d++)
        for (uint32_t i = 0; i < nPix; i++) entries[size_t(i) * dims + d] = samplerTableEntry(cfg, encodeMorton2(px[i], py[i]), d);
      for (uint32_t d = 0; d < dims + 3; d++) hash[d] = hashDim(d);
      SamplerConfig tcfg = cfg;
      tcfg.tab.entries = entries.data(); tcfg.tab.hash = hash.data(); tcfg.tab.sobol1 = byteTab.data();
      tcfg.tab.dims = dims; tcfg.tab.stride = nPix;
      for (uint32_t i = 0; i < nPix; i++) {
        for (uint32_t rep = 0; rep < 40; rep++) {
          Sampler a, b;
          startPixelSample(a, cfg, px[i], py[i], rng.next() % spp);
          a.dim = rng.next() % (dims + 6);                      // also beyond the table: fallback
          b = a; b.pix = i;
          if (getSampleIndexDirect(a, cfg) != getSampleIndex(b, tcfg)) {
            std::fprintf(stderr, "selftest: sample index mismatch spp=%u tile=%u dim=%u\n", spp, tile, a.dim);
            return 3;
          }
          Sampler a2 = a, b2 = b;
          f2 u0 = get2D(a2, cfg, matrix52.data()), u1 = get2D(b2, tcfg, matrix52.data());
          float v0 = get1D(a2, cfg), v1 = get1D(b2, tcfg);
          if (std::memcmp(&u0, &u1, sizeof(u0)) != 0 || std::memcmp(&v0, &v1, 4) != 0 || a2.dim != b2.dim) {
            std::fprintf(stderr, "selftest: sample value mismatch spp=%u tile=%u dim=%u\n", spp, tile, a.dim);
            return 3;
          }
          checked++;
        }
      }
    }
  }
  // v % 24 of the permutation-row selection: the multiply-free form against the operator, random and edge 40-bit values
  for (uint64_t k = 0; k < 400000; k++) {
    uint64_t v = (uint64_t(rng.next()) << 8 | (rng.next() & 0xffu)) & 0xffffffffffull;
    if (k < 64) v = k;
    else if (k < 128) v = 0xffffffffffull - (k - 64);
    else if (k < 192) v = (1ull << (k - 128 < 40 ? k - 128 : 39)) - (k & 1);
    if (mod24of40(v) != uint32_t(v % 24ull)) { std::fprintf(stderr, "selftest: mod24of40(%llu)\n", (unsigned long long) v); return 3; }
    checked++;
  }
  // CDF search
  for (uint32_t n : {1u, 2u, 3u, 7u, 64u, 100u, 1000u}) {
    for (int kind = 0; kind < 4; kind++) {
      std::vector<float> func(n), cdf(n + 1);
      for (uint32_t k = 0; k < n; k++) {
        float f = float(rng.next() % 1000u) / 1000.0f;
        if (kind == 1) f = (k % 5 == 0) ? f : 0.0f;             // long zero runs (flat CDF segments)
        if (kind == 2) f = (k == n / 2) ? 1.0f : 0.0f;          // a single spike
        if (kind == 3) f = 0.0f;                                // all zero -> uniform CDF
        func[k] = f;
      }
      cdf[0] = 0.0f;
      for (uint32_t k = 1; k <= n; k++) cdf[k] = cdf[k - 1] + func[k - 1] / float(n);
      const float integral = cdf[n];
      for (uint32_t k = 1; k <= n; k++) cdf[k] = integral == 0.0f ? float(k) / float(n) : cdf[k] / integral;
      uint32_t K = 1; while (K < n) K <<= 1;
      std::vector<uint32_t> guide;
      uint32_t idx = 1;
      for (uint32_t j = 0; j <= K; j++) {
        const float uj = float(j) / float(K);
        while (idx < n && cdf[idx] < uj) idx++;
        guide.push_back(idx);
      }
      // the interleaved records the environment sampling walks (lights.hpp::pc1dSampleRecords), strides 2 and 4
      std::vector<float> rec2(size_t(n + 1) * 2, 0.0f), rec4(size_t(n + 1) * 4, 0.0f);
      for (uint32_t k = 0; k <= n; k++) {
        rec2[size_t(k) * 2] = rec4[size_t(k) * 4] = cdf[k];
        if (k < n) rec2[size_t(k) * 2 + 1] = rec4[size_t(k) * 4 + 1] = func[k];
      }
      for (uint32_t rep = 0; rep < 4000; rep++) {
        float u = float(rng.next() & 0xffffffu) * 0x1p-24f;
        if (rep % 7 == 0) u = cdf[rng.next() % (n + 1)];        // exactly on a CDF value
        if (u >= 1.0f) u = kOneMinusEpsilon;
        float pdf0, pdf1; uint32_t o0, o1;
        float x0 = pc1dSample(func.data(), cdf.data(), n, integral, 0.0f, 1.0f, u, pdf0, o0);
        float x1 = pc1dSample(func.data(), cdf.data(), n, integral, 0.0f, 1.0f, u, pdf1, o1, guide.data(), K);
        if (o0 != o1 || std::memcmp(&x0, &x1, 4) != 0 || std::memcmp(&pdf0, &pdf1, 4) != 0) {
          std::fprintf(stderr, "selftest: guided CDF search mismatch n=%u kind=%d u=%a (%u vs %u)\n", n, kind, u, o0, o1);
          return 3;
        }
        float pdf2, pdf3; uint32_t o2, o3;
        const float x2 = pc1dSampleRecords<2>(rec2.data(), n, integral, cdf[1], u, pdf2, o2, guide.data(), K);
        const float x3 = pc1dSampleRecords<4>(rec4.data(), n, integral, cdf[1], u, pdf3, o3, nullptr, 0);
        if (o0 != o2 || o0 != o3 || std::memcmp(&x0, &x2, 4) != 0 || std::memcmp(&x0, &x3, 4) != 0 || std::memcmp(&pdf0, &pdf2, 4) != 0 ||
            std::memcmp(&pdf0, &pdf3, 4) != 0) {
          std::fprintf(stderr, "selftest: record-form CDF search mismatch n=%u kind=%d u=%a\n", n, kind, u);
          return 3;
        }
        checked++;
      }
    }
  }
  // device log2f / powf (libm_pow.hpp) against this machine's libm: a dense random sweep (the exhaustive
  // one — every float, ten exponents, 0 mismatches — takes minutes and was run once)
  {
    const float ys[] = {1.0f, 0.8f, 1.35f, 2.2f, 1.0f / 2.2f};
    for (uint32_t rep = 0; rep < 1500000; rep++) {
      uint32_t bits = rng.next();
      if (rep % 3 == 0) bits = (bits & 0x007fffffu) | ((118u + rng.next() % 14u) << 23);   // around [2^-9, 2^5)
      const float x = __builtin_bit_cast(float, bits);
      const float a = libm_pow::log2f_(x), b = std::log2(x);
      bool ok = (a != a && b != b) || std::memcmp(&a, &b, 4) == 0;
      for (float y : ys) {
        const float c = libm_pow::powf_(x, y), d = std::pow(x, y);
        ok = ok && ((c != c && d != d) || std::memcmp(&c, &d, 4) == 0);
      }
      if (!ok) { std::fprintf(stderr, "selftest: log2f / powf emulation differs from libm at x=%a\n", x); return 3; }
      checked++;
    }
  }
  // byte / 255.0f of the texture fetch (bsdf.hpp byteToUnit) against the IEEE divide, all 256 numerators
  for (uint32_t b = 0; b < 256; b++) {
    volatile float x = float(b), c = 255.0f;
    const float q = x / c, r = byteToUnit(b);
    if (std::memcmp(&q, &r, 4) != 0) { std::fprintf(stderr, "selftest: byteToUnit(%u) differs from %u / 255.0f\n", b, b); return 3; }
    checked++;
  }
  std::printf("{\"selftest\": \"ok\", \"checked\": %llu}\n", (unsigned long long) checked);
  return 0;
}

// libm: the device's libm emulation (csrc/ymath.hpp libm_emul, compiled for the host: __builtin_fma is libm's correctly rounded
// fma here) against this machine's libm, bit for bit (NaN == NaN), over the domains tests/test_device_math.py sweeps on the GPU at
// full density — here at a stride, with the windows of +-4096 bit patterns around every branch constant and the special values
// always at full density. log2f / powf (libm_pow.hpp) have their sweep in `selftest`.
namespace libmcheck {
typedef float (*Fn)(float);
struct Sweep { const char* name; Fn emul; Fn volatile libm; uint64_t checked = 0, bad = 0; };
static uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
static void one(Sweep& s, uint32_t bits) {
  const float x = __builtin_bit_cast(float, bits);
  const float a = s.emul(x), b = s.libm(x);
  s.checked++;
  if (fbits(a) == fbits(b) || (a != a && b != b)) return;
  if (s.bad++ < 8) std::fprintf(stderr, "libm: %s(%a = 0x%08x): emulation 0x%08x, this machine's libm 0x%08x\n", s.name, x, bits, fbits(a), fbits(b));
}
// [lo, hi] at `stride`, both ends included; with `bothSigns` the mirrored negative range too
static void range(Sweep& s, uint32_t lo, uint32_t hi, uint32_t stride, bool bothSigns) {
  for (uint64_t b = lo; b <= hi; b += stride) { one(s, uint32_t(b)); if (bothSigns) one(s, uint32_t(b) | 0x80000000u); }
  one(s, hi); if (bothSigns) one(s, hi | 0x80000000u);
}
static void window(Sweep& s, float c) {
  const uint32_t b = fbits(c);
  range(s, b - 4096u, b + 4096u, 1, true);
}
static void specials(Sweep& s) {
  const uint32_t sp[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u, 0x7f7fffffu, 0xff7fffffu,
                         0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7fffffffu};
  for (uint32_t b : sp) one(s, b);
}
}  // namespace libmcheck

static int doLibmCheck() {
  using namespace libmcheck;
  const uint32_t twoPi = fbits(0x1.921fb6p+2f), fltMax = 0x7f7fffffu;
  Sweep sw[6] = {{"sinf", libm_emul::sinf_, sinf}, {"cosf", libm_emul::cosf_, cosf}, {"sinf (2 pi form)", libm_emul::sinf2pi_, sinf},
                 {"cosf (2 pi form)", libm_emul::cosf2pi_, cosf}, {"logf", libm_emul::logf_, logf}, {"expf", libm_emul::expf_, expf}};
  for (int k = 0; k < 4; k++) {
    Sweep& s = sw[k];
    range(s, 0u, twoPi, 167, false);                              // the reachable domain [0, 2 pi]
    window(s, 0x1p-12f); window(s, 0x1.921FB6p-1f);
    range(s, twoPi - 4096u, twoPi, 1, false);
    if (k >= 2) continue;                                         // the 2 pi forms are defined on [0, 120) only
    range(s, twoPi, fbits(120.0f) - 1u, 64 * 7, true);
    window(s, 120.0f);
    range(s, fbits(120.0f), fltMax, 4096 * 3, true);              // the |x| >= 120 tail
    specials(s);
  }
  {
    Sweep& s = sw[4];
    range(s, 0u, 0x3f800000u, 89, false);                        // [+0, 1]: the sampler's values
    range(s, 0u, 4096u, 1, false); window(s, 0x1p-126f); window(s, 1.0f); window(s, 0x1.66p-1f);
    range(s, 0x3f800000u, fltMax, 64 * 61, false);
    range(s, 0x80000000u, 0xff800000u, 65536 * 3 + 1, false);     // negative: NaN
    specials(s);
  }
  {
    Sweep& s = sw[5];
    range(s, fbits(0x1p-40f), fbits(104.0f), 37, true);
    window(s, 80.0f); window(s, 88.0f); window(s, 0x1.62e42ep6f); window(s, 0x1.9fe368p6f); window(s, 0x1.9d1d9ep6f); window(s, 104.0f);
    range(s, 0u, fbits(0x1p-40f), 4096, true);                    // +-0, denormals, tiny
    range(s, fbits(104.0f), fltMax, 4096, true);
    specials(s);
    one(s, 0x4202422fu); one(s, 0xc27c65d9u);                     // the two inputs a product rounded before "z - kd" gets wrong (ymath.hpp expf_)
  }
  uint64_t checked = 0, bad = 0;
  for (const Sweep& s : sw) { checked += s.checked; bad += s.bad; }
  if (bad) {
    std::fprintf(stderr, "libm: %llu of %llu results of the device's libm emulation differ from this machine's libm. Either csrc/ymath.hpp was "
                 "edited, or this machine's glibc selects other sinf / cosf / logf / expf variants than the FMA forms of glibc 2.35 the emulation "
                 "states (the YART_ALLOW_LIBM_DRIFT scenario): then the frame tests' bit identity cannot hold here either.\n",
                 (unsigned long long) bad, (unsigned long long) checked);
    return 3;
  }
  std::printf("{\"libm\": \"ok\", \"checked\": %llu}\n", (unsigned long long) checked);
  return 0;
}

// tonemap: csrc/tonemap.hpp (the device functions, compiled for the host) over an RGBA32F file
static int doTonemap(const char* in, unsigned w, unsigned h, const std::string& look, const char* outF32, const char* outPpm) {
  std::vector<float> px(size_t(w) * h * 4);
  FILE* f = std::fopen(in, "rb");
  if (!f || std::fread(px.data(), 4, px.size(), f) != px.size()) { std::fprintf(stderr, "tonemap: short input\n"); return 2; }
  std::fclose(f);
  const int lk = look == "golden" ? 1 : look == "punchy" ? 2 : look == "none" ? 0 : -1;
  std::vector<uint8_t> bytes(size_t(w) * h * 3);
  for (size_t i = 0; i < size_t(w) * h; i++) {
    if (lk >= 0) {
      const f3 o = agxTonemap(mk3(px[4 * i], px[4 * i + 1], px[4 * i + 2]), agxLook(lk));
      px[4 * i] = o.x; px[4 * i + 1] = o.y; px[4 * i + 2] = o.z; px[4 * i + 3] = 1.0f;
    }
    for (int c = 0; c < 3; c++) bytes[3 * i + c] = ppmByte(px[4 * i + c]);
  }
  f = std::fopen(outF32, "wb"); std::fwrite(px.data(), 4, px.size(), f); std::fclose(f);
  f = std::fopen(outPpm, "wb"); std::fprintf(f, "P6\n%u %u\n255\n", w, h); std::fwrite(bytes.data(), 1, bytes.size(), f); std::fclose(f);
  return 0;
}

// estimator: csrc/estimator.hpp (the functions k_gmon_blend runs, compiled for the host) over groups of `spp`
// RGB samples; sample k goes to bucket k mod m in increasing k, exactly as the kernel's lanes do.
static int doEstimator(int kind, unsigned spp, const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) { std::fprintf(stderr, "estimator: cannot open input\n"); return 2; }
  std::vector<float> smp;
  float buf[3];
  while (std::fread(buf, 4, 3, f) == 3) smp.insert(smp.end(), buf, buf + 3);
  std::fclose(f);
  const size_t groups = smp.size() / 3 / spp;
  std::vector<float> res(groups * 3);
  const int m = estimatorBuckets(kind, int32_t(spp));
  for (size_t g = 0; g < groups; g++) {
    f3 acc[kGmonMax]; uint32_t cnt[kGmonMax];
    for (int b = 0; b < m; b++) {
      acc[b] = mk3(0); cnt[b] = 0;
      for (unsigned k = unsigned(b); k < spp; k += unsigned(m)) {
        const float* p = &smp[(g * spp + k) * 3];
        const f3 v = mk3(p[0], p[1], p[2]);
        if (estimatorAccepts(kind, v)) { acc[b] += v; cnt[b]++; }
      }
    }
    const f3 v = estimatorFinish(kind, acc, cnt, m, spp);
    res[3 * g] = v.x; res[3 * g + 1] = v.y; res[3 * g + 2] = v.z;
  }
  f = std::fopen(out, "wb"); std::fwrite(res.data(), 4, res.size(), f); std::fclose(f);
  return 0;
}


// bvhcheck: the task-parallel BVH build against the plain recursion, every mesh of a scene, byte for byte
static int doBvhCheck(const char* scenePath, unsigned threads) {
  auto loaded = loadSceneFile(scenePath);
  double msSerial = 0, msParallel = 0;
  size_t nodes = 0, tris = 0;
  uint32_t maxLeaf = 0;
  for (uint32_t m = 0; m < loaded->desc.n_meshes; m++) {
    const YartMeshDesc& md = loaded->desc.meshes[m];
    SahBvhBuilder a, b;
    a.setThreads(1); b.setThreads(threads);
    auto t0 = std::chrono::steady_clock::now();
    a.build(md.positions, md.faces, 4, md.n_faces);
    auto t1 = std::chrono::steady_clock::now();
    b.build(md.positions, md.faces, 4, md.n_faces);
    auto t2 = std::chrono::steady_clock::now();
    msSerial += std::chrono::duration<double, std::milli>(t1 - t0).count();
    msParallel += std::chrono::duration<double, std::milli>(t2 - t1).count();
    if (a.nodes.size() != b.nodes.size() || std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(BvhNode)) != 0 ||
        a.indices != b.indices) {
      std::fprintf(stderr, "bvhcheck: mesh %u differs between 1 and %u threads\n", m, threads);
      return 3;
    }
    nodes += a.nodes.size(); tris += md.n_faces;
    for (const BvhNode& n : a.nodes) maxLeaf = std::max(maxLeaf, n.span);
  }
  const float share = buildHostImage(loaded->desc).dominantLobeShare;
  std::printf("{\"bvhcheck\": \"ok\", \"dominant_lobe_share\": %.4f, \"meshes\": %u, \"triangles\": %zu, \"nodes\": %zu, \"max_leaf_span\": %u, \"threads\": %u, \"ms_serial\": %.1f, \"ms_parallel\": %.1f}\n",
              share, loaded->desc.n_meshes, tris, nodes, maxLeaf, threads, msSerial, msParallel);
  return 0;
}

// bvhsum: the "bvh" section of the kat files alone, from the host builder (csrc/bvh_build.hpp) on `threads` threads: per mesh of the
// scene the node count, the FNV-1a of the node words and the FNV-1a of the index array — what the "bvh" section of `yart_ref kat` holds for the
// reference's trees (tests/bvhsuite.py, tests/golden/bvh/README.md: the mutation table is made with this mode)
static int doBvhSum(const char* scenePath, unsigned threads, const char* outPath) {
  auto loaded = loadSceneFile(scenePath);
  std::vector<uint64_t> out;
  for (uint32_t m = 0; m < loaded->desc.n_meshes; m++) {
    const YartMeshDesc& md = loaded->desc.meshes[m];
    SahBvhBuilder b;
    b.setThreads(threads);
    b.build(md.positions, md.faces, 4, md.n_faces);
    out.push_back(b.nodes.size());
    out.push_back(kat::fnv1a(b.nodes.data(), b.nodes.size() * sizeof(BvhNode)));
    out.push_back(kat::fnv1a(b.indices.data(), b.indices.size() * 4));
  }
  kat::Writer w(outPath);
  w.u64("bvh", out);
  return 0;
}

// loadstress: N concurrent host callers of the scene loader and the scene build (what N threads holding their own YartScene
// handles do on the host before anything reaches a device): .yscn parse, flattening, the task-parallel SAH build with its own
// worker pool inside every caller. Every caller must arrive at the same image (node array hashed). Run under
// -fsanitize=thread by tests/test_sanitizers.py: shared mutable state between callers would show as a race.
static int doLoadStress(const char* scenePath, unsigned callers) {
  std::vector<uint64_t> sig(callers, 0);
  std::vector<std::string> err(callers);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < callers; t++)
    th.emplace_back([&, t] {
      try {
        auto loaded = loadSceneFile(scenePath);
        HostImage im = buildHostImage(loaded->desc);
        uint64_t h = 0xcbf29ce484222325ull;
        const uint8_t* b = reinterpret_cast<const uint8_t*>(im.bvhNodes.data());
        for (size_t k = 0; k < im.bvhNodes.size() * sizeof(BvhNode); k++) h = (h ^ b[k]) * 0x100000001b3ull;
        const uint8_t* l = reinterpret_cast<const uint8_t*>(im.leafTris.data());
        for (size_t k = 0; k < im.leafTris.size() * sizeof(LeafTri); k++) h = (h ^ l[k]) * 0x100000001b3ull;
        sig[t] = h;
      } catch (const std::exception& e) { err[t] = e.what(); }
    });
  for (auto& x : th) x.join();
  for (unsigned t = 0; t < callers; t++) {
    if (!err[t].empty()) { std::fprintf(stderr, "loadstress: caller %u: %s\n", t, err[t].c_str()); return 2; }
    if (sig[t] != sig[0]) { std::fprintf(stderr, "loadstress: caller %u built a different image\n", t); return 3; }
  }
  std::printf("{\"loadstress\": \"ok\", \"callers\": %u, \"signature\": \"%016llx\"}\n", callers, (unsigned long long) sig[0]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "selftest") return doSelfTest();
  if (argc == 2 && std::string(argv[1]) == "libm") return doLibmCheck();
  if (argc == 3 && std::string(argv[1]) == "stackbound") return doStackBound(unsigned(std::atoi(argv[2])));
  if (argc == 4 && std::string(argv[1]) == "stackops") {     // split 0: every split from 1 to the bound
    const unsigned split = unsigned(std::atoi(argv[2])), bound = unsigned(std::atoi(argv[3]));
    for (unsigned k = split ? split : 1u; k <= (split ? split : bound); k++) if (int rc = doStackOps(k, bound)) return rc;
    return 0;
  }
  if (argc == 4 && std::string(argv[1]) == "loadstress") return doLoadStress(argv[2], unsigned(std::atoi(argv[3])));
  if (argc == 4 && std::string(argv[1]) == "bvhcheck") return doBvhCheck(argv[2], unsigned(std::atoi(argv[3])));
  if (argc == 5 && std::string(argv[1]) == "bvhsum") return doBvhSum(argv[2], unsigned(std::atoi(argv[3])), argv[4]);
  if (argc == 6 && std::string(argv[1]) == "estimator")
    return doEstimator(std::atoi(argv[2]), unsigned(std::atoi(argv[3])), argv[4], argv[5]);
  if (argc == 8 && std::string(argv[1]) == "tonemap")
    return doTonemap(argv[2], unsigned(std::atoi(argv[3])), unsigned(std::atoi(argv[4])), argv[5], argv[6], argv[7]);
  const bool hits = (argc == 6 || argc == 7) && std::string(argv[1]) == "hits";
  const bool shade = (argc == 6 || argc == 7) && std::string(argv[1]) == "shade";
  if (argc != 5 && !hits && !shade) {
    std::fprintf(stderr, "usage: hostsim kat|render|stackcheck|shade-kat-cases <scene.yscn> <params.txt> <out> | hits <scene.yscn> <params.txt> <rays.bin> <out.bin> [walk]"
                         " | shade <scene.yscn> <params.txt> <cases.bin> <out.bin> [entries]\n");
    return 1;
  }
  try {
    auto loaded = loadSceneFile(argv[2]);
    auto p = params::load(argv[3]);
    Ctx c;
    c.im = buildHostImage(loaded->desc);
    c.sc = c.im.view();
    c.cam = makeCamera(cameraDesc(p));
    c.rc.sampler = makeSamplerConfig(p.spp, p.tile);
    c.rc.maxDepth = p.depth;
    c.rc.background = mk3(p.background[0], p.background[1], p.background[2]);
    std::string mode = argv[1];
    if (hits) return doHits(c, argv[4], argv[5], argc == 7 ? std::atoi(argv[6]) : 0);
    if (shade) return doShade(c, argv[4], argv[5], argc == 7 ? std::atoi(argv[6]) : 0);
    if (mode == "shade-kat-cases") { shaderec::save(argv[4], katShadeCases(c.im.nMaterials, c.sc.nLights)); return 0; }
    if (mode == "kat") return doKat(c, p, argv[4]);
    if (mode == "render") return doRender(c, p, argv[4]);
    if (mode == "stackcheck") return doRender(c, p, argv[4], true);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "hostsim: %s\n", e.what());
    return 2;
  }
  return 1;
}
