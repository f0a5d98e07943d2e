// denoise.hpp — edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) guided by the first-hit feature
// buffers: the arithmetic, as inline functions for the device kernels (denoise_kernels.inc) and for the host (tests/denoisesim/dn_host.hpp).
//
// The definition is the comment above yart_hip_denoise_atrous_device in include/yart_hip.h; this file states it operation by
// operation: every operation an individually rounded binary32 operation in the order written (the build has no FMA contraction),
// exponentials through yexpf, logarithms through ylogf (ymath.hpp: glibc's values on the device).
//
// Per pixel the filter keeps two 16-byte words while it runs, 48 bytes with the second working image:
//   colour  {c.r, c.g, c.b, fourth word}          the working colour of iteration i (two images, read one, write the other)
//   guide   {n.x, n.y, n.z, lz}                   written once by the prepare pass
// The per-channel divisor of the demodulation is not stored: the finish pass forms it again from the caller's albedo buffer,
// which the call never writes.
//
// The filter has two forms, chosen at compile time by VAR; they share every line below except the four places that ask for VAR:
//   plain (VAR = false, yart_hip_denoise_atrous_*): that definition as it stands.
//   variance-guided (VAR = true, yart_hip_denoise_atrous_var_*; the spatial filter of SVGF, Schied et al. 2017): the
//   colour term is measured against the local standard deviation of the luminance, and the variance is filtered along.
// The four places:
//   1. the fourth word of the working colour   plain: valid (u32 0 / 1). variance-guided: the variance v_i(p) of a valid pixel,
//                                              kDnVarInvalid for an invalid one (all ones: no arithmetic produces that NaN).
//   2. the centre pixel's part of the colour term   plain: icol * 4^i. variance-guided: luma(c_i(p)) and the 3 x 3 Gaussian of v_i.
//   3. the colour term of a tap                plain: |dc|^2 * (icol * 4^i). variance-guided: |dluma| / (sigma_luma * sqrt(g) + 1e-6).
//   4. what the fourth word carries on         plain: valid(p). variance-guided: v_(i+1)(p), filtered with the squared weights.
#pragma once
#include "ymath.hpp"

namespace yart_hip {

constexpr uint32_t kDnColor = 1u, kDnNormal = 2u, kDnDepth = 4u;   // DnConst::terms: the terms of e that exist
constexpr uint32_t kDnVarInvalid = 0xffffffffu;

struct DnConst {
  union {                      // one float; each form writes and reads its own name only
    float icol;                // plain: 1 / (sigma_color * sigma_color) (0 where the term does not exist)
    float sigmaLuma;           // variance-guided: sigma_luma itself
  };
  float inrm, idep;            // 1 / (sigma * sigma), formed once on the host in fp32 (0 where the term does not exist)
  uint32_t terms;              // kDn*
};

YART_HD uint32_t dnBits(float f) { return __builtin_bit_cast(uint32_t, f); }
YART_HD f4 dnF4(float x, float y, float z, float w) { f4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
YART_HD bool dnFinite(float v) { return (dnBits(v) & 0x7f800000u) != 0x7f800000u; }
YART_HD float dnKernel(int a) { return a == 0 ? 0.375f : (a == 1 || a == -1) ? 0.25f : 0.0625f; }
YART_HD float dnKernel3(int a) { return a == 0 ? 0.5f : 0.25f; }   // 3x3 Gaussian: 0.25 centre, 0.125 edge, 0.0625 corner
YART_HD float dnLuma(float r, float g, float b) { return r * 0.2126f + g * 0.7152f + b * 0.0722f; }   // estimator.hpp luma

// is the pixel whose working colour has this fourth word valid? (difference 1: the two encodings stay apart)
template <bool VAR>
YART_HD bool dnWordValid(float w) { return VAR ? dnBits(w) != kDnVarInvalid : dnBits(w) != 0u; }

// 1 / (sigma * sigma); a sigma <= 0 switches its term off (host side, fp32)
inline float dnInvSigma2(float sigma) { return sigma > 0.0f ? 1.0f / (sigma * sigma) : 0.0f; }

// The constants of a call (host side): sigmaFirst is sigma_color (plain) or sigma_luma (variance-guided); a guide that is absent
// switches its term off as a sigma <= 0 does.
template <bool VAR>
inline DnConst dnConstants(float sigmaFirst, float sigmaNormal, float sigmaDepth, bool haveNormal, bool haveDepth) {
  DnConst k;
  if constexpr (VAR) k.sigmaLuma = sigmaFirst; else k.icol = dnInvSigma2(sigmaFirst);
  k.inrm = haveNormal ? dnInvSigma2(sigmaNormal) : 0.0f;
  k.idep = haveDepth ? dnInvSigma2(sigmaDepth) : 0.0f;
  k.terms = (sigmaFirst > 0.0f ? kDnColor : 0u) | (haveNormal && sigmaNormal > 0.0f ? kDnNormal : 0u) |
            (haveDepth && sigmaDepth > 0.0f ? kDnDepth : 0u);
  return k;
}

// d = alb > 1e-3f ? alb : 1.0f per channel; alb3 == nullptr: no demodulation, (1, 1, 1)
YART_HD f3 dnDivisor(const float* alb3) {
  if (!alb3) return mk3(1.0f);
  return mk3(alb3[0] > 1e-3f ? alb3[0] : 1.0f, alb3[1] > 1e-3f ? alb3[1] : 1.0f, alb3[2] > 1e-3f ? alb3[2] : 1.0f);
}

// Prepare pass of one pixel. alb3: the pixel's albedo when the call demodulates, else nullptr; nrm3 / dep: the pixel's normal /
// depth when that guide is present, else nullptr. variance is looked at by the variance-guided form only: v_0 = variance /
// (ld * ld), ld = luma(d), and a variance that is not finite or is negative makes the pixel invalid.
template <bool VAR = false>
YART_HD void dnPrepare(f4 rgba, const float* alb3, const float* nrm3, const float* dep, f4& colour, f4& guide, float variance = 0.0f) {
  const f3 d = dnDivisor(alb3);
  const float r = rgba.x / d.x, g = rgba.y / d.y, b = rgba.z / d.z;
  bool valid = dnFinite(r) && dnFinite(g) && dnFinite(b);
  if (alb3) valid = valid && dnFinite(alb3[0]) && dnFinite(alb3[1]) && dnFinite(alb3[2]);
  guide = dnF4(0.0f, 0.0f, 0.0f, 0.0f);
  if (nrm3) {
    guide.x = nrm3[0]; guide.y = nrm3[1]; guide.z = nrm3[2];
    valid = valid && dnFinite(nrm3[0]) && dnFinite(nrm3[1]) && dnFinite(nrm3[2]);
  }
  if (dep) {
    const float z = *dep;
    valid = valid && dnFinite(z);
    guide.w = ylogf(z > 1e-30f ? z : 1e-30f);
  }
  if constexpr (VAR) {
    valid = valid && dnFinite(variance) && variance >= 0.0f;
    const float ld = dnLuma(d.x, d.y, d.z);
    colour = dnF4(r, g, b, valid ? variance / (ld * ld) : __builtin_bit_cast(float, kDnVarInvalid));
  } else {
    colour = dnF4(r, g, b, __builtin_bit_cast(float, valid ? 1u : 0u));
  }
}

// One pixel of iteration i: reads image c_i through src.colour(q) / src.guide(q) (q = y * width + x), returns c_(i+1)(p) with the
// fourth word of p (difference 4). Src decides how a 16-byte word is fetched (global memory on the device, an array on the host).
template <bool VAR = false, class Src>
YART_HD f4 dnFilterPixel(const Src& src, uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t i, const DnConst& k) {
  const int s = 1 << i;
  const size_t p = size_t(y) * width + x;
  const f4 cp = src.colour(p);
  const bool validP = dnWordValid<VAR>(cp.w);
  const bool guided = (k.terms & (kDnNormal | kDnDepth)) != 0u;
  f4 gp = dnF4(0.0f, 0.0f, 0.0f, 0.0f);
  if (guided) gp = src.guide(p);
  float icolI = 0.0f, lyP = 0.0f, den = 1.0f;       // difference 2
  if constexpr (!VAR) {
    icolI = k.icol * float(1u << (2u * i));
  } else if (validP && (k.terms & kDnColor)) {
    // g(p): 3 x 3 Gaussian of v_i at distance 1 (whatever the step), over the valid pixels inside the image
    float gv = 0.0f, gk = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
      const int qy = int(y) + dy;
      if (qy < 0 || qy >= int(height)) continue;
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = int(x) + dx;
        if (qx < 0 || qx >= int(width)) continue;
        const f4 cq = src.colour(size_t(qy) * width + size_t(qx));
        if (!dnWordValid<VAR>(cq.w)) continue;
        const float kk = dnKernel3(dy) * dnKernel3(dx);
        gv = gv + kk * cq.w; gk = gk + kk;
      }
    }
    const float g = gk == 0.0f ? 0.0f : gv / gk;
    den = k.sigmaLuma * sqrtf(g) + 1e-6f;
    lyP = dnLuma(cp.x, cp.y, cp.z);
  }
  float accR = 0.0f, accG = 0.0f, accB = 0.0f, wsum = 0.0f, vacc = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = int(y) + s * dy;
    if (qy < 0 || qy >= int(height)) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = int(x) + s * dx;
      if (qx < 0 || qx >= int(width)) continue;
      const size_t q = size_t(qy) * width + size_t(qx);
      const f4 cq = src.colour(q);
      if (!dnWordValid<VAR>(cq.w)) continue;
      const float h = dnKernel(dy) * dnKernel(dx);
      float e = 0.0f;
      if (validP) {
        bool have = false;
        if (k.terms & kDnColor) {                   // difference 3
          if constexpr (VAR) {
            e = fabsf(dnLuma(cq.x, cq.y, cq.z) - lyP) / den;
          } else {
            const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
            const float dc = (dr * dr + dg * dg) + db * db;
            e = dc * icolI;
          }
          have = true;
        }
        if (guided) {
          const f4 gq = src.guide(q);
          if (k.terms & kDnNormal) {
            const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
            const float dn = (nx * nx + ny * ny) + nz * nz;
            const float t = dn * k.inrm;
            e = have ? e + t : t; have = true;
          }
          if (k.terms & kDnDepth) {
            const float dl = gq.w - gp.w;
            const float t = (dl * dl) * k.idep;
            e = have ? e + t : t;
          }
        }
      }
      const float w = h * yexpf(-e);
      accR = accR + w * cq.x; accG = accG + w * cq.y; accB = accB + w * cq.z;
      wsum = wsum + w;
      if constexpr (VAR) vacc = vacc + (w * w) * cq.w;
    }
  }
  float fourth = cp.w;                              // difference 4
  if constexpr (VAR) fourth = !validP ? __builtin_bit_cast(float, kDnVarInvalid) : wsum == 0.0f ? 0.0f : vacc / (wsum * wsum);
  if (wsum == 0.0f) return dnF4(0.0f, 0.0f, 0.0f, fourth);
  return dnF4(accR / wsum, accG / wsum, accB / wsum, fourth);
}

// The variance-guided form under the names host programs written against this header call it by
using DnVarConst = DnConst;
YART_HD void dnPrepareVar(f4 rgba, float variance, const float* alb3, const float* nrm3, const float* dep, f4& colour, f4& guide) {
  dnPrepare<true>(rgba, alb3, nrm3, dep, colour, guide, variance);
}
template <class Src>
YART_HD f4 dnFilterPixelVar(const Src& src, uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t i, const DnConst& k) {
  return dnFilterPixel<true>(src, width, height, x, y, i, k);
}

// Finish pass of one pixel: re-modulate, alpha from the input frame
YART_HD f4 dnFinish(f4 c, const float* alb3, float alpha) {
  const f3 d = dnDivisor(alb3);
  return dnF4(c.x * d.x, c.y * d.y, c.z * d.z, alpha);
}

}  // namespace yart_hip
