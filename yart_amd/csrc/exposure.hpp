// exposure.hpp — auto-exposure for frame sequences: the arithmetic of yart_hip_exposure_* (the DEFINITION in the header comment
// of include/yart_hip.h), stated once for the kernels (exposure_kernels.inc), the host entries (postprocess.inc) and the host
// statement of the tests (tests/exposuresim). Every operation is one individually rounded binary32 operation in the order
// written unless it says double; the build uses -ffp-contract=off. ylog2f (tonemap.hpp) and yexpf (ymath.hpp) have glibc's values
// on the device and on the host.
#pragma once
#include "tonemap.hpp"

namespace yart_hip {

constexpr uint32_t kExBins = 256u;                 // the histogram's bins: fixed
constexpr uint32_t kExFlagEmpty = 1u;              // YART_EXPOSURE_EMPTY

// what one meter call forms once on the host, in fp32, from YartExposureParams and dt
struct ExConst {
  float evMin, binsPerEv, binWidth, keyEv, compensationEv, gainEvMin, gainEvMax, aUp, aDown, trimLow, trimHigh;
};

// the handle's device record (40 bytes): YartExposureState's fields in its order, and valid
struct ExRecord {
  float curEv, targetEv, meanEv, gain;
  uint32_t nCounted, nIgnored, frames, flags;
  uint32_t valid, pad;
};

YART_HD ExRecord exNewRecord() {                   // a new handle, or one after reset: gain 1
  ExRecord r;
  r.curEv = 0.0f; r.targetEv = 0.0f; r.meanEv = 0.0f; r.gain = 1.0f;
  r.nCounted = 0u; r.nIgnored = 0u; r.frames = 0u; r.flags = 0u; r.valid = 0u; r.pad = 0u;
  return r;
}

inline ExConst exConstants(float evMin, float evMax, float trimLow, float trimHigh, float key, float compensationEv, float gainEvMin,
                           float gainEvMax, float speedUp, float speedDown, float dt) {
  ExConst k;
  k.evMin = evMin;
  k.binsPerEv = 256.0f / (evMax - evMin);
  k.binWidth = (evMax - evMin) / 256.0f;
  k.keyEv = ylog2f(key);
  k.compensationEv = compensationEv;
  k.gainEvMin = gainEvMin; k.gainEvMax = gainEvMax;
  k.aUp = 1.0f - expf(-(dt * speedUp));              // (host code: ymath.hpp's yexpf is libm's expf here)
  k.aDown = 1.0f - expf(-(dt * speedDown));
  k.trimLow = trimLow; k.trimHigh = trimHigh;
  return k;
}

YART_HD bool exFinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

// Meter, one pixel: its bin, or kExBins for a pixel that is ignored. Alpha is not read.
YART_HD uint32_t exBin(float r, float g, float b, const ExConst& k) {
  const float Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
  if (!(exFinite(r) && exFinite(g) && exFinite(b)) || !(Y > 0.0f)) return kExBins;
  const float ev = ylog2f(Y);
  const float t = (ev - k.evMin) * k.binsPerEv;
  return t < 0.0f ? 0u : (t >= 256.0f ? 255u : uint32_t(t));
}

// Resolve: the counted pixels' trim bounds [lo, hi) of N = sum(hist)
struct ExTrim { uint64_t lo, hi; };
YART_HD ExTrim exTrim(uint64_t N, const ExConst& k) {
  ExTrim t;
  t.lo = uint64_t(floor(double(k.trimLow) * double(N)));
  t.hi = N - uint64_t(floor(double(k.trimHigh) * double(N)));
  return t;
}
// bin b's term of S: c pixels lie below the bin, n in it
YART_HD double exTerm(uint32_t b, uint64_t c, uint64_t n, ExTrim t, const ExConst& k) {
  const uint64_t first = c > t.lo ? c : t.lo, last = c + n < t.hi ? c + n : t.hi;
  const uint64_t kb = last > first ? last - first : 0u;
  const float centre = k.evMin + (float(b) + 0.5f) * k.binWidth;
  return double(kb) * double(centre);
}
// the state step from S (the terms summed in ascending bin order, in double) and N; writes every field of the record
YART_HD void exStep(ExRecord& r, double S, uint64_t N, uint32_t nIgnored, ExTrim t, const ExConst& k) {
  r.nCounted = uint32_t(N); r.nIgnored = nIgnored;
  if (N == 0u) { r.flags = kExFlagEmpty; return; }
  r.flags = 0u;
  const float meanEv = float(S / double(t.hi - t.lo));
  const float want = (k.keyEv - meanEv) + k.compensationEv;
  const float target = ymin(k.gainEvMax, ymax(k.gainEvMin, want));
  if (!r.valid) {
    r.curEv = target; r.valid = 1u;
  } else {
    const float d = target - r.curEv;
    r.curEv = r.curEv + d * (d > 0.0f ? k.aUp : k.aDown);
  }
  r.meanEv = meanEv; r.targetEv = target;
  r.gain = yexpf(r.curEv * 0.6931472f);
  r.frames = r.frames + 1u;
}
// the whole resolve on one thread (host entries' checks, tests/exposuresim): hist is cleared by the caller
YART_HD void exResolve(ExRecord& r, const uint32_t* hist, uint32_t nIgnored, const ExConst& k) {
  uint64_t N = 0u;
  for (uint32_t b = 0; b < kExBins; b++) N += hist[b];
  const ExTrim t = exTrim(N, k);
  double S = 0.0;
  uint64_t c = 0u;
  for (uint32_t b = 0; b < kExBins; b++) { S += exTerm(b, c, hist[b], t, k); c += hist[b]; }
  exStep(r, S, N, nIgnored, t, k);
}

// Apply, one pixel: look 0 .. 2 through AgX (alpha 1), look -1 the product itself (alpha kept)
YART_HD f4 exApply(f4 v, float gain, int look, const AgxLook& lk) {
  const f3 c = mk3(v.x * gain, v.y * gain, v.z * gain);
  f4 o;
  if (look >= 0) {
    const f3 m = agxTonemap(c, lk);
    o.x = m.x; o.y = m.y; o.z = m.z; o.w = 1.0f;
  } else {
    o.x = c.x; o.y = c.y; o.z = c.z; o.w = v.w;
  }
  return o;
}

}  // namespace yart_hip
