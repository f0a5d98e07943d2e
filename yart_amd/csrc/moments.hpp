// moments.hpp — per-pixel sample moments (YART_MOMENT_*): the arithmetic, as inline functions for the device kernels
// (moment_kernels.inc) and for the host (tests/momentsim).
//
// The definition is the comment above yart_hip_render_moments in include/yart_hip.h; this file states it operation by operation.
// A pixel's samples arrive wave by wave, so the variance cannot be a two-pass one; the running sums are binary64 (a binary32
// S2 - S1 * S1 / N cancels on low-noise pixels), every operation individually rounded in the order written (no FMA contraction;
// the product y * y of two binary32 values is exact in binary64 either way).
#pragma once
#include "estimator.hpp"

namespace yart_hip {

// Running state of one pixel of the rank: 44 bytes, padded to 48 (16-byte aligned records).
struct MomentState {
  double sr, sg, sb;           // sums of the accepted samples' w = L.xyz * exposureScale, per channel
  double s1, s2;               // sums of y = luma(w) and of y * y
  uint32_t n, pad;             // accepted samples
};
static_assert(sizeof(MomentState) == 48, "MomentState is 48 bytes per pixel");

struct MomentSample {
  f3 w;
  float y;
  bool ok;
};

// One sample: w as k_gmon_blend forms it, its luminance, and whether it counts: no component of w NaN or negative, y finite.
// The rule is fixed (it does not follow YartRenderParams.estimator).
YART_HD MomentSample momentSample(f3 radiance, float exposureScale) {
  MomentSample m;
  m.w = radiance * exposureScale;
  m.y = luma(m.w);
  const bool finiteY = (__builtin_bit_cast(uint32_t, m.y) & 0x7f800000u) != 0x7f800000u;
  // (a comparison with a NaN is false: !(c >= 0) refuses NaN and negative components alike; -0.0f is not negative)
  m.ok = m.w.x >= 0.0f && m.w.y >= 0.0f && m.w.z >= 0.0f && finiteY;
  return m;
}

YART_HD void momentAdd(MomentState& st, float wr, float wg, float wb, float y) {
  const double yd = double(y);
  st.sr = st.sr + double(wr); st.sg = st.sg + double(wg); st.sb = st.sb + double(wb);
  st.s1 = st.s1 + yd;
  st.s2 = st.s2 + yd * yd;
  st.n++;
}

// After the last wave: mean (3 floats), variance of the mean luminance estimate, count.
YART_HD void momentFinish(const MomentState& st, float mean[3], float& variance, uint32_t& count) {
  count = st.n;
  if (st.n == 0u) { mean[0] = mean[1] = mean[2] = 0.0f; variance = 0.0f; return; }
  const double n = double(st.n);
  mean[0] = float(st.sr / n); mean[1] = float(st.sg / n); mean[2] = float(st.sb / n);
  variance = 0.0f;
  if (st.n >= 2u) {
    const double v = ((st.s2 - (st.s1 * st.s1) / n) / (n - 1.0)) / n;
    variance = v < 0.0 ? 0.0f : float(v);
  }
}

}  // namespace yart_hip
