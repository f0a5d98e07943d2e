// temporal.hpp — temporal accumulation with camera reprojection (the temporal half of SVGF, Schied et al. 2017): the
// arithmetic of one pixel, as inline functions for the device kernel (temporal_kernels.inc) and for the host (tests/temporalsim).
//
// The definition is the comment above yart_hip_temporal_accumulate_device in include/yart_hip.h; this file states it operation by
// operation: every operation an individually rounded binary32 operation in the order written (the build has no FMA contraction).
// Only + - * /, floorf, sqrtf (correctly rounded; the clip alone), comparisons and integer min / max: no other libm.
//
// Per pixel the handle keeps three 16-byte records in each of two history images (96 bytes; the pass reads the neighbours of one
// image while it writes the other), each record kind in a plane of its own so that neighbouring lanes load neighbouring words:
//   rec0  {acc.r, acc.g, acc.b, variance}     the accumulated colour (demodulated when the flag is set) and its variance
//   rec1  {P.x, P.y, P.z, length (u32 bits)}  the world-space point; length 0: the record is nobody's tap
//   rec2  {n.x, n.y, n.z, node (u32 bits)}    the normal and ids[0]
// The moments form (yart_hip_temporal_accumulate_moments_*, SVGF's variance estimation) keeps a fourth plane, 128 bytes per pixel:
//   rec3  {m1, m2, w2, 0}                      the accumulated first and second moment of the luminance of the (demodulated)
//                                              colour and the sum of the squared frame weights of that estimate
// and runs a second pass, tpSpatialVariance, over the image the first one wrote: a pixel whose history is too short for the
// temporal estimate takes the variance of m1 over its 7 x 7 neighbourhood on the same surface.
#pragma once
#include <type_traits>
#include "denoise.hpp"
#include "scene_types.hpp"

namespace yart_hip {

// the previous frame's camera: makeCamera's derived quantities and what the projection forms from them once (host, fp32)
struct TpCamera {
  f3 position; float num;      // num = dot(topLeftPixel - position, nrm)
  f3 topLeft;  float dUU;      // dot(pixelDeltaU, pixelDeltaU)
  f3 dU;       float dVV;
  f3 dV;       float pad0;
  f3 nrm;      float pad1;     // cross(pixelDeltaU, pixelDeltaV)
};
inline TpCamera tpCamera(const CameraDev& cd) {
  TpCamera c{};
  c.position = cd.position; c.topLeft = cd.topLeftPixel; c.dU = cd.pixelDeltaU; c.dV = cd.pixelDeltaV;
  c.nrm = cross(c.dU, c.dV);
  c.num = dot(c.topLeft - c.position, c.nrm);
  c.dUU = dot(c.dU, c.dU);
  c.dVV = dot(c.dV, c.dV);
  return c;
}

struct TpConst {
  float alphaMin, normalCosMin, planeTolerance;
  uint32_t maxHistory;
  uint32_t width, height;
  uint32_t haveHistory;        // 0: first frame or after a reset: no tap is read
  uint32_t minMomentHistory;   // the moments form only: below this length a pixel is short
};

struct TpIn {                  // the current pixel
  f4 rgba;
  float variance, depth, coverage;
  uint32_t node;               // ids[0] as it lies in memory
  f3 P, n;
};
struct TpOut {
  f4 rgba;                     // to d_out_rgba
  float variance;              // to d_out_variance
  uint32_t length;             // to d_out_length
  f4 rec0, rec1, rec2;         // the pixel's new history record
  f4 rec3;                     // the moments form only
};

YART_HD bool tpFinite3(f3 a) { return dnFinite(a.x) && dnFinite(a.y) && dnFinite(a.z); }

// dnDivisor: d = alb > 1e-3f ? alb : 1.0f per channel
YART_HD f3 tpDivisor(bool demodulate, f3 alb) {
  return demodulate ? mk3(alb.x > 1e-3f ? alb.x : 1.0f, alb.y > 1e-3f ? alb.y : 1.0f, alb.z > 1e-3f ? alb.z : 1.0f) : mk3(1.0f);
}

// Per-node motion (yart_hip_temporal_set_motion): one record of six 16-byte words per scene node, the map from this frame's world
// space to the previous frame's for points rigidly attached to the node:
//   words 0 .. 2  {M row i}            the 3 x 4 point transform: P' = dot(M row i .xyz, P) + M row i .w
//   words 3 .. 5  {Nm row i, kind | 0} the 3 x 3 normal transform: n' = dot(Nm row i, n); kind (u32 bits, word 3 only) 0 static, 1 moving
// A Motion decides how a word is fetched: motion.nodes() and motion.word(node, i). A pixel is MOVING when its node is below
// nodes() and its record's kind is 1; it is projected, and its taps are validated, with P' and n'. Any other pixel runs the
// operations it ran before there was a motion: nothing is multiplied by an identity (-0 stays -0).
constexpr uint32_t kTpMotionWords = 6;           // 16-byte words per record
constexpr uint32_t kTpMotionMaxNodes = 1u << 20; // exclusive
struct TpNoMotion {                              // no motion is pending: compiles to the code without one
  static constexpr bool kNone = true;
  YART_HD uint32_t nodes() const { return 0u; }
  YART_HD f4 word(uint32_t, uint32_t) const { return dnF4(0.0f, 0.0f, 0.0f, 0.0f); }
};

// Per-pixel motion (yart_hip_temporal_set_pixel_motion): one record of two 16-byte words per pixel, {P'.xyz, kind} and {n'.xyz, 0},
// as yart_hip_scene_pixel_motion_* writes them (scene_motion.hpp). A Motion of this kind has kPixel and is made for ONE pixel:
// motion.word(i) fetches word i of that pixel's record. The pixel is MOVING when kind is 1.
template <class Motion, class = void> struct TpIsPixelMotion : std::false_type {};
template <class Motion> struct TpIsPixelMotion<Motion, std::void_t<decltype(Motion::kPixel)>> : std::true_type {};

// What a pixel is projected with and what its taps are tested with: P' and n' of a moving pixel, P and n of any other.
struct TpMoved { f3 P, n; bool finite; };
template <class Motion>
YART_HD TpMoved tpMoved(const Motion& motion, const TpIn& in) {
  if constexpr (TpIsPixelMotion<Motion>::value) {
    const f4 w0 = motion.word(0u);               // first: it carries kind
    if (dnBits(w0.w) == 1u) {
      const f4 w1 = motion.word(1u);
      TpMoved mv;
      mv.P = mk3(w0.x, w0.y, w0.z);
      mv.n = mk3(w1.x, w1.y, w1.z);
      mv.finite = tpFinite3(mv.P) && tpFinite3(mv.n);
      return mv;
    }
  } else if constexpr (!Motion::kNone) {
    if (in.node < motion.nodes()) {
      const f4 n0 = motion.word(in.node, 3u);    // first: it carries kind
      if (dnBits(n0.w) == 1u) {
        const f4 m0 = motion.word(in.node, 0u), m1 = motion.word(in.node, 1u), m2 = motion.word(in.node, 2u);
        const f4 n1 = motion.word(in.node, 4u), n2 = motion.word(in.node, 5u);
        TpMoved mv;
        mv.P = mk3(dot(mk3(m0.x, m0.y, m0.z), in.P) + m0.w, dot(mk3(m1.x, m1.y, m1.z), in.P) + m1.w,
                   dot(mk3(m2.x, m2.y, m2.z), in.P) + m2.w);
        mv.n = mk3(dot(mk3(n0.x, n0.y, n0.z), in.n), dot(mk3(n1.x, n1.y, n1.z), in.n), dot(mk3(n2.x, n2.y, n2.z), in.n));
        mv.finite = tpFinite3(mv.P) && tpFinite3(mv.n);
        return mv;
      }
    }
  }
  return TpMoved{in.P, in.n, true};
}

// The clip of the history to the frame's neighbourhood (yart_hip_temporal_set_clip; CLIP in the header's definition). A Frame
// decides how a neighbour of the pixel is fetched, and like a per-pixel Motion it is made for ONE pixel: frame.texel(dx, dy) is
// the texel of the pixel (x + dx, y + dy) — {c.r, c.g, c.b, counts}, c = rgb / d the neighbour's demodulated colour and counts
// (u32 bits) 1 when the neighbour counts, 0 when it does not or lies outside the image —; frame.radius() and frame.gamma() are
// the handle's setting. tpTexel forms a texel from a pixel's frame and albedo: the kernel forms each pixel's once per tile
// (temporal_kernels.inc), the host statement on every fetch; the operations, and so the bits, are the same.
struct TpNoFrame {                               // no clip is set: compiles to the code without one
  static constexpr bool kNone = true;
  YART_HD uint32_t radius() const { return 0u; }
  YART_HD float gamma() const { return 0.0f; }
  YART_HD f4 texel(int, int) const { return dnF4(0.0f, 0.0f, 0.0f, 0.0f); }
};
constexpr uint32_t kTpClipMaxRadius = 3;
YART_HD f4 tpTexel(bool demodulate, float r, float g, float b, f3 alb) {
  const f3 d = tpDivisor(demodulate, alb);
  const float cr = r / d.x, cg = g / d.y, cb = b / d.z;
  bool counts = dnFinite(cr) && dnFinite(cg) && dnFinite(cb);
  if (demodulate) counts = counts && tpFinite3(alb);
  return dnF4(cr, cg, cb, __builtin_bit_cast(float, counts ? 1u : 0u));
}
// value clipped to mu +- gamma * sd of the sums s1, s2 over kf neighbours; applied: mu, e2 and sd are finite (else value is returned)
YART_HD float tpClipTo(float value, float s1, float s2, float kf, float gamma, bool& applied) {
  const float mu = s1 / kf, e2 = s2 / kf;
  float var = e2 - mu * mu;
  var = var > 0.0f ? var : 0.0f;
  const float sd = sqrtf(var);
  const float lo = mu - gamma * sd, hi = mu + gamma * sd;
  applied = dnFinite(mu) && dnFinite(e2) && dnFinite(sd);
  if (!applied) return value;
  return value < lo ? lo : (value > hi ? hi : value);
}
// h (and h1, h2 with MOMENTS) of a pixel with a counting tap set, clipped
template <bool MOMENTS, class Frame>
YART_HD void tpClipHistory(const Frame& frame, float& hr, float& hg, float& hb, float& h1, float& h2) {
  const int r = int(frame.radius());
  const float gamma = frame.gamma();
  float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2r = 0.0f, s2g = 0.0f, s2b = 0.0f, sy1 = 0.0f, sy2 = 0.0f;
  uint32_t cnt = 0u;
  for (int dy = -r; dy <= r; dy++)
    for (int dx = -r; dx <= r; dx++) {
      const f4 t = frame.texel(dx, dy);
      if (dnBits(t.w) == 0u) continue;
      s1r = s1r + t.x; s1g = s1g + t.y; s1b = s1b + t.z;
      s2r = s2r + t.x * t.x; s2g = s2g + t.y * t.y; s2b = s2b + t.z * t.z;
      if constexpr (MOMENTS) {
        const float yq = dnLuma(t.x, t.y, t.z);
        sy1 = sy1 + yq; sy2 = sy2 + yq * yq;
      }
      cnt++;
    }
  if (cnt < 2u) return;
  const float kf = float(cnt);
  bool applied;
  hr = tpClipTo(hr, s1r, s2r, kf, gamma, applied);
  hg = tpClipTo(hg, s1g, s2g, kf, gamma, applied);
  hb = tpClipTo(hb, s1b, s2b, kf, gamma, applied);
  if constexpr (MOMENTS) {
    const float to = tpClipTo(h1, sy1, sy2, kf, gamma, applied);
    if (applied && to != h1) {                   // the history's luminance distribution is translated: h2 - h1^2 is kept
      h2 = h2 + (to * to - h1 * h1);
      h1 = to;
    }
  }
}

// One pixel. Hist decides how a 16-byte record of the previous history image is fetched: hist.rec0(q) / rec1(q) / rec2(q) (and
// rec3(q) with MOMENTS), q = y * width + x. demodulate: the call demodulates, and alb is the pixel's albedo (by value: no array
// for the kernel to keep). MOMENTS: the moments form — pass 1 of it; a short pixel's o.variance / rec0.w are provisional.
// Frame: TpNoFrame, or the pixel's neighbourhood in the frame when a clip is set.
template <bool MOMENTS, class Hist, class Motion, class Frame>
YART_HD TpOut tpAccumulatePixel(const Hist& hist, const Motion& motion, const Frame& frame, const TpConst& k, const TpCamera& cam,
                                const TpIn& in, bool demodulate, f3 alb) {
  TpOut o;
  const f3 d = tpDivisor(demodulate, alb);
  const float cr = in.rgba.x / d.x, cg = in.rgba.y / d.y, cb = in.rgba.z / d.z;
  const float ld = dnLuma(d.x, d.y, d.z);
  const float ld2 = ld * ld;
  const float v = in.variance / ld2;
  bool usable = dnFinite(cr) && dnFinite(cg) && dnFinite(cb) && dnFinite(in.variance) && in.variance >= 0.0f && dnFinite(v);
  if (demodulate) usable = usable && tpFinite3(alb);
  if (!usable) {               // passed through; an all-zero record of length 0
    o.rgba = in.rgba; o.variance = in.variance; o.length = 0u;
    o.rec0 = o.rec1 = o.rec2 = o.rec3 = dnF4(0.0f, 0.0f, 0.0f, 0.0f);
    return o;
  }
  const TpMoved mv = tpMoved(motion, in);
  const f3 P = mv.P, n = mv.n;
  const bool reprojectable = in.coverage == 1.0f && tpFinite3(in.P) && tpFinite3(in.n) && dnFinite(in.depth) && mv.finite;
  float accR = 0.0f, accG = 0.0f, accB = 0.0f, accV = 0.0f, wsum = 0.0f;
  float acc1 = 0.0f, acc2 = 0.0f, accW2 = 0.0f;           // MOMENTS: the tap-weighted sums of rec3's words
  uint32_t minLen = 0xffffffffu;
  bool any = false;
  if (k.haveHistory != 0u && reprojectable) {
    const f3 rel = P - cam.position;
    const float den = dot(rel, cam.nrm);
    const float s = cam.num / den;
    if (s > 0.0f && s <= 3.4028235e38f) {      // in front of the previous camera: den has num's sign and is not 0
      const f3 X = (cam.position + rel * s) - cam.topLeft;
      const float jx = dot(X, cam.dU) / cam.dUU, jy = dot(X, cam.dV) / cam.dVV;
      if (jx >= -1.0f && jx < float(k.width) && jy >= -1.0f && jy < float(k.height)) {   // else no tap is inside the image
        const float flx = floorf(jx), fly = floorf(jy);
        const int x0 = int(flx), y0 = int(fly);
        const float fx = jx - flx, fy = jy - fly;
        const float gx = 1.0f - fx, gy = 1.0f - fy;
        const float tol = k.planeTolerance * in.depth;
        for (int t = 0; t < 4; t++) {          // (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
          const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
          if (qx < 0 || qx >= int(k.width) || qy < 0 || qy >= int(k.height)) continue;
          const float w = ((t & 1) ? fx : gx) * ((t >> 1) ? fy : gy);
          if (!(w > 0.0f)) continue;
          const size_t q = size_t(qy) * k.width + size_t(qx);
          const f4 r1 = hist.rec1(q);
          const uint32_t len = dnBits(r1.w);
          if (len < 1u) continue;
          const f4 r2 = hist.rec2(q);
          if (dnBits(r2.w) != in.node) continue;
          if (!(dot(n, mk3(r2.x, r2.y, r2.z)) >= k.normalCosMin)) continue;
          const f3 dP = mk3(r1.x, r1.y, r1.z) - P;
          if (!(fabsf(dot(n, dP)) <= tol)) continue;
          const f4 r0 = hist.rec0(q);
          accR = accR + w * r0.x; accG = accG + w * r0.y; accB = accB + w * r0.z; accV = accV + w * r0.w;
          if constexpr (MOMENTS) {
            const f4 r3 = hist.rec3(q);
            acc1 = acc1 + w * r3.x; acc2 = acc2 + w * r3.y; accW2 = accW2 + w * r3.z;
          }
          wsum = wsum + w;
          minLen = len < minLen ? len : minLen;
          any = true;
        }
      }
    }
  }
  float outR = cr, outG = cg, outB = cb, outV = v;
  uint32_t N = 1u;
  const float y = MOMENTS ? dnLuma(cr, cg, cb) : 0.0f;
  float m1 = y, m2 = y * y, w2 = 1.0f;
  if (any) {
    float hr = accR / wsum, hg = accG / wsum, hb = accB / wsum;
    const float hv = accV / wsum;
    float h1 = 0.0f, h2 = 0.0f;
    if constexpr (!Frame::kNone) {             // the clip: after h (and h1, h2) is formed, before the blend
      if (MOMENTS) { h1 = acc1 / wsum; h2 = acc2 / wsum; }
      tpClipHistory<MOMENTS>(frame, hr, hg, hb, h1, h2);
    }
    N = minLen >= k.maxHistory ? k.maxHistory : minLen + 1u;
    const float inv = 1.0f / float(N);
    const float a = inv > k.alphaMin ? inv : k.alphaMin;
    const float b = 1.0f - a;
    outR = hr + a * (cr - hr); outG = hg + a * (cg - hg); outB = hb + a * (cb - hb);
    outV = (a * a) * v + (b * b) * hv;
    if (MOMENTS) {
      if constexpr (Frame::kNone) { h1 = acc1 / wsum; h2 = acc2 / wsum; }
      const float hw2 = accW2 / wsum;
      m1 = h1 + a * (y - h1);
      m2 = h2 + a * (y * y - h2);
      w2 = (a * a) * 1.0f + (b * b) * hw2;
    }
  }
  if (MOMENTS) {
    float vt = m2 - m1 * m1;
    vt = vt > 0.0f ? vt : 0.0f;
    if (N >= k.minMomentHistory && w2 < 1.0f) outV = vt * (w2 / (1.0f - w2));   // else short: the propagated value, for pass 2
    o.rec3 = dnF4(m1, m2, w2, 0.0f);
  }
  o.rgba = dnF4(outR * d.x, outG * d.y, outB * d.z, in.rgba.w);
  o.variance = outV * ld2;
  o.length = N;
  o.rec0 = dnF4(outR, outG, outB, outV);
  o.rec1 = dnF4(in.P.x, in.P.y, in.P.z, __builtin_bit_cast(float, N));
  o.rec2 = dnF4(in.n.x, in.n.y, in.n.z, __builtin_bit_cast(float, in.node));
  return o;
}

// without a clip, as the callers from before there was one name it
template <bool MOMENTS, class Hist, class Motion>
YART_HD TpOut tpAccumulatePixel(const Hist& hist, const Motion& motion, const TpConst& k, const TpCamera& cam, const TpIn& in,
                                bool demodulate, f3 alb) {
  return tpAccumulatePixel<MOMENTS, Hist, Motion, TpNoFrame>(hist, motion, TpNoFrame{}, k, cam, in, demodulate, alb);
}
// without a motion, as the callers from before there was one name it
template <bool MOMENTS, class Hist>
YART_HD TpOut tpAccumulatePixel(const Hist& hist, const TpConst& k, const TpCamera& cam, const TpIn& in, bool demodulate, f3 alb) {
  return tpAccumulatePixel<MOMENTS, Hist, TpNoMotion, TpNoFrame>(hist, TpNoMotion{}, TpNoFrame{}, k, cam, in, demodulate, alb);
}
// the plain form, as its callers have always named it
template <class Hist>
YART_HD TpOut tpAccumulatePixel(const Hist& hist, const TpConst& k, const TpCamera& cam, const TpIn& in, bool demodulate, f3 alb) {
  return tpAccumulatePixel<false, Hist, TpNoMotion, TpNoFrame>(hist, TpNoMotion{}, TpNoFrame{}, k, cam, in, demodulate, alb);
}

// Pass 2 of the moments form, one pixel (x, y) of the image pass 1 just wrote (hist: rec1 / rec2 / rec3 of that image); depth is
// the pixel's depth(p). True: the pixel is short and at least two pixels of its 7 x 7 window lie on its surface: vAcc is its
// spatial estimate, to be written to rec0.w and, times luma(d)^2, to out_variance. False: the pixel keeps what pass 1 wrote.
constexpr int kTpSpatialRadius = 3;
template <class Hist>
YART_HD bool tpSpatialVariance(const Hist& hist, const TpConst& k, uint32_t x, uint32_t y, float depth, float& vAcc) {
  const size_t p = size_t(y) * k.width + x;
  const f4 c1 = hist.rec1(p);
  const uint32_t N = dnBits(c1.w);
  if (N < 1u) return false;                      // not usable: passed through
  const f4 c3 = hist.rec3(p);
  if (N >= k.minMomentHistory && c3.z < 1.0f) return false;                      // long: the temporal estimate stands
  const f4 c2 = hist.rec2(p);
  const f3 P = mk3(c1.x, c1.y, c1.z), n = mk3(c2.x, c2.y, c2.z);
  const uint32_t node = dnBits(c2.w);
  const float tol = k.planeTolerance * depth;
  float s1 = 0.0f, s2 = 0.0f;
  uint32_t cnt = 0u;
  for (int dy = -kTpSpatialRadius; dy <= kTpSpatialRadius; dy++) {
    const int qy = int(y) + dy;
    if (qy < 0 || qy >= int(k.height)) continue;
    for (int dx = -kTpSpatialRadius; dx <= kTpSpatialRadius; dx++) {
      const int qx = int(x) + dx;
      if (qx < 0 || qx >= int(k.width)) continue;
      const size_t q = size_t(qy) * k.width + size_t(qx);
      const f4 r1 = hist.rec1(q);
      if (dnBits(r1.w) < 1u) continue;
      const f4 r2 = hist.rec2(q);
      if (dnBits(r2.w) != node) continue;
      if (!(dot(n, mk3(r2.x, r2.y, r2.z)) >= k.normalCosMin)) continue;
      const f3 dP = mk3(r1.x, r1.y, r1.z) - P;
      if (!(fabsf(dot(n, dP)) <= tol)) continue;
      const f4 r3 = hist.rec3(q);
      s1 = s1 + r3.x; s2 = s2 + r3.y;
      cnt++;
    }
  }
  if (cnt < 2u) return false;
  const float kf = float(cnt);
  const float e1 = s1 / kf, e2 = s2 / kf;
  float vs = e2 - e1 * e1;
  vs = vs > 0.0f ? vs : 0.0f;
  vAcc = (vs * (kf / float(cnt - 1u))) * c3.z;
  return true;
}

}  // namespace yart_hip
