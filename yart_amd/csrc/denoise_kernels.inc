// denoise_kernels.inc — edge-avoiding à-trous filter (yart_hip_denoise_atrous_* and yart_hip_denoise_atrous_var_*), device side
// (included by postprocess.inc, unit 0, with the filter's host driver and entries). The arithmetic is denoise.hpp; the definition is the header comment
// of include/yart_hip.h. VAR chooses the form (denoise.hpp): false the plain filter, true the variance-guided one. Both forms have
// the same passes, tiles and 48 bytes per pixel: the variance travels in the fourth word of the working colour (where the plain
// filter keeps the valid flag), so a tap is two aligned 16-byte loads in either; the 3 x 3 Gaussian of the variance reads nine words
// that the 25 taps of step 1 read anyway.
//
//   k_dn_prepare<VAR>  one lane per pixel: frame, (variance,) albedo, normal, depth -> the 16-byte working colour and the 16-byte
//                      guide record {n.xyz, lz}, so that a tap of the filter is two aligned 16-byte loads.
//   k_dn_atrous<VAR, CLASS>
//                      one lane per pixel, 25 taps at distance step = 1 << i, read through the caches (no LDS tile; the
//                      LDS form of the small steps has not been built or measured, DESIGN §5). What CLASS chooses is the tile a
//                      workgroup of 256 lanes covers:
//                        0  steps 1 and 2: 16 x 16 pixels. The 25 taps of a tile fall into (16 + 4 step)^2 pixels — 1.6 / 2.3
//                           times the tile — so most of a tap's lines are in the CU's vector cache already; a wave covers four
//                           256-byte row segments per tap.
//                        1  steps of 4 and more: 64 x 4 pixels. No two taps of a tile share a line across rows, so a compact
//                           tile gains nothing; a wave covers one 1024-byte row segment per tap (eight whole 128-byte lines).
//   k_dn_finish        one lane per pixel: re-modulation by the divisor (formed again from the albedo buffer) and the input's alpha;
//                      it does not look at the fourth word, so both forms share it.
//
// Scratch: two working-colour images and the guide records, 48 bytes per pixel, allocated by the library per call.
// No kernel here uses LDS or scratch memory.

typedef float dn_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) dn_v4 dn_v4_global;
__device__ __forceinline__ f4 dnLd(const f4* p) {             // aligned 16-byte load, cached: neighbouring lanes' taps read it again
  const dn_v4 v = *(const dn_v4_global*) reinterpret_cast<const dn_v4*>(p);
  return dnF4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void dnSt(f4* p, f4 v) {
  dn_v4 q; q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
  *(dn_v4_global*) reinterpret_cast<dn_v4*>(p) = q;
}
struct DnDeviceSrc {
  const f4 *c, *g;
  __device__ __forceinline__ f4 colour(size_t q) const { return dnLd(c + q); }
  __device__ __forceinline__ f4 guide(size_t q) const { return dnLd(g + q); }
};

// the variance pointer exists in the variance-guided form's arguments only: the plain kernel is handed no pointer it does not use
struct DnNoVariance {};
struct DnVariance { const float* variance; };
template <bool VAR>
struct DnPrepareArgs : std::conditional_t<VAR, DnVariance, DnNoVariance> {
  const float *rgba, *albedo, *normal, *depth;     // albedo: only when the call demodulates; normal / depth: only when present
  f4 *colour, *guide;
  uint32_t n, pad;
};
template <bool VAR>
__global__ void __launch_bounds__(kBlock) k_dn_prepare(DnPrepareArgs<VAR> a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const float* in = a.rgba + size_t(p) * 4;
  float variance = 0.0f;
  if constexpr (VAR) variance = a.variance[p];
  f4 c, g;
  dnPrepare<VAR>(dnF4(in[0], in[1], in[2], in[3]), a.albedo ? a.albedo + size_t(p) * 3 : nullptr,
                 a.normal ? a.normal + size_t(p) * 3 : nullptr, a.depth ? a.depth + p : nullptr, c, g, variance);
  dnSt(a.colour + p, c);
  dnSt(a.guide + p, g);
}

struct DnAtrousArgs {
  const f4 *in, *guide;
  f4* out;
  uint32_t width, height, iteration, tilesX;
  DnConst k;
};
template <bool VAR, int STEP_CLASS>
__global__ void __launch_bounds__(kBlock) k_dn_atrous(DnAtrousArgs a) {
  constexpr uint32_t kTileW = STEP_CLASS == 0 ? 16u : 64u, kTileH = kBlock / kTileW;
  const uint32_t ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
  const uint32_t x = tx * kTileW + (threadIdx.x % kTileW), y = ty * kTileH + (threadIdx.x / kTileW);
  if (x >= a.width || y >= a.height) return;
  DnDeviceSrc src;
  src.c = a.in; src.g = a.guide;
  dnSt(a.out + (size_t(y) * a.width + x), dnFilterPixel<VAR>(src, a.width, a.height, x, y, a.iteration, a.k));
}

struct DnFinishArgs {
  const f4* colour;
  const float *rgba, *albedo;                      // albedo: only when the call demodulates
  float* out;                                      // may be rgba: a lane reads its own pixel's alpha before it writes the pixel
  uint32_t n, pad;
};
__global__ void __launch_bounds__(kBlock) k_dn_finish(DnFinishArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const float alpha = a.rgba[size_t(p) * 4 + 3];
  const f4 o = dnFinish(dnLd(a.colour + p), a.albedo ? a.albedo + size_t(p) * 3 : nullptr, alpha);
  float* q = a.out + size_t(p) * 4;
  q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = o.w;
}
