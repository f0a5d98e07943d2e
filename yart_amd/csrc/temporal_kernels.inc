// temporal_kernels.inc — temporal accumulation with camera reprojection (yart_hip_temporal_*), device side (included by
// postprocess.inc, unit 0, after denoise_kernels.inc whose 16-byte load / store it uses). The arithmetic is temporal.hpp; the
// definition is the header comment of include/yart_hip.h.
//
//   k_tp_accumulate   one lane per pixel in the 16 x 16 tile of k_dn_atrous<0>: reads the pixel's frame, variance and feature
//                     buffers (64 bytes with albedo), projects its surface point into the previous camera, reads up to four taps
//                     of the previous history image — three aligned 16-byte loads each, the colour record only for a tap that
//                     counts —, blends, writes the pixel's record into the other history image (48 bytes) and the caller's
//                     outputs (24 bytes). For any smooth camera move the taps of a tile fall into a tile-sized neighbourhood of
//                     the previous image, so neighbouring lanes' taps share lines in the CU's vector cache: no LDS tile.
//                     A first frame (or the first after a reset) reads no tap: TpConst::haveHistory is uniform over the launch.
//
//   k_tp_accumulate<·, true>   with a pending per-node motion (yart_hip_temporal_set_motion): a lane whose node has a record loads
//                     the record's word 3, which carries kind, and the other five 16-byte words only when the node moves — six
//                     aligned loads; a tile's lanes mostly share a node, so all but the first are line hits. Launched only for
//                     the call that consumes a motion: the <·, false> kernels are the code from before there was one.
//
//   k_tp_accumulate<·, true, true>   with pending per-pixel records (yart_hip_temporal_set_pixel_motion): a lane loads the first
//                     word of its pixel's record, which carries kind, and the second only when the pixel moved — two aligned,
//                     coalesced 16-byte loads (32 bytes per pixel). Launched only for the call that consumes the records.
//
//   k_tp_accumulate<true>   the moments form, pass 1: the same, with rec3 — one more aligned 16-byte load per counting tap and
//                     one more 16-byte store.
//   k_tp_spatial_variance   the moments form, pass 2, launched after pass 1 on the image it wrote, same tile: a lane whose pixel
//                     is long (or not usable) returns after two loads of its own records, so a wave without a short pixel ends
//                     before its first tap load. A short pixel walks its 7 x 7 window through the caches — rec1, then rec2, and
//                     rec3 only for a tap that counts; a tile's taps fall into 22 x 22 pixels, 1.9 times the tile, the regime
//                     of k_dn_atrous<·, 0>: no LDS tile — and writes its own rec0.w and out_variance, nothing a neighbour reads.
//
//   k_tp_accumulate<·, ·, ·, true>   with a clip set on the handle (yart_hip_temporal_set_clip): the workgroup first forms the texel
//                     {c.rgb, counts} of every pixel of its tile and a halo of `radius` around it — at most 22 x 22 — ONCE, into
//                     LDS: all 256 lanes take part, those outside the image included, before any returns; image edges are bounds
//                     checked and a texel outside the image does not count. After the barrier a lane with a counting tap set sums
//                     its (2 radius + 1)^2 window from LDS in the defined order, one 16-byte LDS read per neighbour, where it
//                     would otherwise issue 3 IEEE divides and load 28 bytes per neighbour. Chosen over a pre-pass that writes
//                     mu and sd per pixel, which was not built: a second launch and 24 - 32 bytes per pixel written and read
//                     back, where the tile adds no memory traffic beyond the halo (profiles/temporal_clip.txt has the times).
//                     Launched only while a clip is set: the <·, ·, ·, false> kernels are the code from before there was one
//                     (profiles/temporal_clip_resources.txt).
//
// History: two images of three (the moments form: four) planes of 16-byte records (temporal.hpp), 96 (128) bytes per pixel, owned
// by the YartTemporal handle. The CLIP kernels use 11 KB of LDS (below); no other kernel here uses LDS, and none uses scratch
// memory; none of the existing kernels changes.

struct TpDeviceHist {
  const f4 *r0, *r1, *r2, *r3;                     // r3: the moments form only
  __device__ __forceinline__ f4 rec0(size_t q) const { return dnLd(r0 + q); }
  __device__ __forceinline__ f4 rec1(size_t q) const { return dnLd(r1 + q); }
  __device__ __forceinline__ f4 rec2(size_t q) const { return dnLd(r2 + q); }
  __device__ __forceinline__ f4 rec3(size_t q) const { return dnLd(r3 + q); }
};

struct TpDeviceMotion {
  static constexpr bool kNone = false;
  const f4* rec;                                   // kTpMotionWords words per node
  uint32_t n;
  __device__ __forceinline__ uint32_t nodes() const { return n; }
  __device__ __forceinline__ f4 word(uint32_t node, uint32_t i) const { return dnLd(rec + size_t(node) * kTpMotionWords + i); }
};

struct TpArgs {
  const float *rgba, *variance, *albedo;           // albedo: only when the call demodulates
  const float *position, *normal, *depth, *coverage;
  const int32_t* ids;                              // 4 per pixel; [0] = node
  const f4* histIn;                                // planes rec0 | rec1 | rec2 (| rec3), n records each
  f4* histOut;
  float *outRgba, *outVariance;                    // outRgba may be rgba, outVariance may be variance: a lane reads its own
  uint32_t* outLength;                             // pixel before it writes it; outVariance / outLength may be null
  uint32_t n, tilesX;
  TpConst k;
  TpCamera cam;
  uint32_t clipRadius;                             // the CLIP kernels only: the handle's setting
  float clipGamma;
};
// per-pixel records (yart_hip_temporal_set_pixel_motion): the launch's argument, and what a lane makes of it for its pixel
struct TpDevicePixelMotion {
  static constexpr bool kNone = false, kPixel = true;
  const f4* rec;                                   // the pixel's two words
  __device__ __forceinline__ f4 word(uint32_t i) const { return dnLd(rec + i); }
};
struct TpDevicePixelRecords { const f4* rec; };    // two words per pixel

// MOTION: the launch has a motion, `motion` — per-node records, or with PIXEL per-pixel ones; else the second argument is empty and
// the code is that of a kernel without a motion
template <bool MOTION, bool PIXEL>
using TpMotionArg = typename std::conditional<PIXEL, TpDevicePixelRecords,
                                              typename std::conditional<MOTION, TpDeviceMotion, TpNoMotion>::type>::type;
template <bool MOTION, bool PIXEL>
__device__ __forceinline__ auto tpMotionOf(const TpMotionArg<MOTION, PIXEL>& motion, size_t p) {
  if constexpr (PIXEL) return TpDevicePixelMotion{motion.rec + p * 2u};
  else return motion;
}
// The clip's tile: the texels (temporal.hpp tpTexel) of the workgroup's 16 x 16 pixels and a halo of `radius` around them, at most
// 22 rows, in LDS. A row is kTpTilePitch = 32 texels = 512 bytes, two bank rows: the lanes of a wave read 4 rows x 16 consecutive
// texels with one 16-byte LDS read, whose four 16-lane groups each take 8 lanes of one row and 4 + 4 of the next — at a pitch that
// is a multiple of 16 texels the 16 lanes of a group fall on 16 different 16-byte slots, whatever the window offset (a pitch of 22
// puts 8 of them on slots another 8 use: measured at 1920 x 1080 and radius 3, + 0.016 ms on a call of 0.164 ms, a third again
// of the clip's cost; profiles/temporal_clip.txt).
constexpr uint32_t kTpTilePitch = 32u;
constexpr uint32_t kTpTileRows = 16u + 2u * kTpClipMaxRadius;
struct TpDeviceFrame {
  static constexpr bool kNone = false;
  const f4* at;                                    // the pixel's own texel in the tile
  uint32_t r;
  float g;
  __device__ __forceinline__ uint32_t radius() const { return r; }
  __device__ __forceinline__ float gamma() const { return g; }
  __device__ __forceinline__ f4 texel(int dx, int dy) const { return at[dy * int(kTpTilePitch) + dx]; }
};

template <bool CLIP>
__device__ __forceinline__ auto tpFrameOf(const f4* own, const TpArgs& a) {
  if constexpr (CLIP) return TpDeviceFrame{own, a.clipRadius, a.clipGamma};
  else return TpNoFrame{};
}

template <bool MOMENTS, bool MOTION, bool PIXEL = false, bool CLIP = false>
__global__ void __launch_bounds__(kBlock) k_tp_accumulate(TpArgs a, TpMotionArg<MOTION, PIXEL> motion) {
  static_assert(MOTION || !PIXEL, "per-pixel records are a motion");
  const uint32_t ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
  const uint32_t x = tx * 16u + (threadIdx.x % 16u), y = ty * 16u + (threadIdx.x / 16u);
  [[maybe_unused]] const f4* own = nullptr;
  if constexpr (CLIP) {                            // every lane of the workgroup, those outside the image included, before any returns
    __shared__ f4 tile[kTpTileRows * kTpTilePitch];
    const int r = int(a.clipRadius), side = 16 + 2 * r;
    const int x0 = int(tx * 16u) - r, y0 = int(ty * 16u) - r;
    for (int i = int(threadIdx.x); i < side * side; i += int(kBlock)) {
      const int ly = i / side, lx = i - ly * side;
      const int qx = x0 + lx, qy = y0 + ly;
      f4 t = dnF4(0.0f, 0.0f, 0.0f, 0.0f);         // outside the image: does not count
      if (qx >= 0 && qx < int(a.k.width) && qy >= 0 && qy < int(a.k.height)) {
        const size_t q = size_t(qy) * a.k.width + size_t(qx);
        f3 alb = mk3(1.0f);
        if (a.albedo) alb = mk3(a.albedo[q * 3], a.albedo[q * 3 + 1], a.albedo[q * 3 + 2]);
        t = tpTexel(a.albedo != nullptr, a.rgba[q * 4], a.rgba[q * 4 + 1], a.rgba[q * 4 + 2], alb);
      }
      tile[uint32_t(ly) * kTpTilePitch + uint32_t(lx)] = t;
    }
    __syncthreads();
    own = tile + (threadIdx.x / 16u + uint32_t(r)) * kTpTilePitch + (threadIdx.x % 16u + uint32_t(r));
  }
  if (x >= a.k.width || y >= a.k.height) return;
  const size_t p = size_t(y) * a.k.width + x;
  TpIn in;
  in.rgba = dnF4(a.rgba[p * 4], a.rgba[p * 4 + 1], a.rgba[p * 4 + 2], a.rgba[p * 4 + 3]);
  in.variance = a.variance[p];
  in.depth = a.depth[p];
  in.coverage = a.coverage[p];
  in.node = uint32_t(a.ids[p * 4]);
  in.P = mk3(a.position[p * 3], a.position[p * 3 + 1], a.position[p * 3 + 2]);
  in.n = mk3(a.normal[p * 3], a.normal[p * 3 + 1], a.normal[p * 3 + 2]);
  f3 alb = mk3(1.0f);
  if (a.albedo) alb = mk3(a.albedo[p * 3], a.albedo[p * 3 + 1], a.albedo[p * 3 + 2]);
  TpDeviceHist hist;
  hist.r0 = a.histIn; hist.r1 = a.histIn + a.n; hist.r2 = a.histIn + size_t(a.n) * 2;
  hist.r3 = MOMENTS ? a.histIn + size_t(a.n) * 3 : nullptr;
  const TpOut o = tpAccumulatePixel<MOMENTS>(hist, tpMotionOf<MOTION, PIXEL>(motion, p), tpFrameOf<CLIP>(own, a), a.k, a.cam, in,
                                             a.albedo != nullptr, alb);
  dnSt(a.histOut + p, o.rec0);
  dnSt(a.histOut + a.n + p, o.rec1);
  dnSt(a.histOut + size_t(a.n) * 2 + p, o.rec2);
  if (MOMENTS) dnSt(a.histOut + size_t(a.n) * 3 + p, o.rec3);
  float* q = a.outRgba + p * 4;                    // the caller's buffers are only known to be 4-byte aligned
  q[0] = o.rgba.x; q[1] = o.rgba.y; q[2] = o.rgba.z; q[3] = o.rgba.w;
  if (a.outVariance) a.outVariance[p] = o.variance;
  if (a.outLength) a.outLength[p] = o.length;
}

// a: the arguments of the k_tp_accumulate<true, ·> launch it follows; reads a.depth and a.albedo of its own pixel and a.histOut
__global__ void __launch_bounds__(kBlock) k_tp_spatial_variance(TpArgs a) {
  const uint32_t ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
  const uint32_t x = tx * 16u + (threadIdx.x % 16u), y = ty * 16u + (threadIdx.x / 16u);
  if (x >= a.k.width || y >= a.k.height) return;
  const size_t p = size_t(y) * a.k.width + x;
  TpDeviceHist hist;
  hist.r0 = a.histOut; hist.r1 = a.histOut + a.n; hist.r2 = a.histOut + size_t(a.n) * 2; hist.r3 = a.histOut + size_t(a.n) * 3;
  float vAcc;
  if (!tpSpatialVariance(hist, a.k, x, y, a.depth[p], vAcc)) return;
  reinterpret_cast<float*>(a.histOut + p)[3] = vAcc;           // rec0.w
  if (a.outVariance) {
    f3 alb = mk3(1.0f);
    if (a.albedo) alb = mk3(a.albedo[p * 3], a.albedo[p * 3 + 1], a.albedo[p * 3 + 2]);
    const f3 d = tpDivisor(a.albedo != nullptr, alb);
    const float ld = dnLuma(d.x, d.y, d.z);
    a.outVariance[p] = vAcc * (ld * ld);
  }
}
