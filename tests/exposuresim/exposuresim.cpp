// exposuresim — csrc/exposure.hpp compiled for the host (g++ -ffp-contract=off): the auto-exposure arithmetic the kernels run,
// on one thread. The tests compare it with yart_amd/exposure.py on bits, and run it under the sanitizers.
//
//   exposuresim IN OUT
// IN:  uint32 width, height, n_frames; int32 look; float ev_min, ev_max, trim_low, trim_high, key, compensation_ev, gain_ev_min,
//      gain_ev_max, speed_up, speed_down; uint32 x0, y0, x1, y1 (all 0: the whole frame);
//      then per frame: float dt; uint32 reset_before; width * height * 4 floats.
// OUT: per frame: 256 uint32 bins; cur_ev, target_ev, mean_ev, gain (float), n_counted, n_ignored, frames, flags, valid (uint32);
//      width * height * 4 floats (ldr); width * height * 3 bytes (rgb8).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../yart_amd/csrc/exposure.hpp"

using namespace yart_hip;

template <class T>
static void get(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "exposuresim: short input\n"); exit(2); }
}
template <class T>
static void put(FILE* f, const T* p, size_t n) {
  if (fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "exposuresim: short write\n"); exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: exposuresim IN OUT\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "exposuresim: cannot open a file\n"); return 2; }
  uint32_t head[3]; int32_t look; float p[10]; uint32_t win[4];
  get(in, head, 3); get(in, &look, 1); get(in, p, 10); get(in, win, 4);
  const uint32_t w = head[0], h = head[1], frames = head[2];
  uint32_t x0 = 0, y0 = 0, x1 = w, y1 = h;
  if (win[0] || win[1] || win[2] || win[3]) { x0 = win[0]; y0 = win[1]; x1 = win[2]; y1 = win[3]; }
  if (!(x0 < x1 && x1 <= w && y0 < y1 && y1 <= h)) { fprintf(stderr, "exposuresim: bad window\n"); return 2; }
  ExRecord rec = exNewRecord();
  const AgxLook lk = agxLook(look);
  std::vector<float> frame(size_t(w) * h * 4), ldr(size_t(w) * h * 4);
  std::vector<uint8_t> bytes(size_t(w) * h * 3);
  for (uint32_t k = 0; k < frames; k++) {
    float dt; uint32_t reset;
    get(in, &dt, 1); get(in, &reset, 1); get(in, frame.data(), frame.size());
    if (reset) rec = exNewRecord();
    const ExConst c = exConstants(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], dt);
    std::vector<uint32_t> hist(kExBins + 1u, 0u);
    for (uint32_t y = y0; y < y1; y++)
      for (uint32_t x = x0; x < x1; x++) {
        const float* v = &frame[(size_t(y) * w + x) * 4];
        hist[exBin(v[0], v[1], v[2], c)]++;
      }
    exResolve(rec, hist.data(), hist[kExBins], c);
    for (size_t i = 0; i < size_t(w) * h; i++) {
      f4 v; v.x = frame[4 * i]; v.y = frame[4 * i + 1]; v.z = frame[4 * i + 2]; v.w = frame[4 * i + 3];
      const f4 o = exApply(v, rec.gain, look, lk);
      ldr[4 * i] = o.x; ldr[4 * i + 1] = o.y; ldr[4 * i + 2] = o.z; ldr[4 * i + 3] = o.w;
      bytes[3 * i] = ppmByte(o.x); bytes[3 * i + 1] = ppmByte(o.y); bytes[3 * i + 2] = ppmByte(o.z);
    }
    put(out, hist.data(), kExBins);
    const float fs[4] = {rec.curEv, rec.targetEv, rec.meanEv, rec.gain};
    const uint32_t us[5] = {rec.nCounted, rec.nIgnored, rec.frames, rec.flags, rec.valid};
    put(out, fs, 4); put(out, us, 5);
    put(out, ldr.data(), ldr.size()); put(out, bytes.data(), bytes.size());
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  return 0;
}
