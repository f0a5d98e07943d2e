// render_host.hpp — host-only pieces of a render that more than one entry point needs: the wave schedule, and one table per
// caller-facing buffer struct (YartAovBuffers, YartMomentBuffers) with the helpers that walk it. Plain C++, no HIP: yart_hip.hip
// and multi_device.inc use it, and tests/plansim compiles it alone (also under ASan + UBSan).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/yart_hip.h"

namespace yart_hip {

// The wave schedule of tile-renderer.hpp:121-124, 264-289: w0 = min(first, samples), then min(2 w, max), capped by what is left —
// a first wave of one sample is followed by another single one. next() steps to the following wave (false: none is left);
// wave / samples / takenBefore / takenAfter describe the wave it stepped to.
struct WaveSchedule {
  uint64_t wave = 0, samples = 0, takenBefore = 0, takenAfter = 0;
  WaveSchedule(uint32_t totalSamples, uint32_t firstWaveSamples, uint32_t maxWaveSamples)
      : total_(totalSamples), max_(maxWaveSamples), upcoming_(std::min(firstWaveSamples, totalSamples)) {}
  bool next() {
    if (upcoming_ == 0) return false;
    wave = takenAfter == 0 ? 0 : wave + 1;
    const uint64_t waveSamples = upcoming_;
    samples = waveSamples; takenBefore = takenAfter; takenAfter += waveSamples;
    const uint64_t grown = (wave > 0 || waveSamples > 1) ? std::min<uint64_t>(waveSamples * 2, max_) : 1;
    upcoming_ = std::min(grown, total_ - takenAfter);
    return true;
  }

 private:
  uint64_t total_, max_, upcoming_;
};

// One buffer of a YartAovBuffers / YartMomentBuffers: its mask bit, where its pointer sits in the struct, 4-byte words per pixel,
// the byte an untouched pixel is cleared to (0x00; 0xff = -1 for ids) and the names the error messages are formed from.
struct BufferField { uint32_t bit; size_t off; uint32_t words; int clear; const char* bitName; const char* name; };
template <class S, size_t N>
struct BufferTable {
  const char* structName;      // "YartAovBuffers"
  const char* bitFamily;       // "YART_AOV_*"
  uint32_t all;                // every defined mask bit
  BufferField fields[N];       // in the order of the host staging layout
  const BufferField* begin() const { return fields; }
  const BufferField* end() const { return fields + N; }
  const BufferField& field(uint32_t bit) const {
    for (const BufferField& f : fields) if (f.bit == bit) return f;
    throw std::logic_error("BufferTable: no such bit");
  }
};
constexpr BufferTable<YartAovBuffers, 7> kAovTable = {"YartAovBuffers", "YART_AOV_*", YART_AOV_ALL, {
    {YART_AOV_ALBEDO, offsetof(YartAovBuffers, albedo), 3, 0x00, "YART_AOV_ALBEDO", "albedo"},
    {YART_AOV_NORMAL, offsetof(YartAovBuffers, normal), 3, 0x00, "YART_AOV_NORMAL", "normal"},
    {YART_AOV_POSITION, offsetof(YartAovBuffers, position), 3, 0x00, "YART_AOV_POSITION", "position"},
    {YART_AOV_DEPTH, offsetof(YartAovBuffers, depth), 1, 0x00, "YART_AOV_DEPTH", "depth"},
    {YART_AOV_COVERAGE, offsetof(YartAovBuffers, coverage), 1, 0x00, "YART_AOV_COVERAGE", "coverage"},
    {YART_AOV_IDS, offsetof(YartAovBuffers, ids), 4, 0xff, "YART_AOV_IDS", "ids"},
    {YART_AOV_RAYS, offsetof(YartAovBuffers, rays), 1, 0x00, "YART_AOV_RAYS", "rays"}}};
constexpr BufferTable<YartMomentBuffers, 3> kMomentTable = {"YartMomentBuffers", "YART_MOMENT_*", YART_MOMENT_ALL, {
    {YART_MOMENT_MEAN, offsetof(YartMomentBuffers, mean), 3, 0x00, "YART_MOMENT_MEAN", "mean"},
    {YART_MOMENT_VARIANCE, offsetof(YartMomentBuffers, variance), 1, 0x00, "YART_MOMENT_VARIANCE", "variance"},
    {YART_MOMENT_COUNT, offsetof(YartMomentBuffers, count), 1, 0x00, "YART_MOMENT_COUNT", "count"}}};

template <class S> void* fieldPtr(const S& s, const BufferField& f) {
  return *reinterpret_cast<void* const*>(reinterpret_cast<const char*>(&s) + f.off);
}
template <class S> void setFieldPtr(S& s, const BufferField& f, void* p) {
  *reinterpret_cast<void**>(reinterpret_cast<char*>(&s) + f.off) = p;
}

// --- check and copy -------------------------------------------------------------------------------------------------------
// A caller's struct may be shorter than this build's (struct_size): nothing past in.struct_size is read.
// The head: struct_size covers struct_size and mask, and the mask has no unknown bit (`prefix` goes in front of the message)
template <class S, size_t N>
void checkBufferHead(const BufferTable<S, N>& t, const S& in, const char* prefix = "") {
  if (in.struct_size < 2 * sizeof(uint32_t)) throw std::invalid_argument(std::string(prefix) + t.structName + ".struct_size is too small for the struct's head");
  if ((in.mask & ~t.all) != 0u) throw std::invalid_argument(std::string(prefix) + t.structName + ".mask has bits that are no " + t.bitFamily + " value");
}
// One field: its pointer copied from `in` to `out` if the mask requests it, the struct reaches it and it is not null — else false
template <class S>
bool takeBufferField(const S& in, const BufferField& f, S& out) {
  if (!(in.mask & f.bit) || in.struct_size < f.off + sizeof(void*)) return false;
  void* p = fieldPtr(in, f);
  if (p == nullptr) return false;
  setFieldPtr(out, f, p);
  return true;
}
// The whole struct, into one of this build's size: every requested buffer must be inside the caller's struct and non-null
template <class S, size_t N>
void checkAndCopyBuffers(const BufferTable<S, N>& t, const S& in, S& out) {
  checkBufferHead(t, in);
  for (const BufferField& f : t) {
    if (!(in.mask & f.bit)) continue;
    if (in.struct_size < f.off + sizeof(void*)) throw std::invalid_argument(std::string(t.structName) + ".struct_size ends before a buffer the mask requests");
    if (!takeBufferField(in, f, out))
      throw std::invalid_argument(std::string(f.bitName) + " is requested and " + t.structName + "." + f.name + " is null");
  }
  out.struct_size = uint32_t(sizeof(S)); out.mask = in.mask;
}

// --- lay out in one allocation, copy back ------------------------------------------------------------------------------
// The requested buffers side by side, in table order, as 4-byte words: returns the words they take; with `base` set, `dev`'s
// pointers are pointed into it
template <class S, size_t N>
size_t layOutBuffers(const BufferTable<S, N>& t, uint32_t mask, size_t pixels, uint32_t* base, S& dev) {
  size_t at = 0;
  for (const BufferField& f : t) {
    if (!(mask & f.bit)) continue;
    if (base) setFieldPtr(dev, f, base + at);
    at += f.words * pixels;
  }
  return at;
}
// copy(to.field, from.field, bytes) for every requested buffer, in table order
template <class S, size_t N, class Copy>
void copyBuffers(const BufferTable<S, N>& t, const S& to, const S& from, size_t pixels, Copy copy) {
  for (const BufferField& f : t)
    if (to.mask & f.bit) copy(fieldPtr(to, f), fieldPtr(from, f), size_t(f.words) * pixels * 4);
}

// --- clear ----------------------------------------------------------------------------------------------------------------
// set(buffer, byte, bytes) for every requested buffer, in table order
template <class S, size_t N, class Set>
void clearBuffers(const BufferTable<S, N>& t, const S& bufs, size_t pixels, Set set) {
  for (const BufferField& f : t)
    if (bufs.mask & f.bit) set(fieldPtr(bufs, f), f.clear, size_t(f.words) * pixels * 4);
}

}  // namespace yart_hip
