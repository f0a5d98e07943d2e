// plansim.cpp — TEST INFRASTRUCTURE for tests/test_plansim.py, never part of libyart_hip.so.
//
// csrc/render_host.hpp (the wave schedule and the buffer tables with their helpers) compiled alone as host C++, also under
// ASan + UBSan. Checks, and prints one line per group; exit status 0 only if all hold:
//   schedule   WaveSchedule over samples 1..70 x first, max in {1, 2, 3, 8, 64}: the waves sum to `samples` and follow the rule
//              of tile-renderer.hpp:121-124, 284-289, restated here wave by wave
//   check      checkAndCopyBuffers over both structs: caller structs cut short at every length (allocated at exactly that length, so
//              a read past struct_size is an ASan report), unknown mask bits, a null pointer behind every requested bit
//   layout     layOutBuffers / copyBuffers / clearBuffers: offsets, order and sizes for every mask
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../yart_amd/csrc/render_host.hpp"

using namespace yart_hip;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
  do {                                                                        \
    if (!(cond)) { failures++; std::fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
  } while (0)

static void testSchedule() {
  const uint32_t sizes[] = {1, 2, 3, 8, 64};
  size_t cases = 0;
  for (uint32_t samples = 1; samples <= 70; samples++)
    for (uint32_t first : sizes)
      for (uint32_t max : sizes) {
        WaveSchedule ws(samples, first, max);
        uint64_t sum = 0, prev = 0, n = 0;
        while (ws.next()) {
          CHECK(ws.wave == n, "%u %u %u: wave %llu", samples, first, max, (unsigned long long)ws.wave);
          CHECK(ws.takenBefore == sum && ws.takenAfter == sum + ws.samples, "%u %u %u: taken", samples, first, max);
          CHECK(ws.samples >= 1, "%u %u %u: an empty wave", samples, first, max);
          const uint64_t left = samples - sum;
          uint64_t want;
          if (n == 0) want = std::min<uint64_t>(first, samples);
          else if (n == 1 && prev == 1) want = 1;                                    // a lone first sample is followed by another single one
          else want = std::min<uint64_t>(std::min<uint64_t>(2 * prev, max), left);
          if (n == 1 && prev == 1) want = std::min<uint64_t>(want, left);
          CHECK(ws.samples == want, "%u %u %u: wave %llu has %llu samples, the rule gives %llu", samples, first, max,
                (unsigned long long)n, (unsigned long long)ws.samples, (unsigned long long)want);
          sum += ws.samples; prev = ws.samples; n++;
          if (n > 200) { CHECK(false, "%u %u %u: the schedule does not end", samples, first, max); break; }
        }
        CHECK(sum == samples, "%u %u %u: the waves sum to %llu", samples, first, max, (unsigned long long)sum);
        CHECK(!ws.next(), "%u %u %u: next() after the end", samples, first, max);
        cases++;
      }
  std::printf("schedule %zu cases\n", cases);
}

// what(): the message of the std::invalid_argument `f` throws, "" if it returns
template <class F>
static std::string thrown(F&& f) {
  try { f(); } catch (const std::invalid_argument& e) { return e.what(); }
  return "";
}

template <class S, size_t N>
static void testCheck(const BufferTable<S, N>& t) {
  static uint32_t target[4];                       // something non-null to point at
  size_t cases = 0;
  const std::string name = t.structName;
  for (uint32_t mask = 0; mask <= t.all; mask++) {
    S full{};
    full.mask = mask;
    for (const BufferField& f : t) setFieldPtr(full, f, target);
    // every length of the caller's struct, the object allocated at exactly that length
    for (size_t size = 0; size <= sizeof(S); size += 4) {
      full.struct_size = uint32_t(size);
      const size_t bytes = std::max<size_t>(size, 8);      // (the head itself is always there: struct_size says how far the rest goes)
      S* in = static_cast<S*>(std::malloc(bytes));
      std::memcpy(in, &full, bytes);
      S out{};
      const std::string msg = thrown([&] { checkAndCopyBuffers(t, *in, out); });
      std::string want;
      if (size < 8) want = name + ".struct_size is too small for the struct's head";
      else
        for (const BufferField& f : t)
          if ((mask & f.bit) && size < f.off + sizeof(void*)) { want = name + ".struct_size ends before a buffer the mask requests"; break; }
      CHECK(msg == want, "%s mask %u size %zu: \"%s\", expected \"%s\"", t.structName, mask, size, msg.c_str(), want.c_str());
      if (want.empty()) {
        CHECK(out.mask == mask && out.struct_size == sizeof(S), "%s mask %u size %zu: head of the copy", t.structName, mask, size);
        for (const BufferField& f : t)
          CHECK(fieldPtr(out, f) == ((mask & f.bit) ? static_cast<void*>(target) : nullptr), "%s mask %u size %zu: %s", t.structName, mask, size, f.name);
      }
      std::free(in);
      cases++;
    }
    // a null pointer behind each requested bit: the first one in table order is named
    full.struct_size = uint32_t(sizeof(S));
    for (const BufferField& f : t) {
      if (!(mask & f.bit)) continue;
      S in = full, out{};
      setFieldPtr(in, f, nullptr);
      const std::string msg = thrown([&] { checkAndCopyBuffers(t, in, out); });
      const std::string want = std::string(f.bitName) + " is requested and " + name + "." + f.name + " is null";
      CHECK(msg == want, "%s mask %u: \"%s\", expected \"%s\"", t.structName, mask, msg.c_str(), want.c_str());
      cases++;
    }
  }
  // unknown mask bits
  for (uint32_t bit = 0; bit < 32; bit++) {
    if (t.all & (1u << bit)) continue;
    S in{}, out{};
    in.struct_size = uint32_t(sizeof(S)); in.mask = 1u << bit;
    const std::string msg = thrown([&] { checkAndCopyBuffers(t, in, out); });
    CHECK(msg == name + ".mask has bits that are no " + t.bitFamily + " value", "%s bit %u: \"%s\"", t.structName, bit, msg.c_str());
    const std::string prefixed = thrown([&] { checkBufferHead(t, in, "temporal: "); });
    CHECK(prefixed == "temporal: " + msg, "%s bit %u: prefix", t.structName, bit);
    cases++;
  }
  std::printf("check %s %zu cases\n", t.structName, cases);
}

template <class S, size_t N>
static void testLayout(const BufferTable<S, N>& t) {
  const size_t pixels = 7;
  size_t cases = 0;
  for (uint32_t mask = 0; mask <= t.all; mask++) {
    S dev{}, host{};
    dev.mask = host.mask = mask;
    const size_t words = layOutBuffers(t, mask, pixels, nullptr, dev);
    size_t want = 0;
    for (const BufferField& f : t) if (mask & f.bit) want += f.words * pixels;
    CHECK(words == want, "%s mask %u: %zu words", t.structName, mask, words);
    for (const BufferField& f : t) CHECK(fieldPtr(dev, f) == nullptr, "%s mask %u: a pointer set without a base", t.structName, mask);
    std::vector<uint32_t> devMem(words + 1, 0x5a5a5a5au), hostMem(words + 1, 0u);
    CHECK(layOutBuffers(t, mask, pixels, devMem.data(), dev) == words, "%s mask %u: second pass", t.structName, mask);
    layOutBuffers(t, mask, pixels, hostMem.data(), host);
    size_t at = 0;
    for (const BufferField& f : t) {
      if (!(mask & f.bit)) { CHECK(fieldPtr(dev, f) == nullptr, "%s mask %u: %s not requested", t.structName, mask, f.name); continue; }
      CHECK(fieldPtr(dev, f) == devMem.data() + at, "%s mask %u: %s at %zu", t.structName, mask, f.name, at);
      at += f.words * pixels;
    }
    // clear: every requested buffer whole, with its byte, in table order; then copy back
    std::vector<uint32_t> order;
    clearBuffers(t, dev, pixels, [&](void* p, int byte, size_t bytes) { std::memset(p, byte, bytes); order.push_back(uint32_t(static_cast<uint32_t*>(p) - devMem.data())); });
    for (size_t i = 1; i < order.size(); i++) CHECK(order[i - 1] < order[i], "%s mask %u: clear order", t.structName, mask);
    at = 0;
    for (const BufferField& f : t) {
      if (!(mask & f.bit)) continue;
      for (size_t i = 0; i < f.words * pixels; i++)
        CHECK(devMem[at + i] == (f.clear ? 0xffffffffu : 0u), "%s mask %u: %s word %zu after clear", t.structName, mask, f.name, i);
      at += f.words * pixels;
    }
    CHECK(devMem[words] == 0x5a5a5a5au, "%s mask %u: clear ran past the end", t.structName, mask);
    size_t copied = 0;
    copyBuffers(t, host, dev, pixels, [&](void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); copied += bytes; });
    CHECK(copied == words * 4, "%s mask %u: %zu bytes copied", t.structName, mask, copied);
    CHECK(std::memcmp(hostMem.data(), devMem.data(), words * 4) == 0 && hostMem[words] == 0u, "%s mask %u: copy", t.structName, mask);
    cases++;
  }
  std::printf("layout %s %zu cases\n", t.structName, cases);
}

int main() {
  testSchedule();
  testCheck(kAovTable); testCheck(kMomentTable);
  testLayout(kAovTable); testLayout(kMomentTable);
  // the ids are the one buffer cleared to -1, and the per-pixel widths are the ABI's (include/yart_hip.h)
  CHECK(kAovTable.field(YART_AOV_IDS).clear == 0xff && kAovTable.field(YART_AOV_IDS).words == 4, "ids");
  CHECK(kAovTable.field(YART_AOV_DEPTH).words == 1 && kAovTable.field(YART_AOV_ALBEDO).words == 3, "widths");
  if (failures) { std::fprintf(stderr, "plansim: %d checks failed\n", failures); return 1; }
  std::printf("plansim ok\n");
  return 0;
}
