// hip_common.hpp — what every translation unit of libyart_hip.so starts from: the launch and traversal-stack constants the
// kernels and their launches share, and the host's error type, error check and device buffer.
// Included first by yart_hip.hip (unit 0) and by wavefront_units.hip (units 1-4). Everything is in the anonymous namespace, as
// the kernels are: each unit has its own copy and no symbol of it leaves the unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "traverse.hpp"

namespace {

constexpr int kBlock = 256;            // 4 waves per workgroup
#ifndef YART_STREAM_BLOCKS
#define YART_STREAM_BLOCKS 8           // workgroups per CU of the streaming kernels (generate, post, compact); shade + post stage at 1080p x 64 spp: 4 -> 105.5, 8 -> 106.1, 16 -> 106.4, 32 -> 106.6 ms
#endif
constexpr int kLdsStack = 24;          // traversal stack entries kept in LDS per lane (8 B each)
constexpr int kSpillDepth = int(yart_hip::kRefStackDepth) - kLdsStack;
constexpr int kSpillDepthMax = int(yart_hip::kRefStackDepth);   // spill area sized for the shallowest LDS stack
constexpr int kNumCounters = 32;       // [0] rays, [1..4] instrumented tallies, [8..31] debug statistics

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
#define HIP_CHECK(expr)                                                                     \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      throw HipError(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  void ensure(size_t count) {
    if (count <= n) return;
    release();
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
    n = count;
  }
  void upload(const std::vector<T>& v) {
    ensure(std::max<size_t>(v.size(), 1));
    if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
};

}  // namespace
