// wavefront_units.hip — units 1-4 of libyart_hip.so: the path kernels of the wavefront pipelines. Compiled four times
// (csrc/Makefile, -DYART_TU=1..4); the kernels are templates (wavefront_kernels.inc) and a unit emits those its pickers below
// name, so the four objects build in parallel and each kernel exists once:
//   1  the lean closest-hit kernels k_wf_extend_lean<MODE, NODES>          2  the lean any-hit kernels k_wf_shadow_lean<MODE, NODES>
//   3  the general kernels: retry (resumed walks), one-ray-per-lane lean and general forms        4  the shade kernel k_wf_shade<SORT, FIT, ENV1>
// Unit 0 (yart_hip.hip) holds everything else and launches these kernels through the pickers (kernel_units.hpp).
#if !defined(YART_TU) || YART_TU < 1 || YART_TU > 4
#error "wavefront_units.hip is compiled with -DYART_TU=1, 2, 3 or 4"
#endif
#include "hip_common.hpp"
#include "wavefront.hpp"
#include "trace_lean.hpp"
#include "kernel_units.hpp"

using namespace yart_hip;

namespace {
#include "wavefront_kernels.inc"
}  // namespace

// the kernels of this unit, for unit 0 (function pointers to the host stubs; the argument type is the same struct in every unit)
namespace yart_hip { namespace tu {
#define YART_ANY(K) reinterpret_cast<AnyKernel>(static_cast<void (*)(WfArgs)>(K))
#define YART_LEAN_FORM(KERNEL, M, N) (ident ? YART_ANY((KERNEL<(M) | TRAV_IDENTITY, N>)) : YART_ANY((KERNEL<(M), N>)))
#define YART_PICK_LEAN(KERNEL, M)                                                                        \
  (nodesForm == kNodesMaskLds ? YART_LEAN_FORM(KERNEL, M, kNodesMaskLds)                                 \
   : nodesForm == kNodesTlas ? YART_LEAN_FORM(KERNEL, M, kNodesTlas)                                     \
   : nodesForm == kNodesWalk ? YART_LEAN_FORM(KERNEL, M, kNodesWalk)                                     \
   : nodesForm == kNodesChunked ? YART_LEAN_FORM(KERNEL, M, kNodesChunked)                               \
                                : YART_LEAN_FORM(KERNEL, M, kNodesMask))
#define YART_PICK_RETRY(KERNEL)                                                                          \
  (nodesForm == kNodesMaskLds ? YART_ANY(KERNEL<kNodesMaskLds>) : nodesForm == kNodesTlas ? YART_ANY(KERNEL<kNodesTlas>)   \
   : nodesForm == kNodesWalk ? YART_ANY(KERNEL<kNodesWalk>) : nodesForm == kNodesChunked ? YART_ANY(KERNEL<kNodesChunked>) \
                                                                                         : YART_ANY(KERNEL<kNodesMask>))
#if YART_TU == 1
AnyKernel extendLean(int nodesForm, bool ident) { return YART_PICK_LEAN(k_wf_extend_lean, TRAV_FAST); }
#elif YART_TU == 2
AnyKernel shadowLean(int nodesForm, bool ident) { return YART_PICK_LEAN(k_wf_shadow_lean, TRAV_FAST); }
#elif YART_TU == 3
AnyKernel extendRetry(int nodesForm) { return YART_PICK_RETRY(k_wf_extend_retry_lean); }
AnyKernel shadowRetry(int nodesForm) { return YART_PICK_RETRY(k_wf_shadow_retry_lean); }
AnyKernel extendFast(bool ident) { return ident ? YART_ANY((k_wf_extend_fast<TRAV_FAST | TRAV_IDENTITY>)) : YART_ANY(k_wf_extend_fast<TRAV_FAST>); }
AnyKernel shadowFast(bool ident) { return ident ? YART_ANY((k_wf_shadow_fast<TRAV_FAST | TRAV_IDENTITY>)) : YART_ANY(k_wf_shadow_fast<TRAV_FAST>); }
AnyKernel extendGeneral(bool retry) { return retry ? YART_ANY(k_wf_extend<true>) : YART_ANY(k_wf_extend<false>); }
AnyKernel shadowGeneral(bool retry) { return retry ? YART_ANY(k_wf_shadow<true>) : YART_ANY(k_wf_shadow<false>); }
#elif YART_TU == 4
AnyKernel shade(bool sort, bool fit, bool env1) {
  return sort ? (env1 ? YART_ANY((k_wf_shade<true, true, true>)) : fit ? YART_ANY((k_wf_shade<true, true, false>)) : YART_ANY((k_wf_shade<true, false, false>)))
              : (env1 ? YART_ANY((k_wf_shade<false, true, true>)) : fit ? YART_ANY((k_wf_shade<false, true, false>)) : YART_ANY((k_wf_shade<false, false, false>)));
}
#if defined(YART_SHADE_REGIONS)
void shadeRegionsTake(unsigned long long* v48) {          // (measurement builds: the kernel's region counters live in this unit)
  (void)hipMemcpyFromSymbol(v48, HIP_SYMBOL(g_shadeRegion), 48 * sizeof(unsigned long long));
  const unsigned long long zero[48] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_shadeRegion), zero, sizeof(zero));
}
#endif
#endif
#undef YART_PICK_RETRY
#undef YART_PICK_LEAN
#undef YART_LEAN_FORM
#undef YART_ANY
#if defined(YART_COUNT_TRAVERSAL)
// (instrumented build: every unit tallies the texel bytes of ITS kernels' lookups; unit 0 sums them)
#define YART_CAT2(a, b) a##b
#define YART_CAT(a, b) YART_CAT2(a, b)
void YART_CAT(texTapReset, YART_TU)() { const unsigned long long zero = 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_texTapBytes), &zero, sizeof(zero)); }
unsigned long long YART_CAT(texTapRead, YART_TU)() { unsigned long long v = 0; (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_texTapBytes), sizeof(v)); return v; }
#endif
}}  // namespace yart_hip::tu
