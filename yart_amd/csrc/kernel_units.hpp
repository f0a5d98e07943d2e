// kernel_units.hpp — the interface between the translation units of libyart_hip.so. Units 1-4 (wavefront_units.hip) hold the path
// kernels and hand them out as type-erased host stubs; unit 0 (yart_hip.hip) picks them here and launches them. Included by
// both, so the compiler sees every declaration next to its definition. The argument of every kernel is the same WfArgs
// (wavefront_kernels.inc) in every unit.
#pragma once

namespace yart_hip { namespace tu {
typedef void (*AnyKernel)();
AnyKernel extendLean(int nodesForm, bool ident);      // unit 1: k_wf_extend_lean<MODE, NODES>
AnyKernel shadowLean(int nodesForm, bool ident);      // unit 2: k_wf_shadow_lean<MODE, NODES>
AnyKernel extendRetry(int nodesForm);                 // unit 3: k_wf_extend_retry_lean<NODES> ...
AnyKernel shadowRetry(int nodesForm);
AnyKernel extendFast(bool ident);
AnyKernel shadowFast(bool ident);
AnyKernel extendGeneral(bool retry);
AnyKernel shadowGeneral(bool retry);
AnyKernel shade(bool sort, bool fit, bool env1);      // unit 4: k_wf_shade<SORT, FIT, ENV1>
// (unit 0 alone holds the diagnostics of probes.inc, k_probe_rays<MODE> among them: the three walks of traverseScene it
// instantiates are copies of its own, so no path kernel's code or unit changes with it; likewise k_probe_shading, whose copies
// of bsdf.hpp / lights.hpp and of the shade kernel's LDS set-up are unit 0's own)
#if defined(YART_SHADE_REGIONS)
void shadeRegionsTake(unsigned long long* v48);       // (measurement builds: the shade kernel's region counters live in unit 4)
#endif
#if defined(YART_COUNT_TRAVERSAL)
// (instrumented build: every unit tallies the texel bytes of ITS kernels' lookups; unit 0 sums them)
void texTapReset1(); void texTapReset2(); void texTapReset3(); void texTapReset4();
unsigned long long texTapRead1(); unsigned long long texTapRead2(); unsigned long long texTapRead3(); unsigned long long texTapRead4();
#endif
}}  // namespace yart_hip::tu
