// ptm_de_mfma_kernel.hpp -- differential evolution on the f64 matrix cores: the 32-D sweep of a big population whose proposal set
// is the reference sampler's default one (differential evolution from the chain's own saved history + Gaussians).
//
// The kernel is the GEN 1 / HIST / non-compacted build of mfma32_body (ptm_mfma_kernel.hpp) with DE = true: a tile's Gaussian
// chains go through both matrix products as they do in sweep_mfma32_kernel, and a chain whose picked member is differential
// evolution has its proposed state formed from two (or one) rows of its history instead -- see "DE" in the body.  Compiled in
// ptm_engine.hip, under a name of its own: the nine ptm_sweep_dp*.hip units and plan_sweep know nothing of it, the engine asks
// de_mfma_applies (ptm_sweep_plan.hpp) next to its plan.
#pragma once
#include <hip/hip_runtime.h>

#include "ptm_mfma_kernel.hpp"

namespace ptm {

#ifndef PTM_DE_MFMA_WAVES
#define PTM_DE_MFMA_WAVES 2   // waves per SIMD the register budget is cut for: the GEN 1 history build sits near its cap at 3, and this one
                              // adds the hand-over of a DE move (two row indices, a coefficient) and the rows it reads
#endif

// KIND: KIND_DENSE or KIND_LOWER (a diagonal factor is a Cholesky factor); EV: per-chain temperatures (evolving ladders)
template <int KIND, bool EV>
__global__ __launch_bounds__(256, PTM_DE_MFMA_WAVES) void de_mfma32_kernel(const Dev p) {
  mfma32_body<KIND, true, 1, EV, false, true>(p);
}

static inline const void* de_mfma32_kernel_of(int kind, bool ev) {
  if (kind == KIND_DENSE) return ev ? (const void*)de_mfma32_kernel<KIND_DENSE, true> : (const void*)de_mfma32_kernel<KIND_DENSE, false>;
  return ev ? (const void*)de_mfma32_kernel<KIND_LOWER, true> : (const void*)de_mfma32_kernel<KIND_LOWER, false>;
}

// one block per 256-chain tile of the launch's range (p.c_begin .. p.c_end, multiples of 64)
static inline hipError_t launch_de_mfma32(const Dev& p, int kind, bool ev, hipStream_t st) {
  const int chains = p.c_end - p.c_begin;
  const size_t lds = Mfma32Lds(nullptr, true, false, chains / p.W).bytes;
  void* args[] = {(void*)&p};
  return hipLaunchKernel(de_mfma32_kernel_of(kind, ev), dim3((chains + 255) / 256), dim3(256), args, lds, st);
}

// the kernel's name as rocprofv3 prints it
static inline int format_de_mfma_name(int kind, bool ev, char* b, size_t n) {
  return snprintf(b, n, "de_mfma32_kernel<%d, %s>", kind == KIND_DENSE ? KIND_DENSE : KIND_LOWER, ev ? "true" : "false");
}

}  // namespace ptm
