// ptm_devprior_kernels.hpp -- the device-prior plug-in (ptm_set_prior_device): the reference's prior gate as ONE function for the host
// path and the device path, and the kernels behind the user's batched log-prior.
//
// A step on that path is  exchange kernel -> propose pass (mode 1) -> count + pack of the VALID proposals (gate bit 1; the count and
// pack kernels of ptm_devlike_kernels.hpp with mask (1, 1), into the prior's own batch) -> the user's prior work -> devprior_gate_kernel
// -> count + pack of the WANTED proposals (gate bit 2) -> the user's likelihood work -> scatter (+ best) -> accept pass (mode 2), all
// queued on the engine's stream: no host wait.  Three engine kernels more per step than the device likelihood alone.
//  - prior_gate(): want_like of MH_chain::step (chain.cc:980) with oldlprior = current_lpost - invtemp * current_llike (:973), every
//    operation rounded on its own, in the order the host path (callback_host_part, ptm_engine.hip) has always taken them.  Plain C++:
//    tests/cxx/devprior_gate_main.cc includes this header without HIP.
//  - devprior_gate_kernel: one thread per ROW of the prior's batch.  The pack's row -> chain index is a permutation of the chains whose
//    first `count` entries are the chains with gate bit 1, so row k < count carries chain c's log-prior: lprior_new[c] = it, gate[c] =
//    1 | (want ? 2 : 0).  A row past the count names a chain without bit 1: lprior_new[c] = -inf, its gate byte stays as the propose pass
//    wrote it.  Every chain is written by exactly one thread.
//  - devprior_valid_kernel / devprior_states_kernel: the set-up calls (ptm_set_states, ptm_restore).  The chains whose device-side lprior
//    is above -inf are the valid ones; the user's log-prior replaces theirs, the others keep -inf.
// Vector stores only; nothing here is written through the scalar unit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTM_PRIOR_FN __host__ __device__ inline
#else
#define PTM_PRIOR_FN inline
#endif

namespace ptm {

// the gate byte of a valid proposal whose log-prior is `nl`: bit 1 (valid) | bit 2 (the likelihood is wanted).  lprior / llike / beta:
// the chain's current log-prior, log-likelihood and inverse temperature.  No contraction: a fused multiply-add would not round bl.
PTM_PRIOR_FN unsigned char prior_gate(double nl, double lprior, double llike, double beta, double min_prior) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double bl = beta * llike;
  const double cur_lpost = lprior + bl;
  const double oldlprior = cur_lpost - bl;
  const bool want = nl > -1e200 || nl - oldlprior > min_prior;
  return (unsigned char)(1 | (want ? 2 : 0));
}

#if defined(__HIPCC__)

constexpr int DEVPRIOR_THREADS = 256;

// grid: ceil(n / DEVPRIOR_THREADS).  betaC: the chains' own inverse temperatures (evolving ladders) or nullptr: beta[r0 + c / W]
__global__ __launch_bounds__(DEVPRIOR_THREADS) void devprior_gate_kernel(int n, int W, int r0, const int32_t* __restrict__ count,
                                                                        const int* __restrict__ row_chain, const double* __restrict__ out,
                                                                        const double* __restrict__ lp, const double* __restrict__ ll,
                                                                        const double* __restrict__ beta, const double* __restrict__ betaC,
                                                                        double min_prior, double* __restrict__ lprior_new,
                                                                        unsigned char* __restrict__ gate) {
  const int k = blockIdx.x * DEVPRIOR_THREADS + threadIdx.x;
  if (k >= n) return;
  const int c = row_chain[k];
  if (c < 0 || c >= n) return;   // (never: the pack writes a permutation)
  if (k < count[0]) {
    const double nl = out[k];
    const double b = betaC ? betaC[c] : beta[r0 + c / W];
    lprior_new[c] = nl;
    gate[c] = prior_gate(nl, lp[c], ll[c], b, min_prior);
  } else {
    lprior_new[c] = -__builtin_inf();
  }
}

// set-up: gate[c] = 1 for the chains whose device-side lprior is above -inf (the valid ones), else 0
__global__ __launch_bounds__(DEVPRIOR_THREADS) void devprior_valid_kernel(int n, const double* __restrict__ lp, unsigned char* __restrict__ gate) {
  const int c = blockIdx.x * DEVPRIOR_THREADS + threadIdx.x;
  if (c < n) gate[c] = lp[c] > -__builtin_inf() ? 1 : 0;
}

// set-up: lp[chain[k]] = out[k] for k < count; the other chains keep their -inf
__global__ __launch_bounds__(DEVPRIOR_THREADS) void devprior_states_kernel(int n, const int32_t* __restrict__ count, const int* __restrict__ row_chain,
                                                                          const double* __restrict__ out, double* __restrict__ lp) {
  const int k = blockIdx.x * DEVPRIOR_THREADS + threadIdx.x;
  if (k >= n || k >= count[0]) return;
  const int c = row_chain[k];
  if (c >= 0 && c < n) lp[c] = out[k];
}

#endif  // __HIPCC__

}  // namespace ptm
