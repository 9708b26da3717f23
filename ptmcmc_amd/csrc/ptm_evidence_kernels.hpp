// ptm_evidence_kernels.hpp -- the log-evidence by thermodynamic integration over the ladder (ptm_log_evidence): the facade's
// evidence_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh; parallel_tempering_chains::log_evidence_ratio, chain.cc:1984-2012, and the
// total of chain.cc:1585-1597) restated with one lane per recorded chain.
//
//  - evidence_ratio_kernel: lane = rung * W + walker (the walker fastest: a wave reads consecutive doubles of llike[slot * HC + chain]).
//    The lane takes its chain's own count of add_state calls, forms the window of MH_chain::get_state_idx (chain.cc:1041-1049) --
//    saved rows [1 + (Nhist - ilen) / add_every, 1 + (Nhist - 1) / add_every): the newest saved row is left out, a chain shorter
//    than ilen has an empty window -- and walks the rows in order.  Each row is loaded once and feeds two sums: the pair below's
//    "up" ratio (beta[r-1] - beta[r]) and the pair above's "down" ratio (beta[r+1] - beta[r]).  The loads of EVID_AHEAD rows are issued
//    before their adds, so the walk is not one dependent load per row.
//    CHECK: the ring has wrapped, so a row is there only if its slot still names it (meta.w); a missing row raises *flag and the
//    caller throws the launch's outputs away.
//  - evidence_total_kernel: lane = walker; the sequential sum over the pairs and the extrapolation below the hottest rung.
// Every sum is one lane's own sequential sum in the host's order -- multiply, then add; the engine is compiled with
// -ffp-contract=off -- so the answers carry the host estimator's bits; nothing is reduced across lanes.
// Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ptm {

constexpr int EVID_THREADS = 256;   // lanes per workgroup
constexpr int EVID_AHEAD = 8;       // rows whose loads are in flight before the first of their adds

struct EvidSrc {
  const double* ll;            // the ring's llikes: [slot * HC + chain]
  const int4* meta;            // [slot * HC + chain].w: the saved row number the slot holds
  const unsigned int* nhist;   // [chain] add_state calls
  const double* beta;          // [Nt] the common ladder ...
  const double* beta_w;        // ... or, once the ladders evolve, each walker's own: [walker * Nt + rung] (else null)
  int HC, cap, W, Nt, add_every, ilen;
};
__device__ __forceinline__ double evid_beta(const EvidSrc& s, int r, int w) { return s.beta_w ? s.beta_w[(long long)w * s.Nt + r] : s.beta[r]; }
// MH_chain::get_state_idx in the ring's numbering (the start state is row 0 however many initial rows the reference would hold in
// front, Nzero = 0): an i outside [0, Nhist) becomes Nhist - 1 (C division, towards zero)
__device__ __forceinline__ long long evid_idx(long long i, long long nhist, int add_every) {
  if (i < 0 || i >= nhist) i = nhist - 1;
  return 1 + i / add_every;
}

template <bool CHECK>
__global__ __launch_bounds__(EVID_THREADS) void evidence_ratio_kernel(EvidSrc s, double* __restrict__ up, double* __restrict__ down, int* __restrict__ count,
                                                                      int* __restrict__ flag) {
  const int c = blockIdx.x * EVID_THREADS + threadIdx.x;
  if (c >= s.Nt * s.W) return;
  const int r = c / s.W, w = c - r * s.W;
  const long long nh = s.nhist[c];
  const long long first = evid_idx(nh - s.ilen, nh, s.add_every), last = evid_idx(nh, nh, s.add_every);
  const double b = evid_beta(s, r, w);
  const double amb_up = r > 0 ? evid_beta(s, r - 1, w) - b : 0.0, amb_dn = r + 1 < s.Nt ? evid_beta(s, r + 1, w) - b : 0.0;
  const double* lls = s.ll + c;
  const int4* ms = s.meta + c;
  double s_up = 0, s_dn = 0;
  bool missing = false;
  for (long long row = first; row < last; row += EVID_AHEAD) {
    double v[EVID_AHEAD];
    bool there[EVID_AHEAD];
#pragma unroll
    for (int k = 0; k < EVID_AHEAD; ++k) {
      const long long rk = row + k;
      const bool in = rk < last;
      const long long slot = CHECK ? rk % s.cap : rk;   // (not wrapped: last <= cap - 1, the slot is the row)
      v[k] = in ? lls[slot * s.HC] : 0.0;
      there[k] = (CHECK && in) ? ms[slot * s.HC].w == (int)rk : true;
    }
#pragma unroll
    for (int k = 0; k < EVID_AHEAD; ++k) {
      if (row + k >= last) break;
      if (!there[k]) missing = true;
      s_up += v[k] * amb_up;
      s_dn += v[k] * amb_dn;
    }
  }
  if (missing) *flag = 1;
  const long long n = last > first ? last - first : 0;
  const double cnt = (double)n;   // (0: the reference's 0 / 0)
  if (r > 0) up[(long long)(r - 1) * s.W + w] = s_up / cnt;
  if (r + 1 < s.Nt) down[(long long)r * s.W + w] = -(s_dn / cnt);
  count[c] = (int)n;
}

__global__ __launch_bounds__(EVID_THREADS) void evidence_total_kernel(EvidSrc s, const double* __restrict__ up, const double* __restrict__ down,
                                                                      double* __restrict__ evidence) {
  const int w = blockIdx.x * EVID_THREADS + threadIdx.x;
  if (w >= s.W) return;
  double ev = 0;
  for (int i = 0; i < s.Nt - 1; ++i) ev += (up[(long long)i * s.W + w] + down[(long long)i * s.W + w]) / 2.0;
  const long long o = (long long)(s.Nt - 2) * s.W + w;
  const double dE = (up[o] + down[o]) / 2.0 / (evid_beta(s, s.Nt - 2, w) / evid_beta(s, s.Nt - 1, w) - 1);
  evidence[w] = ev + dE;
}

}  // namespace ptm
