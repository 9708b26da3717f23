// ptm_rhat_kernels.hpp -- split R-hat across the walkers of a recorded rung (ptm_rhat, ptm_rhat_series): the facade's
// rhat_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated with one lane per (walker, half, feature).  The Gelman-Rubin diagnostic
// on split chains (Gelman et al., "Bayesian Data Analysis", 3rd ed., sec. 11.4); the reference runs one ladder and has no counterpart.
//
// A chain is one walker's saved rows -- the history ring of a recorded rung, or a caller's plain array -- and its first nfeat
// parameters are the features.  Its window is its own newest nrows saved rows, newest = first_row + (steps - 1) / add_every (the row
// ESS assigns to nominal step steps - 1): rows newest - nrows + 1 .. newest in ascending order; the first n = nrows / 2 of them are
// sequence 2w, the others sequence 2w + 1.
//  - rhat_sequence_kernel: lane = (2w + half) * nfeat + f, the feature fastest: in the ring layout a wave reads consecutive doubles
//    across features and neighbouring walkers.  Two walks over the lane's n rows: mean = (sum x) / n, then
//    var = (sum (x - mean) * (x - mean)) / (n - 1).  The loads of RHAT_AHEAD rows are issued before their adds.
//    CHECK: the ring has wrapped, so a row is there only if its slot still names it (meta.w); a missing row raises *flag and the
//    caller throws the launch's outputs away.
//  - rhat_reduce_kernel: lane = feature; the sequential loops over the m = 2W sequences: M = (sum mean_k) / m,
//    between = n * (sum (mean_k - M)^2) / (m - 1), within = (sum var_k) / m, var_plus = ((n - 1) / n) * within + between / n.
//    It stays one lane per feature so that the order of the adds -- and with it every bit -- is defined.
// Every sum is one lane's own sequential sum in the host's order -- multiply, then add; the engine is compiled with
// -ffp-contract=off -- so the answers carry the host estimator's bits; nothing is reduced across lanes.  The final
// sqrt(var_plus / within) is formed on the host.
// Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_ess_kernels.hpp"

namespace ptm {

constexpr int RHAT_THREADS = 256;   // lanes per workgroup
constexpr int RHAT_AHEAD = 8;       // rows whose loads are in flight before the first of their adds
constexpr int RHAT_REDUCE_AHEAD = 32;   // ... and sequences, in the reduce kernel (one wave at most: nothing else hides the latency)

// slot of saved row `row` of a chain (ms: its column of the meta table), or -1 if the ring no longer holds the row
template <bool CHECK>
__device__ __forceinline__ long long rhat_slot(const EssSrc& s, const int4* ms, long long row) {
  if (!CHECK) return row;   // (not wrapped: newest < cap, the slot is the row)
  const long long slot = row % s.cap;
  return ms[slot * s.meta_stride].w == (int)row ? slot : -1;
}

// nhist: [walker] each chain's own count of add_state calls (null: src.steps for all)
template <bool CHECK>
__global__ __launch_bounds__(RHAT_THREADS) void rhat_sequence_kernel(EssSrc src, const unsigned int* __restrict__ nhist, int W, int nfeat, int nrows,
                                                                     double* __restrict__ seq_mean, double* __restrict__ seq_var, int* __restrict__ flag) {
  const long long lane = (long long)blockIdx.x * RHAT_THREADS + threadIdx.x;
  if (lane >= 2ll * W * nfeat) return;
  const int k = (int)(lane / nfeat), f = (int)(lane - (long long)k * nfeat);
  const int w = k >> 1, half = k & 1, n = nrows / 2;
  const long long steps = nhist ? (long long)nhist[w] : (long long)src.steps;
  const long long newest = src.first_row + (steps - 1) / src.add_every;
  const long long first = newest - nrows + 1 + (long long)half * n;
  // (the caller has checked all of this: a lane never reads outside the ring)
  if (steps < 1 || newest - nrows + 1 < src.first_row || nrows > src.cap || (!CHECK && newest >= src.cap)) { *flag = 1; return; }
  const double* xs = src.x + (long long)w * src.series_stride + ess_pos(src, f);
  const int4* ms = CHECK ? src.meta + w : nullptr;
  bool missing = false;
  double sum = 0;
  for (int i = 0; i < n; i += RHAT_AHEAD) {
    double v[RHAT_AHEAD];
#pragma unroll
    for (int j = 0; j < RHAT_AHEAD; ++j) {
      const long long slot = i + j < n ? rhat_slot<CHECK>(src, ms, first + i + j) : 0;
      if (slot < 0) missing = true;
      v[j] = (i + j < n && slot >= 0) ? xs[slot * src.slot_stride] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < RHAT_AHEAD; ++j) {
      if (i + j >= n) break;
      sum += v[j];
    }
  }
  if (missing) { *flag = 1; return; }
  const double mean = sum / (double)n;
  double ssq = 0;
  for (int i = 0; i < n; i += RHAT_AHEAD) {   // (every row was there a moment ago: the slots need no second look)
    double v[RHAT_AHEAD];
#pragma unroll
    for (int j = 0; j < RHAT_AHEAD; ++j) {
      const long long row = first + i + j;
      v[j] = i + j < n ? xs[(CHECK ? row % src.cap : row) * src.slot_stride] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < RHAT_AHEAD; ++j) {
      if (i + j >= n) break;
      const double d = v[j] - mean;
      ssq += d * d;
    }
  }
  seq_mean[lane] = mean;
  seq_var[lane] = ssq / (double)(n - 1);
}

// out[f], out[nfeat + f], out[2 nfeat + f], out[3 nfeat + f] = M, within, between, var_plus of feature f
__global__ __launch_bounds__(RHAT_THREADS) void rhat_reduce_kernel(int m, int nfeat, int n, const double* __restrict__ seq_mean,
                                                                   const double* __restrict__ seq_var, double* __restrict__ out) {
  const int f = blockIdx.x * RHAT_THREADS + threadIdx.x;
  if (f >= nfeat) return;
  const double nd = (double)n, md = (double)m;
  const double *sm = seq_mean + f, *sv = seq_var + f;
  // two walks over the sequences (the second needs M); each sum is its own sequential chain over k = 0 .. m - 1, and the loads of
  // RHAT_REDUCE_AHEAD sequences are issued before their adds: the walk is not one dependent load per sequence
  double msum = 0, wsum = 0;
  for (int k0 = 0; k0 < m; k0 += RHAT_REDUCE_AHEAD) {
    double a[RHAT_REDUCE_AHEAD], v[RHAT_REDUCE_AHEAD];
#pragma unroll
    for (int j = 0; j < RHAT_REDUCE_AHEAD; ++j) {
      const bool in = k0 + j < m;
      a[j] = in ? sm[(long long)(k0 + j) * nfeat] : 0.0;
      v[j] = in ? sv[(long long)(k0 + j) * nfeat] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < RHAT_REDUCE_AHEAD; ++j) {
      if (k0 + j < m) {
        msum += a[j];
        wsum += v[j];
      }
    }
  }
  const double M = msum / md;
  double bsum = 0;
  for (int k0 = 0; k0 < m; k0 += RHAT_REDUCE_AHEAD) {
    double a[RHAT_REDUCE_AHEAD];
#pragma unroll
    for (int j = 0; j < RHAT_REDUCE_AHEAD; ++j) a[j] = k0 + j < m ? sm[(long long)(k0 + j) * nfeat] : 0.0;
#pragma unroll
    for (int j = 0; j < RHAT_REDUCE_AHEAD; ++j) {
      if (k0 + j < m) {
        const double d = a[j] - M;
        bsum += d * d;
      }
    }
  }
  const double between = nd * bsum / (md - 1.0), within = wsum / md;
  out[f] = M;
  out[nfeat + f] = within;
  out[2 * nfeat + f] = between;
  out[3 * nfeat + f] = ((nd - 1.0) / nd) * within + between / nd;
}

}  // namespace ptm
