// ptm_ess_kernels.hpp -- effective sample size of many saved series at once (ptm_ess_*): the facade's
// ess_estimator::windowed (ptmcmc_amd/host/ptmcmc_gpu.hh; chain::report_effective_samples, chain.cc:126-643) restated with one
// lane per (series, feature).
//
// A series is one chain's saved rows -- the history ring of a recorded rung, or a caller's plain array -- and its first nfeat
// parameters are the features.  Three passes per chunk of series (the table of a chunk must fit the workspace):
//  - ess_accumulate_kernel: grid (lane blocks, windows, lag chunks).  A lane walks its window's samples in the order i = 0, 1, ...
//    and keeps the sums of ESS_LAGS lags in registers, so a base sample is loaded once per lag chunk; it then forms the cell
//    {mean, cov, count} of each of its lags exactly as the host does.  Lanes are feature-fastest: in the ring layout a wave reads
//    consecutive doubles across features and neighbouring walkers.
//  - ess_combine_kernel: per lane, for n = 1 .. nwin newest windows: M, rho(L), the initially-positive-sequence cut, the length
//    and ess(n) of that feature.
//  - ess_reduce_kernel: per series, the minimum over features and the best n (the first n wins ties).
// The series of a pass may differ in length (EssWho): each lane derives its series' windows from that series' own step count.
// Every sum is a lane's own sequential sum in the host's order and the engine is compiled with -ffp-contract=off, so the answers
// carry the host estimator's bits; nothing is reduced across lanes but the exact minimum and the comparison of the last pass.
// Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ptm {

constexpr int ESS_LAGS = 8;        // lags a lane accumulates per pass over its window
constexpr int ESS_THREADS = 256;   // lanes per workgroup

// where the samples are: element (slot, series, feature) at x[slot * slot_stride + series * series_stride + pos(feature)]
struct EssSrc {
  const double* x;
  const int4* meta;         // ring: [slot * meta_stride + series].w is the saved row number held by the slot; null: every row is there
  long long slot_stride;    // doubles between two slots
  long long meta_stride;    // int4s between two slots
  int series_stride;        // doubles between two series
  int cap;                  // slots
  int add_every;            // nominal steps per saved row
  int first_row;            // row number of nominal step 0 (the ring: 1, behind the start state; a plain series: 0)
  int permuted;             // rows in the accumulator layout of the 32 / 64 / 128-dimensional kernels (row_pos)
  int steps;                // nominal steps of the series: a sample of step < 0 or >= steps does not exist
};
// which series a pass works on, and each one's own length.  A chain's count of add_state calls is its own (a rung exchanged twice in
// a step makes one more), so the series of one rung differ in `steps`, and with it in the number of windows and where they begin.
struct EssWho {
  const int* sel;        // local series k is series sel[k] of the source (null: k itself)
  const int* steps_of;   // [series of the source] its nominal steps (null: EssSrc::steps for all)
  int span, burn;        // steps a window covers, windows in front that only feed the lags
};
__device__ __forceinline__ int ess_series(const EssWho& q, int local) { return q.sel ? q.sel[local] : local; }
__device__ __forceinline__ int ess_steps(const EssSrc& s, const EssWho& q, int series) { return q.steps_of ? q.steps_of[series] : s.steps; }
// windows of a series (ess_estimator::windowed: steps / span - burn), none if that is below 1; never more than the table holds
__device__ __forceinline__ int ess_nwin(int steps, const EssWho& q, int nwin_max) {
  const int n = steps / q.span - q.burn;
  return n < 0 ? 0 : (n > nwin_max ? nwin_max : n);
}

__device__ __forceinline__ int ess_pos(const EssSrc& s, int f) {
  return s.permuted ? 8 * (f >> 3) + 2 * (f & 3) + ((f >> 2) & 1) : f;
}
// the sample of nominal step `step`: its slot, or -1 if it does not exist (cold_row's rule)
__device__ __forceinline__ long long ess_slot(const EssSrc& s, int steps, int series, int step) {
  if (step < 0 || step >= steps) return -1;
  const int idx = s.first_row + step / s.add_every;
  const int slot = idx % s.cap;
  if (s.meta && s.meta[(long long)slot * s.meta_stride + series].w != idx) return -1;
  return slot;
}

// table of a chunk of `lanes` = series x nfeat lanes: cell (w, l) of a lane at (w * nlag + l) * lanes + lane.
// LINEAR: the stride is a multiple of add_every and the ring has not wrapped (a plain series always), so the saved row of a
// sample is row(w0) + i * (every / add_every) - lag / add_every and its slot is the row itself: no division per sample.
template <bool LINEAR>
__global__ __launch_bounds__(ESS_THREADS) void ess_accumulate_kernel(EssSrc src, EssWho who, int series0, int lanes, int nfeat, int per_window, int every,
                                                                     int nlag, const int* __restrict__ lags, double* __restrict__ mean,
                                                                     double* __restrict__ cov, int* __restrict__ count) {
  const int lane = blockIdx.x * ESS_THREADS + threadIdx.x;
  if (lane >= lanes) return;
  const int series = ess_series(who, series0 + lane / nfeat), pos = ess_pos(src, lane % nfeat);
  const int steps = ess_steps(src, who, series), nwin = ess_nwin(steps, who, (int)gridDim.y);
  const int w = blockIdx.y, l0 = blockIdx.z * ESS_LAGS;
  if (w >= nwin) return;   // (a shorter series of the pass: its cells of this window are never read)
  const int w0 = steps - nwin * who.span + w * who.span;
  const double* xs = src.x + (long long)series * src.series_stride + pos;
  const int4* ms = src.meta ? src.meta + series : nullptr;
  int lag[ESS_LAGS], lag_rows[ESS_LAGS];
#pragma unroll
  for (int k = 0; k < ESS_LAGS; ++k) {
    lag[k] = l0 + k < nlag ? lags[l0 + k] : -1;
    lag_rows[k] = lag[k] > 0 ? lag[k] / src.add_every : 0;
  }
  const int row0 = src.first_row + w0 / src.add_every, row_step = every / src.add_every;   // (LINEAR; w0 >= 0)
  double s1[ESS_LAGS], s2[ESS_LAGS];
  int n[ESS_LAGS];
#pragma unroll
  for (int k = 0; k < ESS_LAGS; ++k) { s1[k] = 0.0; s2[k] = 0.0; n[k] = 0; }
  for (int i = 0; i < per_window; ++i) {
    const int step = w0 + i * every;
    long long at;
    if (LINEAR) {
      const int row = row0 + i * row_step;
      at = (step < steps && (!ms || ms[(long long)row * src.meta_stride].w == row)) ? row : -1;
    } else at = ess_slot(src, steps, series, step);
    if (at < 0) continue;
    const double base = xs[at * src.slot_stride];
#pragma unroll
    for (int k = 0; k < ESS_LAGS; ++k) {
      if (lag[k] < 0) continue;
      if (lag[k] == 0) {   // (only lag 0 of the list)
        s1[k] += base;
        s2[k] += base * base;
      } else {
        long long at2;
        if (LINEAR) {
          const int row = row0 + i * row_step - lag_rows[k];
          at2 = (step - lag[k] >= 0 && (!ms || ms[(long long)row * src.meta_stride].w == row)) ? row : -1;
        } else at2 = ess_slot(src, steps, series, step - lag[k]);
        if (at2 < 0) continue;
        const double then = xs[at2 * src.slot_stride];
        s1[k] += then + base;
        s2[k] += then * base;
      }
      n[k]++;
    }
  }
#pragma unroll
  for (int k = 0; k < ESS_LAGS; ++k) {
    if (lag[k] < 0) continue;
    const size_t o = ((size_t)w * nlag + (l0 + k)) * (size_t)lanes + lane;
    const double m = lag[k] == 0 ? s1[k] / n[k] : s1[k] / n[k] / 2;
    count[o] = n[k];
    mean[o] = m;
    cov[o] = s2[k] / n[k] - m * m;
  }
}

// e_of_n[(n - 1) * lanes + lane] = this feature's ess over the newest n windows
__global__ __launch_bounds__(ESS_THREADS) void ess_combine_kernel(EssSrc src, EssWho who, int series0, int lanes, int nfeat, int nwin_max, int nlag,
                                                                  const int* __restrict__ lags, int width, int every,
                                                                  const double* __restrict__ mean, const double* __restrict__ cov,
                                                                  const int* __restrict__ count, double* __restrict__ e_of_n) {
  const int lane = blockIdx.x * ESS_THREADS + threadIdx.x;
  if (lane >= lanes) return;
  const size_t L = (size_t)lanes;
  const int nwin = ess_nwin(ess_steps(src, who, ess_series(who, series0 + lane / nfeat)), who, nwin_max);
  for (int n = 1; n <= nwin; ++n) {
    double msum = 0;
    for (int w = nwin - n; w < nwin; ++w) msum += mean[((size_t)w * nlag) * L + lane];
    const double M = msum / n;
    double length = 1.0, last_term = 0, previous = 1;
    int last_lag = 0;
    for (int l = 1; l < nlag; ++l) {
      double top = 0, bottom = 0;
      for (int w = nwin - n; w < nwin; ++w) {
        const size_t o = ((size_t)w * nlag + l) * L + lane, o0 = ((size_t)w * nlag) * L + lane;
        const double dm = M - mean[o], dm0 = M - mean[o0];
        const double cv = cov[o] + dm * dm, var = cov[o0] + dm0 * dm0;
        const int c = count[o];
        top += cv * c;
        bottom += var * c;
      }
      const double rho = top / bottom;
      if (previous < 0 && rho < 0) { length -= last_term; break; }
      previous = rho;
      last_term = 2.0 * (lags[l] - last_lag) * rho;
      length += last_term;
      last_lag = lags[l];
    }
    double e = n * width / length;
    if (length < every) e = n * width / 3.0 / every;
    e_of_n[(size_t)(n - 1) * L + lane] = e;
  }
}

__global__ __launch_bounds__(ESS_THREADS) void ess_reduce_kernel(EssSrc src, EssWho who, int series0, int nseries, int nfeat, int nwin_max,
                                                                 const double* __restrict__ e_of_n, double* __restrict__ ess, int* __restrict__ nwin_out) {
  const int s = blockIdx.x * ESS_THREADS + threadIdx.x;
  if (s >= nseries) return;
  const size_t L = (size_t)nseries * nfeat;
  const int nwin = ess_nwin(ess_steps(src, who, ess_series(who, series0 + s)), who, nwin_max);
  double best = 0;
  int best_n = 0;
  for (int n = 1; n <= nwin; ++n) {
    double worst = 1e100;
    for (int f = 0; f < nfeat; ++f) {
      const double e = e_of_n[(size_t)(n - 1) * L + (size_t)s * nfeat + f];
      if (e < worst) worst = e;
    }
    if (worst > best) { best = worst; best_n = n; }
  }
  ess[s] = best;
  nwin_out[s] = best_n;
}

}  // namespace ptm
