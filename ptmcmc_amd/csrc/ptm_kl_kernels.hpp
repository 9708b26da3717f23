// ptm_kl_kernels.hpp -- exact nearest-neighbour squared distances for the k-NN Kullback-Leibler estimator (ptm_nn_dist2): the
// facade's kl_estimator::one_nnd2 / all_nnd2 (ptmcmc_amd/host/ptmcmc_gpu.hh; test_proposal.hh:424-464, state::dist2
// states.cc:207-233) restated with one lane per query point.  The reference falls back to approximate neighbours at the sampler's
// sizes; here the exact search is brute force, O(nP nQ dim), on the device.
//
//  - kl_prepare_kernel: lane = (point, padded dimension).  It lays a set out for the search -- the queries dimension-major
//    [d][nP padded to the block] so a wave's loads are consecutive, the searched set point-major [j][row] so a tile is one
//    contiguous run of wave-uniform addresses -- pads the dimensions up to DP with zeros (|0 - 0|^2 adds +0.0 to a sum that is never
//    negative: no bit changes) and, with a wrapped dimension, writes the coordinate's alternative beside it: the point shifted by
//    half the domain and wrap-enforced (boundary_enforce, the sweeps' own).  state::dist2 shifts and enforces the two points of a
//    pair separately, so the alternative belongs to the point, not the pair: it is formed once per point.  A dimension that is not
//    wrapped repeats the coordinate: |xb' - xa'| is |xb - xa| there and the smaller of the two is either.
//  - kl_nn_kernel<DP, WRAP>: lane = query point i; blockIdx.y = a split of the searched set, rows [y per_split,
//    (y + 1) per_split).  Per pair, in dimension order: diff = |xb - xa| (WRAP: the smaller of it and the alternative's),
//    sum += diff * diff -- multiply, then add; the engine is compiled with -ffp-contract=off -- so each pair's sum carries the host's
//    bits; the minimum over pairs is exact in any order.  The query's coordinates stay in registers (DP <= KL_CHUNK; above, KL_TILE
//    running sums are kept and the query is re-read chunk by chunk, still in dimension order).  The searched set streams through in
//    tiles of KL_TILE points whose addresses are the same in every lane; they are read where they lie, and the compiler turns the
//    uniform reads into scalar loads.  (A tile copied into LDS first, where one address is a broadcast, was measured beside it at
//    10000 .. 40000 points in 2, 6 and 32 dimensions: the same times within the spread of repeats, so the kernel keeps no LDS and
//    no barrier.)  same_set: pair (i, i) is skipped, a duplicate elsewhere still gives 0.
//  - kl_min_kernel: lane = query point; the minimum over the splits' partial minima [splits][nP].  No floating-point atomics.
// The Gaussian "fake KL" of the same test stays on the host: it is O(N dim^2), a few milliseconds at the sampler's sizes.
// Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_kernels.hpp"

namespace ptm {

constexpr int KL_THREADS = 64;    // lanes per workgroup: one wave, so that ten thousand queries already are 157 workgroups
constexpr int KL_TILE = 16;       // points of the searched set per tile
constexpr int KL_CHUNK = 32;      // most dimensions of a query held in registers at a time (half of it with alternatives)
constexpr int KL_MAX_DIM = 128;

constexpr int kl_chunk(int DP, bool WRAP) { return DP < (WRAP ? KL_CHUNK / 2 : KL_CHUNK) ? DP : (WRAP ? KL_CHUNK / 2 : KL_CHUNK); }
constexpr int kl_row(int DP, bool WRAP) { return WRAP ? 2 * DP : DP; }   // doubles per point of the searched set

// out[i * point_stride + d * dim_stride] = X[i][d] (0 for dim <= d < DP); alt: the same place + alt_offset holds the alternative
__global__ __launch_bounds__(256) void kl_prepare_kernel(const double* __restrict__ X, long long n, int dim, int DP, const int* __restrict__ wrapped,
                                                         const double* __restrict__ xmin, const double* __restrict__ xmax, double* __restrict__ out,
                                                         long long point_stride, long long dim_stride, long long alt_offset, int alt) {
  const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= n * DP) return;
  const long long i = lane / DP;
  const int d = (int)(lane - i * DP);
  const double x = d < dim ? X[i * dim + d] : 0.0;
  const long long at = i * point_stride + d * dim_stride;
  out[at] = x;
  if (!alt) return;
  double xa = x;
  if (d < dim && wrapped[d]) {
    const double halfwrap = (xmax[d] - xmin[d]) / 2;
    xa -= halfwrap;
    (void)boundary_enforce(B_WRAP, B_WRAP, xmin[d], xmax[d], xa);
  }
  out[at + alt_offset] = xa;
}

// Pt: the queries [kl_row(DP)][nP_pad] (nP_pad a multiple of KL_THREADS: every lane of the grid has a column); Qr: the searched set
// [nQ_pad][kl_row(DP)] (nQ_pad a multiple of KL_TILE: every tile is there); per_split a multiple of KL_TILE; part [gridDim.y][nP]
template <int DP, bool WRAP>
__global__ __launch_bounds__(KL_THREADS) void kl_nn_kernel(const double* __restrict__ Pt, long long nP_pad, int nP, const double* __restrict__ Qr, int nQ,
                                                           int per_split, int same_set, double* __restrict__ part) {
  constexpr int CH = kl_chunk(DP, WRAP), NCH = DP / CH, ROW = kl_row(DP, WRAP);
  const int i = blockIdx.x * KL_THREADS + threadIdx.x;   // (< nP_pad)
  const long long j0 = (long long)blockIdx.y * per_split;
  const long long j1 = j0 + per_split < nQ ? j0 + per_split : nQ;
  const double* pcol = Pt + i;
  double p[CH], pa[WRAP ? CH : 1];
  if (NCH == 1) {
#pragma unroll
    for (int d = 0; d < CH; ++d) {
      p[d] = pcol[d * nP_pad];
      if (WRAP) pa[d] = pcol[(DP + d) * nP_pad];
    }
  }
  double best = INFINITY;
  for (long long t = j0; t < j1; t += KL_TILE) {
    const double* q = Qr + t * ROW;   // (the same in every lane)
    double acc[KL_TILE];
#pragma unroll
    for (int jj = 0; jj < KL_TILE; ++jj) acc[jj] = 0.0;
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
      if (NCH > 1) {
#pragma unroll
        for (int d = 0; d < CH; ++d) {
          p[d] = pcol[(c * CH + d) * nP_pad];
          if (WRAP) pa[d] = pcol[(DP + c * CH + d) * nP_pad];
        }
      }
#pragma unroll
      for (int jj = 0; jj < KL_TILE; ++jj) {
#pragma unroll
        for (int d = 0; d < CH; ++d) {
          double diff = __builtin_fabs(q[jj * ROW + c * CH + d] - p[d]);
          if (WRAP) {
            const double altdiff = __builtin_fabs(q[jj * ROW + DP + c * CH + d] - pa[d]);
            if (altdiff < diff) diff = altdiff;
          }
          acc[jj] += diff * diff;
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < KL_TILE; ++jj) {
      const long long j = t + jj;
      if (j < j1 && !(same_set && j == i) && acc[jj] < best) best = acc[jj];
    }
  }
  if (i < nP) part[(long long)blockIdx.y * nP + i] = best;
}

__global__ __launch_bounds__(256) void kl_min_kernel(const double* __restrict__ part, int splits, int nP, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nP) return;
  double best = part[i];
  for (int s = 1; s < splits; ++s) {
    const double v = part[(long long)s * nP + i];
    if (v < best) best = v;
  }
  out[i] = best;
}

}  // namespace ptm
