// ptm_moments_kernels.hpp -- pooled posterior mean and covariance over the walkers of a recorded rung (ptm_moments, ptm_moments_series):
// the facade's moments_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated for the device.  The reference runs one ladder and its
// write_covariance / read_covariance are empty (ptmcmc.cc:761-768): no reference counterpart.
//
// A chain is one walker's saved rows -- the history ring of a recorded rung, or a caller's plain array -- and its first nfeat
// parameters are the features.  Its window is its own newest nrows saved rows in ascending order (ptm_rhat's rule).  The definition
// (include/ptm_engine.h) sums in three levels: over a walker's rows, over the MOM_GROUP walkers of a block, over the blocks.
//  - moments_sum_kernel: lane = w * nfeat + f, the feature fastest.  One walk over the lane's rows: the sum of x, or, given the means,
//    of (x - mean) * (x - mean) (the variances alone: nfeat above MOM_COV_NFEAT_MAX, or no covariance asked for).  The loads of
//    MOM_AHEAD rows are issued before their adds.
//  - moments_cross_kernel: a workgroup owns a walker and a chunk of MOM_THREADS * NP pairs, NP <= MOM_PAIRS pairs a lane (as few as
//    hold every pair of a small nfeat in one chunk: only in the last chunk does a lane add up a pair it does not store).  It stages
//    tiles of the window's rows into LDS, coalesced, with the mean taken off once per element, and every lane adds d_i * d_j of
//    its pairs in row order.  Pairs are numbered along the rows of the upper triangle, so the lanes of a wave share i (one
//    address: a broadcast) and step j (consecutive doubles: no bank conflict).
//  - moments_block_kernel: lane = (block, column): the sequential sum of the block's walkers.  Columns are features or pairs.
//  - moments_final_kernel: lane = column: the sequential sum over the blocks, divided; for pairs both triangles are written.
// CHECK: the ring has wrapped, so a row is there only if its slot still names it; a missing row raises *flag and the caller throws
// the launch's outputs away.
// Every sum is one lane's own sequential sum in the host's order -- multiply, then add; the engine is compiled with
// -ffp-contract=off -- so the answers carry the host estimator's bits; nothing is reduced across lanes.
// Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_rhat_kernels.hpp"

namespace ptm {

constexpr int MOM_THREADS = 256;          // lanes per workgroup
constexpr int MOM_AHEAD = 8;              // rows (walkers, blocks) whose loads are in flight before the first of their adds
constexpr int MOM_GROUP = 64;             // walkers of a block: G of the definition
constexpr int MOM_PAIRS = 4;              // pairs a lane of the cross kernel accumulates, at most
constexpr int MOM_TILE_DOUBLES = 4096;    // the staging tile: 32 KiB of the CU's 160 KiB, five workgroups (20 waves) a CU
constexpr int MOM_COV_NFEAT_MAX = 128;    // the covariance is offered up to here: a row of the tile is then at most 1 KiB
// rows of the window a staging tile holds (nfeat <= MOM_COV_NFEAT_MAX: at least 32)
__host__ __device__ inline int moments_tile_rows(int nfeat) { return MOM_TILE_DOUBLES / nfeat; }

// pair p of the upper triangle, numbered along its rows: (0,0) (0,1) .. (0,nfeat-1) (1,1) ..
__host__ __device__ inline void moments_pair(int nfeat, long long p, int* i, int* j) {
  int row = 0, len = nfeat;
  while (p >= len) { p -= len; --len; ++row; }
  *i = row;
  *j = row + (int)p;
}

// the first row of walker w's window; false: the window is not one the caller has checked (a lane never reads outside the ring)
template <bool CHECK>
__device__ __forceinline__ bool moments_window(const EssSrc& src, const unsigned int* nhist, int w, int nrows, long long* first) {
  const long long steps = nhist ? (long long)nhist[w] : (long long)src.steps;
  const long long newest = src.first_row + (steps - 1) / src.add_every;
  *first = newest - nrows + 1;
  return !(steps < 1 || *first < src.first_row || nrows > src.cap || (!CHECK && newest >= src.cap));
}

// out[w * nfeat + f] = sum over the window's rows of x (mean null) or of (x - mean[f]) * (x - mean[f])
template <bool CHECK>
__global__ __launch_bounds__(MOM_THREADS) void moments_sum_kernel(EssSrc src, const unsigned int* __restrict__ nhist, int W, int nfeat, int nrows,
                                                                  const double* __restrict__ mean, double* __restrict__ out, int* __restrict__ flag) {
  const long long lane = (long long)blockIdx.x * MOM_THREADS + threadIdx.x;
  if (lane >= (long long)W * nfeat) return;
  const int w = (int)(lane / nfeat), f = (int)(lane - (long long)w * nfeat);
  long long first;
  if (!moments_window<CHECK>(src, nhist, w, nrows, &first)) { *flag = 1; return; }
  const double* xs = src.x + (long long)w * src.series_stride + ess_pos(src, f);
  const int4* ms = CHECK ? src.meta + w : nullptr;
  const bool squares = mean != nullptr;
  const double m = squares ? mean[f] : 0.0;
  bool missing = false;
  double sum = 0;
  for (int i = 0; i < nrows; i += MOM_AHEAD) {
    double v[MOM_AHEAD];
#pragma unroll
    for (int j = 0; j < MOM_AHEAD; ++j) {
      const long long slot = i + j < nrows ? rhat_slot<CHECK>(src, ms, first + i + j) : 0;
      if (slot < 0) missing = true;
      v[j] = (i + j < nrows && slot >= 0) ? xs[slot * src.slot_stride] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < MOM_AHEAD; ++j) {
      if (i + j >= nrows) break;
      if (squares) {
        const double d = v[j] - m;
        sum += d * d;
      } else sum += v[j];
    }
  }
  if (missing) { *flag = 1; return; }
  out[lane] = sum;
}

// c_w[(w - w0) * npairs + p] = sum over walker w's window, in row order, of d_i * d_j for pair p = (i, j), d = x - mean.
// grid (walkers of the launch, chunks of MOM_THREADS * NP pairs); nfeat <= MOM_COV_NFEAT_MAX.
template <bool CHECK, int NP>
__global__ __launch_bounds__(MOM_THREADS) void moments_cross_kernel(EssSrc src, const unsigned int* __restrict__ nhist, int w0, int nfeat, int nrows, int npairs,
                                                                    const double* __restrict__ mean, double* __restrict__ c_w, int* __restrict__ flag) {
  __shared__ double tile[MOM_TILE_DOUBLES];
  const int w = w0 + (int)blockIdx.x, tid = (int)threadIdx.x;
  const int p0 = (int)blockIdx.y * (MOM_THREADS * NP);
  long long first;
  if (!moments_window<CHECK>(src, nhist, w, nrows, &first)) {   // (the same for every lane of the workgroup: no lane waits at a barrier)
    if (tid == 0) *flag = 1;
    return;
  }
  const double* xs = src.x + (long long)w * src.series_stride;
  const int4* ms = CHECK ? src.meta + w : nullptr;
  int pi[NP], pj[NP];
  double acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int p = p0 + k * MOM_THREADS + tid;
    pi[k] = 0; pj[k] = 0; acc[k] = 0.0;
    if (p < npairs) moments_pair(nfeat, p, &pi[k], &pj[k]);   // (a lane past the last pair adds up pair (0,0) and stores nothing)
  }
  const int tile_rows = moments_tile_rows(nfeat);
  bool missing = false;
  for (int r0 = 0; r0 < nrows; r0 += tile_rows) {
    const int nr = nrows - r0 < tile_rows ? nrows - r0 : tile_rows, count = nr * nfeat;   // (count <= MOM_TILE_DOUBLES)
    __syncthreads();   // the tile before this one has been used up
#pragma unroll 4
    for (int e = tid; e < count; e += MOM_THREADS) {
      const int r = e / nfeat, f = e - r * nfeat;
      const long long slot = rhat_slot<CHECK>(src, ms, first + r0 + r);
      if (slot < 0) missing = true;
      tile[e] = slot >= 0 ? xs[slot * src.slot_stride + ess_pos(src, f)] - mean[f] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const double* t = tile + r * nfeat;
#pragma unroll
      for (int k = 0; k < NP; ++k) acc[k] += t[pi[k]] * t[pj[k]];
    }
  }
  if (missing) *flag = 1;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int p = p0 + k * MOM_THREADS + tid;
    if (p < npairs) c_w[(size_t)blockIdx.x * npairs + p] = acc[k];
  }
}

// out[b * ncol + c] = the sequential sum over the walkers of block b (of the nw walkers at `in`) of in[w * ncol + c]
__global__ __launch_bounds__(MOM_THREADS) void moments_block_kernel(int nw, int ncol, const double* __restrict__ in, double* __restrict__ out) {
  const long long lane = (long long)blockIdx.x * MOM_THREADS + threadIdx.x;
  const int nblocks = (nw + MOM_GROUP - 1) / MOM_GROUP;
  if (lane >= (long long)nblocks * ncol) return;
  const int b = (int)(lane / ncol), c = (int)(lane - (long long)b * ncol);
  const int begin = b * MOM_GROUP, n = nw - begin < MOM_GROUP ? nw - begin : MOM_GROUP;
  const double* p = in + (size_t)begin * ncol + c;
  double sum = 0;
  for (int k0 = 0; k0 < n; k0 += MOM_AHEAD) {
    double v[MOM_AHEAD];
#pragma unroll
    for (int j = 0; j < MOM_AHEAD; ++j) v[j] = k0 + j < n ? p[(size_t)(k0 + j) * ncol] : 0.0;
#pragma unroll
    for (int j = 0; j < MOM_AHEAD; ++j)
      if (k0 + j < n) sum += v[j];
  }
  out[lane] = sum;
}

// column c: (the sequential sum over the blocks of in[b * ncol + c]) / denom, to out[c]; tri_nfeat > 0: the columns are the pairs
// of tri_nfeat features and the quotient goes to out[i * tri_nfeat + j] and out[j * tri_nfeat + i]
__global__ __launch_bounds__(MOM_THREADS) void moments_final_kernel(int nblocks, int ncol, const double* __restrict__ in, double denom, int tri_nfeat,
                                                                    double* __restrict__ out) {
  const int c = blockIdx.x * MOM_THREADS + threadIdx.x;
  if (c >= ncol) return;
  const double* p = in + c;
  double sum = 0;
  for (int b0 = 0; b0 < nblocks; b0 += MOM_AHEAD) {
    double v[MOM_AHEAD];
#pragma unroll
    for (int j = 0; j < MOM_AHEAD; ++j) v[j] = b0 + j < nblocks ? p[(size_t)(b0 + j) * ncol] : 0.0;
#pragma unroll
    for (int j = 0; j < MOM_AHEAD; ++j)
      if (b0 + j < nblocks) sum += v[j];
  }
  const double q = sum / denom;
  if (tri_nfeat > 0) {
    int i, j;
    moments_pair(tri_nfeat, c, &i, &j);
    out[(size_t)i * tri_nfeat + j] = q;
    out[(size_t)j * tri_nfeat + i] = q;
  } else out[c] = q;
}

}  // namespace ptm
