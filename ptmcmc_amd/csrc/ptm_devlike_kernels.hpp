// ptm_devlike_kernels.hpp -- the device-likelihood plug-in (ptm_set_target_device): the kernels around the user's batched function.
//
// A step on that path is  exchange kernel -> propose pass (mode 1) -> chunk count -> pack -> the user's work -> scatter -> accept
// pass (mode 2), all queued on the engine's stream: no host wait.
//  - devlike_count_kernel: per chunk of DL_CHUNK chains, how many are selected (gate & gmask) == gval (propose pass: bit 1, the
//    proposals that passed enforce, the prior and the prior gate -- what the host path hands its callback).
//  - devlike_pack_kernel<DP>: a STABLE compaction.  Row k < count is the k-th selected chain in local-chain order, gathered from the
//    padded row layout (row_pos<DP>) into natural dimension order; rows count.. hold the other chains' current states (or, where
//    there are none to trust, a copy of row 0) so that every row is a real in-support state.  Inside a wave the ranks come from a
//    ballot and mbcnt, across waves from four totals in LDS, across chunks from one scan of the chunk totals.  Also writes *count
//    and the row -> chain index.
//  - devlike_scatter_kernel: out[k] -> dst[chain[k]] for k < count, and, fused, the best log-posterior lprior + llike over those
//    rows with its state (bayes_likelihood::bestPost / bestState): ties to the lowest row (= chain), NaN never wins, a step's best
//    replaces the kept one only if strictly greater (ties to the earliest step).  One workgroup: the reduction needs no second pass.
// No scalar-memory stores: the kept best is written by plain vector stores from one lane.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_kernels.hpp"

namespace ptm {

constexpr int DL_CHUNK = 256;          // chains per workgroup of the count / pack kernels (4 waves, one chain per lane)
constexpr int DL_SCATTER_THREADS = 1024;

__device__ __forceinline__ bool dl_selected(const unsigned char* gate, int gmask, int gval, int c) {
  return gate ? ((int)gate[c] & gmask) == gval : true;
}

__global__ __launch_bounds__(DL_CHUNK) void devlike_count_kernel(int n, const unsigned char* __restrict__ gate, int gmask, int gval,
                                                                int* __restrict__ chunk_tot) {
  __shared__ int wtot[DL_CHUNK / 64];
  const int c = blockIdx.x * DL_CHUNK + threadIdx.x;
  const bool sel = c < n && dl_selected(gate, gmask, gval, c);
  const uint64_t m = __builtin_amdgcn_ballot_w64(sel);
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = __builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < DL_CHUNK / 64; ++w) s += wtot[w];
    chunk_tot[blockIdx.x] = s;
  }
}

// grid: one workgroup per chunk.  xsel: rows of the selected chains [n][DP]; xrest: rows of the others (nullptr: copy row 0 instead,
// which exists whenever count > 0 -- the set-up calls, whose unselected chains hold no state yet)
template <int DP>
__global__ __launch_bounds__(DL_CHUNK) void devlike_pack_kernel(int n, int D, int nchunk, const unsigned char* __restrict__ gate, int gmask,
                                                               int gval, const int* __restrict__ chunk_tot, const double* __restrict__ xsel,
                                                               const double* __restrict__ xrest, double* __restrict__ X,
                                                               int* __restrict__ row_chain, int32_t* __restrict__ count) {
  __shared__ int red[2][DL_CHUNK / 64];
  __shared__ int wtot[DL_CHUNK / 64];
  __shared__ int s_src[DL_CHUNK], s_row[DL_CHUNK];
  __shared__ int s_total, s_before;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // the scan of the chunk totals: this chunk's offset and the grand total
  int before = 0, total = 0;
  for (int j = threadIdx.x; j < nchunk; j += DL_CHUNK) {
    const int t = chunk_tot[j];
    total += t;
    if (j < (int)blockIdx.x) before += t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o, 64); total += __shfl_xor(total, o, 64); }
  if (lane == 0) { red[0][wv] = before; red[1][wv] = total; }
  // ranks inside the chunk
  const int c = blockIdx.x * DL_CHUNK + threadIdx.x;
  const bool live = c < n;
  const bool sel = live && dl_selected(gate, gmask, gval, c);
  const uint64_t m = __builtin_amdgcn_ballot_w64(sel);
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (lane == 0) wtot[wv] = __builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0, t = 0;
#pragma unroll
    for (int w = 0; w < DL_CHUNK / 64; ++w) { b += red[0][w]; t += red[1][w]; }
    s_before = b; s_total = t;
    if (blockIdx.x == 0) count[0] = t;
  }
  __syncthreads();
  int wbefore = 0;
  for (int w = 0; w < wv; ++w) wbefore += wtot[w];
  const int gsel_before = s_before + wbefore + rank;   // selected chains in front of c
  int row = -1;
  if (live) row = sel ? gsel_before : s_total + (c - gsel_before);
  s_src[threadIdx.x] = sel ? 1 : 0;
  s_row[threadIdx.x] = row;
  if (live) row_chain[row] = c;
  __syncthreads();
  // the rows: natural dimension order out of the padded layout, D consecutive doubles per row
  const int c0 = blockIdx.x * DL_CHUNK;
  const int nr = min(DL_CHUNK, n - c0);
  for (int i = threadIdx.x; i < nr * D; i += DL_CHUNK) {
    const int r = i / D, d = i - r * D, cc = c0 + r;
    const int pos = row_pos<DP>(d);
    double v;
    if (s_src[r]) v = xsel[(size_t)cc * DP + pos];
    else if (xrest) v = xrest[(size_t)cc * DP + pos];
    else v = __builtin_nan("");   // (filled below from row 0)
    X[(size_t)s_row[r] * D + d] = v;
  }
}

// the set-up calls' rows past the count: copies of row 0 (a drawn, in-support state)
__global__ __launch_bounds__(256) void devlike_fill_kernel(int n, int D, const int32_t* __restrict__ count, double* __restrict__ X) {
  const int k0 = count[0];
  if (k0 <= 0) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t first = (size_t)k0 * D, end = (size_t)n * D;
  if (first + i < end) X[first + i] = X[i % (size_t)D];
}

// one workgroup.  dst[chain[k]] = out[k] for k < count.  gate_out (set-up redraw loop): llike < -1e100 -> gate 0 (draw again),
// else gate 2 (done).  best (nullptr: off) = {lpost, x[D]}: the kept best, replaced by this batch's if strictly greater.
__global__ __launch_bounds__(DL_SCATTER_THREADS) void devlike_scatter_kernel(int D, const int32_t* __restrict__ count, const int* __restrict__ row_chain,
                                                                            const double* __restrict__ out, double* __restrict__ dst,
                                                                            unsigned char* __restrict__ gate_out, const double* __restrict__ lprior,
                                                                            const double* __restrict__ X, double* __restrict__ best) {
  __shared__ double s_v[DL_SCATTER_THREADS / 64];
  __shared__ int s_k[DL_SCATTER_THREADS / 64];
  __shared__ int s_win;
  const int n = count[0];
  double bv = -__builtin_inf();
  int bk = 0x7fffffff;
  for (int k = threadIdx.x; k < n; k += DL_SCATTER_THREADS) {
    const int c = row_chain[k];
    const double v = out[k];
    if (gate_out) {
      if (v < -1e100) gate_out[c] = 0;   // chain.cc:858: (slike = evaluate_log(s)) < -1e100 => redraw
      else { gate_out[c] = 2; dst[c] = v; }
    } else {
      dst[c] = v;
    }
    if (best) {
      const double post = lprior[c] + v;
      if (post > bv || (post == bv && k < bk)) { bv = post; bk = k; }   // (a NaN compares false both ways: never taken)
    }
  }
  if (!best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int ok = __shfl_xor(bk, o, 64);
    if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
  }
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = bv; s_k[threadIdx.x >> 6] = bk; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < DL_SCATTER_THREADS / 64; ++w)
      if (s_v[w] > bv || (s_v[w] == bv && s_k[w] < bk)) { bv = s_v[w]; bk = s_k[w]; }
    const bool win = bk < n && bv > best[0];
    s_win = win ? bk : -1;
    if (win) best[0] = bv;
  }
  __syncthreads();
  const int w = s_win;
  if (w >= 0)
    for (int d = threadIdx.x; d < D; d += DL_SCATTER_THREADS) best[1 + d] = X[(size_t)w * D + d];
}

}  // namespace ptm
