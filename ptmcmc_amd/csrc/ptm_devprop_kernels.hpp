// ptm_devprop_kernels.hpp -- the device-proposal plug-in (ptm_set_proposal_device): the kernels around the user's batched function.
//
// A sweep on that path is  chunk count -> pack (devlike_count_kernel / devlike_pack_kernel of ptm_devlike_kernels.hpp, gated by the
// exchange phase's touch flags: the chains that make a Metropolis move, stably compacted into natural dimension order) -> ids ->
// the user's work -> unpack -> the sweep kernel(s) with host_prop = 1 -> result (if asked), all queued on the engine's stream: no
// host wait.
//  - devprop_ids_kernel: per row the GLOBAL rung and walker of its chain, and the presets log_hastings = 0, type = 0, valid = 1.
//  - devprop_unpack_kernel<DP>: row k < count goes back into its chain's row of the padded layout (row_pos<DP>), padding zeroed,
//    with its log-Hastings ratio, type and validity by chain: what the lanes kernel's general build reads under host_prop.  One
//    thread per POSITION of the padded row, so a wave's stores are consecutive doubles (the compaction is stable: consecutive rows
//    are chains in ascending order, mostly neighbours).  Chains past the count are not written.
//  - devprop_result_kernel: accepted[k] = (acc_out[chain of row k] == 1) for k < count.
// No scalar-memory stores: every value is written by a plain vector store from the lane that owns it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_kernels.hpp"

namespace ptm {

constexpr int DEVPROP_THREADS = 256;   // threads per workgroup of these kernels (4 waves)

// the dimension that sits at position pos of a padded row: the inverse of row_pos<DP>
template <int DP>
__host__ __device__ constexpr int devprop_dim_at(int pos) {
  return (DP == 32 || DP == 64 || DP == 128) ? (pos & ~7) + 4 * (pos & 1) + ((pos & 7) >> 1) : pos;
}
constexpr int devprop_row_pos_perm(int d) { return 8 * ((d >> 2) >> 1) + 2 * (d & 3) + ((d >> 2) & 1); }   // (row_pos<32 / 64 / 128>, for the check below)
constexpr bool devprop_inverse_ok() {
  for (int d = 0; d < 128; ++d)
    if (devprop_dim_at<128>(devprop_row_pos_perm(d)) != d) return false;
  return true;
}
static_assert(devprop_inverse_ok(), "devprop_dim_at is not the inverse of row_pos");

// grid: ceil(n / DEVPROP_THREADS).  chain c = row_chain[k] is local: rung r0 + c / W, walker walker_begin + c % W (ptm_engine.h)
__global__ __launch_bounds__(DEVPROP_THREADS) void devprop_ids_kernel(int n, int W, int r0, int walker_begin, const int* __restrict__ row_chain,
                                                                int32_t* __restrict__ rung, int32_t* __restrict__ walker,
                                                                double* __restrict__ hast, int32_t* __restrict__ type, int32_t* __restrict__ valid) {
  const int k = blockIdx.x * DEVPROP_THREADS + threadIdx.x;
  if (k >= n) return;
  const int c = row_chain[k];
  const int r = c / W;
  rung[k] = r0 + r;
  walker[k] = walker_begin + (c - r * W);
  hast[k] = 0.0;
  type[k] = 0;
  valid[k] = 1;
}

// grid: ceil(n * DP / DEVPROP_THREADS).  Thread i: position i % DP of row i / DP.
template <int DP>
__global__ __launch_bounds__(DEVPROP_THREADS) void devprop_unpack_kernel(int n, int D, const int32_t* __restrict__ count, const int* __restrict__ row_chain,
                                                                   const double* __restrict__ X, const double* __restrict__ hast,
                                                                   const int32_t* __restrict__ type, const int32_t* __restrict__ valid,
                                                                   double* __restrict__ xprop, double* __restrict__ hastings, int* __restrict__ htype,
                                                                   unsigned char* __restrict__ hvalid) {
  const size_t i = (size_t)blockIdx.x * DEVPROP_THREADS + threadIdx.x;
  const size_t k = i / DP;
  const int pos = (int)(i % DP);
  int cnt = count[0];
  if (cnt > n) cnt = n;
  if (k >= (size_t)cnt) return;
  const int c = row_chain[k];
  const int d = devprop_dim_at<DP>(pos);
  xprop[(size_t)c * DP + pos] = d < D ? X[k * D + d] : 0.0;
  if (pos == 0) {
    hastings[c] = hast[k];
    htype[c] = type[k];
    hvalid[c] = valid[k] != 0 ? (unsigned char)1 : (unsigned char)0;
  }
}

// grid: ceil(n / DEVPROP_THREADS).  acc_out: 1 accepted, 0 rejected (2: no move -- never among the rows below the count)
__global__ __launch_bounds__(DEVPROP_THREADS) void devprop_result_kernel(int n, const int32_t* __restrict__ count, const int* __restrict__ row_chain,
                                                                   const unsigned char* __restrict__ acc_out, int32_t* __restrict__ accepted) {
  const int k = blockIdx.x * DEVPROP_THREADS + threadIdx.x;
  int cnt = count[0];
  if (cnt > n) cnt = n;
  if (k >= cnt) return;
  accepted[k] = acc_out[row_chain[k]] == 1 ? 1 : 0;
}

}  // namespace ptm
