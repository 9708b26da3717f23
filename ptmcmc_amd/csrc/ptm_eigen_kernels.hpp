// ptm_eigen_kernels.hpp -- the Gaussian proposal factor of a batch of covariance matrices (ptm_eigen_factors, ptm_adapt_proposals):
// the facade's gaussian_prop::eigen_factor (ptmcmc_amd/host/ptmcmc_gpu.hh) restated for the device -- detail::jacobi_eigen as it is
// written there, its swap sort of the diagonal, then F[i][j] = V[i][j] * sqrt(max(lambda_j, 0)).  The reference's counterpart is
// user_gaussian_prop::reset_dist (proposal_distribution.cc:340-403), which hands a new covariance to Eigen's solver on the host.
//
//  - eigen_factor_kernel: one matrix a workgroup.  The matrix A lies in LDS, rows padded to an odd length (eigen_ld) so that a walk
//    down a column meets every bank once.  The accumulated rotations are kept transposed, QT[p][k] = Q[k][p]: the host's loop over the
//    rows k of columns p, q of Q is then a walk along rows p, q of QT, and lane k only ever touches column k of QT.  Up to
//    EIG_Q_LDS_N_MAX (64) dimensions QT lies in LDS behind A; above that A alone takes up to 129 KiB of the CU's 160 KiB and QT lies
//    in a workspace in global memory, where lane k's loads and stores are coalesced and stay in the L2.
//    A rotation (p, q) is decided by every lane from A[p][p], A[q][q], A[p][q] (the same three loads, the same bits), then lane k
//    does element k of the column loop and of the loop over Q, a barrier, element k of the row loop (which reads what the column
//    loop wrote at k = p, q), a barrier.  A third barrier stands between the decision's loads and the column loop's stores.
//    The sum of the squared off-diagonals at the head of a sweep and the sort at the end are lane 0's sequential work in the host's
//    order.  One wave serves up to 64 dimensions, two waves up to 128.
//  - eigen_status_kernel: 1 where an entry of the matrix is not finite, else 2 where the smallest eigenvalue is not above 0, else 0.
//  - diag_factor_kernel: the same rule and scale * sqrt(var_d) for the diagonal kind.
// Roots are dsqrt (correctly rounded), quotients plain divisions, multiply then add (-ffp-contract=off): the answers carry the host's
// bits.  Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ptm_device_math.hpp"

namespace ptm {

constexpr int EIG_N_MAX = 128;         // the covariance limit of ptm_moments
constexpr int EIG_SWEEPS_MAX = 100;    // jacobi_eigen's sweep limit
constexpr int EIG_Q_LDS_N_MAX = 64;    // up to here the rotations' matrix lies in LDS beside A
constexpr int EIG_STATUS_THREADS = 64;

__host__ __device__ inline int eigen_ld(int n) { return n | 1; }                    // a row of A in LDS, in doubles
__host__ __device__ inline int eigen_threads(int n) { return n <= 64 ? 64 : 128; }  // one lane for every k of a rotation's loops
__host__ __device__ inline bool eigen_q_in_lds(int n) { return n <= EIG_Q_LDS_N_MAX; }
// dynamic LDS of a workgroup: A, QT where it fits, the stop flag and the sort's order
__host__ __device__ inline size_t eigen_lds_bytes(int n) {
  return (size_t)n * eigen_ld(n) * 8 * (eigen_q_in_lds(n) ? 2 : 1) + (size_t)(n + 2) * 4;
}

// grid: the matrices; eigen_threads(n) lanes; eigen_lds_bytes(n) of dynamic LDS.  qt_ws: [n_mat][n * n], used when !QLDS.
// factors[m][i * n + j] = scale * (V[i][j] * sqrt(max(lambda_j, 0))) (scale 1.0 changes no bit); lambda, sweeps may be null.
template <bool QLDS>
__global__ __launch_bounds__(128) void eigen_factor_kernel(const double* __restrict__ cov, int n, double scale, double* __restrict__ qt_ws,
                                                           double* __restrict__ factors, double* __restrict__ lambda, int32_t* __restrict__ sweeps) {
  extern __shared__ __attribute__((aligned(16))) double eig_lds[];
  const int m = (int)blockIdx.x, tid = (int)threadIdx.x, nt = (int)blockDim.x, ld = eigen_ld(n), nn = n * n;
  double* A = eig_lds;
  double* QT = QLDS ? A + n * ld : qt_ws + (size_t)m * nn;
  const int qld = QLDS ? ld : n;
  int* ctl = (int*)(A + (size_t)n * ld * (QLDS ? 2 : 1));   // [0]: the sweep's stop flag; [1 + j]: the sort's order
  const double* C = cov + (size_t)m * nn;
  for (int e = tid; e < nn; e += nt) {
    const int i = e / n, j = e - i * n;
    A[i * ld + j] = C[e];
    QT[i * qld + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  int sweep = 0;
  for (; sweep < EIG_SWEEPS_MAX; ++sweep) {
    if (tid == 0) {
      double off = 0;
      for (int p = 0; p < n; ++p)
        for (int q = p + 1; q < n; ++q) off += A[p * ld + q] * A[p * ld + q];
      ctl[0] = off < 1e-300 ? 1 : 0;
    }
    __syncthreads();
    const int stop = ctl[0];
    __syncthreads();
    if (stop) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * ld + q], app = A[p * ld + p], aqq = A[q * ld + q];
        __syncthreads();   // every lane holds the three before the column loop overwrites them
        const bool rotate = !(__builtin_fabs(apq) < 1e-300);   // (the same for every lane)
        double c = 1.0, sn = 0.0;
        if (rotate) {
          const double theta = (aqq - app) / (2 * apq);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + dsqrt(theta * theta + 1));
          c = 1 / dsqrt(t * t + 1);
          sn = t * c;
          if (tid < n) {
            const int k = tid;
            { const double a = A[k * ld + p], b = A[k * ld + q]; A[k * ld + p] = c * a - sn * b; A[k * ld + q] = sn * a + c * b; }
            { const double a = QT[p * qld + k], b = QT[q * qld + k]; QT[p * qld + k] = c * a - sn * b; QT[q * qld + k] = sn * a + c * b; }
          }
        }
        __syncthreads();   // the row loop reads what the column loop wrote at k = p, q
        if (rotate && tid < n) {
          const int k = tid;
          const double a = A[p * ld + k], b = A[q * ld + k];
          A[p * ld + k] = c * a - sn * b;
          A[q * ld + k] = sn * a + c * b;
        }
        __syncthreads();
      }
  }
  if (tid == 0) {
    int* order = ctl + 1;
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j)
        if (A[order[j] * ld + order[j]] < A[order[i] * ld + order[i]]) { const int o = order[i]; order[i] = order[j]; order[j] = o; }
    if (sweeps) sweeps[m] = sweep;
  }
  __syncthreads();   // (also makes every lane's column of a QT in global memory visible to the workgroup)
  const int* order = ctl + 1;
  double* F = factors + (size_t)m * nn;
  for (int e = tid; e < nn; e += nt) {
    const int i = e / n, j = e - i * n, o = order[j];
    const double lam = A[o * ld + o];
    const double sg = dsqrt(lam > 0 ? lam : 0.0);
    F[e] = scale * (QT[o * qld + i] * sg);
    if (lambda && i == 0) lambda[(size_t)m * n + j] = lam;
  }
}

// status[m]: 1: an entry of cov[m] is not finite; else 2: lambda[m][0], the smallest eigenvalue, is not above 0; else 0.  grid: the matrices.
__global__ __launch_bounds__(EIG_STATUS_THREADS) void eigen_status_kernel(const double* __restrict__ cov, const double* __restrict__ lambda, int n,
                                                                          int32_t* __restrict__ status) {
  const int m = (int)blockIdx.x, tid = (int)threadIdx.x, nn = n * n;
  const double* C = cov + (size_t)m * nn;
  int bad = 0;
  for (int e = tid; e < nn; e += EIG_STATUS_THREADS) {
    const double v = C[e];
    if (!(__builtin_fabs(v) < __builtin_inf())) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) status[m] = bad ? 1 : (lambda[(size_t)m * n] > 0 ? 0 : 2);
}

// the diagonal kind: sigma[m][d] = scale * sqrt(var[m][d]); status[m]: 1: a variance is not finite; else 2: a variance is not above
// 0; else 0.  grid: the rungs.
__global__ __launch_bounds__(EIG_STATUS_THREADS) void diag_factor_kernel(const double* __restrict__ var, int n, double scale, double* __restrict__ sigma,
                                                                         int32_t* __restrict__ status) {
  const int m = (int)blockIdx.x, tid = (int)threadIdx.x;
  int inf = 0, low = 0;
  for (int d = tid; d < n; d += EIG_STATUS_THREADS) {
    const double v = var[(size_t)m * n + d];
    if (!(__builtin_fabs(v) < __builtin_inf())) inf = 1;
    else if (!(v > 0)) low = 1;
    sigma[(size_t)m * n + d] = scale * dsqrt(v);
  }
  inf = __syncthreads_or(inf);
  low = __syncthreads_or(low);
  if (tid == 0) status[m] = inf ? 1 : (low ? 2 : 0);
}

}  // namespace ptm
