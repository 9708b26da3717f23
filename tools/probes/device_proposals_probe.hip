// device_proposals_probe.hip -- what tools/device_proposals_probe.py needs beside examples/scripted_device_proposal.hip:
//  - probe_propose_host: the scripted proposal as a HOST callback of the ptm_propose_batch_fn shape (the same numbers as the device
//    launcher: build with -ffp-contract=off), for the host-proposal step the device path is measured against;
//  - probe_loglike_device: a diagonal quadratic as a device likelihood (ptm_loglike_device_fn), one lane per row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ptm_engine.h"

namespace {
inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline double uniform_of(uint64_t base, int col) {
  const uint64_t z = mix64(base + (uint64_t)(col + 1) * 0xD6E8FEB86659FD93ull);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
__global__ __launch_bounds__(256) void probe_loglike_kernel(int n, int dim, const double* __restrict__ X, double* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double acc = 0.0;
  for (int d = 0; d < dim; d++) {
    const double t = X[(size_t)k * dim + d] * (0.7 + 0.02 * d);
    acc = acc + t * t;
  }
  out[k] = -0.5 * acc;
}
}  // namespace

// user: const double* scale_of_rung (host memory)
extern "C" void probe_propose_host(void* user, int n, int dim, const double* X_cur, const int32_t* rung, const int32_t* walker, uint64_t step,
                                   double* X_prop, double* log_hastings, int32_t* type, int32_t* valid) {
  const double* scale = (const double*)user;
  for (int k = 0; k < n; k++) {
    const int r = rung[k];
    const uint64_t base = (uint64_t)r * 0x9E3779B97F4A7C15ull + (uint64_t)walker[k] * 0xC2B2AE3D27D4EB4Full + step * 0x165667B19E3779F9ull;
    const bool big = uniform_of(base, dim) < 0.04;
    for (int d = 0; d < dim; d++) {
      double p = X_cur[(size_t)k * dim + d] + scale[r] * (2 * uniform_of(base, d) - 1);
      if (big) p = p * 40.0 + 7.0;
      X_prop[(size_t)k * dim + d] = p;
    }
    const double u1 = uniform_of(base, dim + 1), u2 = uniform_of(base, dim + 2), u3 = uniform_of(base, dim + 3);
    double h = 1.6 * (u1 - 0.5);
    if (u2 < 0.05) h = 0.0;
    if (u2 > 0.97) h = NAN;
    log_hastings[k] = h;
    type[k] = (int32_t)(u3 * 5);
    valid[k] = u3 > 0.03 ? 1 : 0;
  }
}

extern "C" void probe_loglike_device(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                     double* out_llike_dev) {
  (void)user; (void)count_dev;
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(probe_loglike_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_rows, dim, X_dev, out_llike_dev);
}
