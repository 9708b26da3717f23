// scripted_device_proposal.hip -- a user proposal drawn ON THE DEVICE (ptm_set_proposal_device): a HIP kernel for gfx950 with an
// extern "C" launcher of the ptm_propose_device_fn shape and a result launcher of the ptm_proposal_result_device_fn shape
// (include/ptm_engine.h).  Hand them to ptm_set_proposal_device (C), Engine.set_proposal_device_c (Python) or call them from a
// device_proposal's draw_device / result_device (tests/cxx/device_proposal_main.cc).
// The proposal is the device twin of scripted_proposal in tests/test_gpu_host_proposals.py: deterministic in (rung, walker, step),
// its uniforms the splitmix64 finaliser of (rung, walker, step, column); a jump of the rung's scale per dimension, now and then far
// out of any prior's support, log-Hastings ratios of either sign, zero and NaN, type codes 0..4 and invalid states.  It uses the
// same double operations in the same order as the numpy form; built with -ffp-contract=off every one is an exactly rounded +, * or
// conversion, so host and device twins agree bit for bit.
//   build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared -ffp-contract=off -Iinclude examples/scripted_device_proposal.hip -o libscripted_proposal.so
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ptm_engine.h"

// what `user` points to (host memory; the pointers in it are device pointers)
struct scripted_proposal_user {
  const double* scale_dev;     // [n_rungs] the jump scale of each GLOBAL rung
  int32_t* accepted_out_dev;   // the result launcher copies the outcomes [n_rows] here, ...
  int32_t* rung_out_dev;       // ... the rows' rungs and walkers [n_rows] ...
  int32_t* walker_out_dev;
  int32_t* count_out_dev;      // ... and the count [1]; each may be NULL
  uint64_t calls, result_calls;   // how often each launcher has run (host side)
  uint64_t last_step[4];          // the step of propose call number i at [i % 4]
};

namespace {
__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // the splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// u in [0, 1) of column col (0-based) for the chain whose base is `base`
__device__ __forceinline__ double uniform_of(uint64_t base, int col) {
  const uint64_t z = mix64(base + (uint64_t)(col + 1) * 0xD6E8FEB86659FD93ull);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// one thread per (row, dimension); the thread of dimension 0 also writes the row's ratio, type and validity.  Every row is
// computed (a fixed shape: rows past *count hold real states and ids, and their outputs are never read).
__global__ __launch_bounds__(256) void scripted_proposal_kernel(int n, int dim, const double* __restrict__ X, const int32_t* __restrict__ rung,
                                                              const int32_t* __restrict__ walker, uint64_t step, const double* __restrict__ scale,
                                                              double* __restrict__ P, double* __restrict__ H, int32_t* __restrict__ T,
                                                              int32_t* __restrict__ V) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * dim) return;
  const size_t k = i / dim;
  const int d = (int)(i - k * dim);
  const int r = rung[k];
  const uint64_t base = (uint64_t)r * 0x9E3779B97F4A7C15ull + (uint64_t)walker[k] * 0xC2B2AE3D27D4EB4Full + step * 0x165667B19E3779F9ull;
  const double u = uniform_of(base, d);
  double p = X[i] + scale[r] * (2 * u - 1);
  if (uniform_of(base, dim) < 0.04) p = p * 40.0 + 7.0;   // now and then far out of the prior's support
  P[i] = p;
  if (d == 0) {
    const double u1 = uniform_of(base, dim + 1), u2 = uniform_of(base, dim + 2), u3 = uniform_of(base, dim + 3);
    double h = 1.6 * (u1 - 0.5);                          // a log-Hastings ratio of either sign ...
    if (u2 < 0.05) h = 0.0;
    if (u2 > 0.97) h = __builtin_nan("");                 // ... and the reference's NaN rule (chain.cc:990-993)
    H[k] = h;
    T[k] = (int32_t)(u3 * 5);                             // proposal_distribution::type()
    V[k] = u3 > 0.03 ? 1 : 0;                             // state::invalid()
  }
}
}  // namespace

// ptm_propose_device_fn: enqueue on the engine's stream and return
extern "C" void scripted_propose_device(void* user, void* stream, int n_rows, int dim, const double* X_cur_dev, const int32_t* rung_dev,
                                        const int32_t* walker_dev, const int32_t* count_dev, uint64_t step, double* X_prop_dev,
                                        double* log_hastings_dev, int32_t* type_dev, int32_t* valid_dev) {
  (void)count_dev;
  scripted_proposal_user* u = (scripted_proposal_user*)user;
  u->last_step[u->calls % 4] = step;
  u->calls += 1;
  if (n_rows <= 0 || dim <= 0) return;
  const size_t tot = (size_t)n_rows * dim;
  hipLaunchKernelGGL(scripted_proposal_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_rows, dim, X_cur_dev,
                     rung_dev, walker_dev, step, u->scale_dev, X_prop_dev, log_hastings_dev, type_dev, valid_dev);
}

// ptm_proposal_result_device_fn: keep the outcomes (and whose they are) where the caller can fetch them after ptm_sync
extern "C" void scripted_result_device(void* user, void* stream, int n_rows, const int32_t* rung_dev, const int32_t* walker_dev,
                                       const int32_t* count_dev, const int32_t* accepted_dev) {
  scripted_proposal_user* u = (scripted_proposal_user*)user;
  u->result_calls += 1;
  hipStream_t s = (hipStream_t)stream;
  const size_t b = (size_t)(n_rows > 0 ? n_rows : 0) * sizeof(int32_t);
  if (u->accepted_out_dev && b) (void)hipMemcpyAsync(u->accepted_out_dev, accepted_dev, b, hipMemcpyDeviceToDevice, s);
  if (u->rung_out_dev && b) (void)hipMemcpyAsync(u->rung_out_dev, rung_dev, b, hipMemcpyDeviceToDevice, s);
  if (u->walker_out_dev && b) (void)hipMemcpyAsync(u->walker_out_dev, walker_dev, b, hipMemcpyDeviceToDevice, s);
  if (u->count_out_dev) (void)hipMemcpyAsync(u->count_out_dev, count_dev, sizeof(int32_t), hipMemcpyDeviceToDevice, s);
}
