// correlated_prior_device.hip -- a prior ptm_set_prior cannot describe, as a HIP kernel for gfx950 with an extern "C" launcher of the
// ptm_logprior_device_fn shape (include/ptm_engine.h): hand it to ptm_set_prior_device (C), Engine.set_prior_device_c (Python) or call
// it from a device_prior's evaluate_log_prior_device (examples/example_lisa_device_prior.cc).
//
// The prior is the toy-LISA product prior (d, phi, lambda, psi uniform; inc polar; beta co-polar: examples/example_lisa.cc) times a
// correlated Gaussian in distance and inclination, with a hard cut:
//   log p(x) = log sin(inc) + log cos(beta) - 1/2 [u^2 - 2 RHO u v + v^2] / (1 - RHO^2) + LOG_NORM,
//              u = (d - D0) / SD,  v = (inc - I0) / SI;     -inf where d > D_CUT or outside the product prior's box
// One function, correlated_logprior(), serves the kernel and the host form (correlated_logprior_host, the device_prior's evaluate_log).
// It uses + - * / and comparisons ONLY -- the cosine is its Taylor polynomial on [-pi/2, pi/2] (sin(inc) = cos(inc - pi/2)), the
// logarithm a halving / doubling loop and the atanh series; the log-prior is within 1e-11 of the library functions' on draws of the
// product prior -- so that under -ffp-contract=off host and device give the SAME BITS: the device route and the host route
// (PTM_DEVICE_PRIOR=0) then walk the same chains.
// Every row is evaluated (a fixed shape: rows past *count are in-support states), one lane per row.
//   build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared -ffp-contract=off -Iinclude examples/correlated_prior_device.hip -o libcorrelated_prior.so
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptm_engine.h"

namespace {
constexpr double PI = 3.14159265358979323846, HALF_PI = PI / 2;
constexpr double D_LO = 1.667 - 1.333, D_HI = 1.667 + 1.333;   // the product prior's box in d (the angles' boxes are their bounds)
constexpr double D0 = 1.5, SD = 0.6, I0 = 1.2, SI = 0.7, RHO = 0.6, D_CUT = 2.6;
constexpr double LOG_NORM = -7.25;   // the uniform factors' and the Gaussian's constants (a constant shifts no chain)
constexpr double INF = __builtin_huge_val();

// cos(x) for |x| <= pi/2 (a little beyond does no harm): the Taylor polynomial to x^26, Horner in x^2; the first term left out is
// (pi/2)^28 / 28! < 1e-24
__host__ __device__ inline double poly_cos(double x) {
  const double z = x * x;
  double r = 1.0;
#pragma unroll
  for (int k = 13; k >= 1; --k) r = 1.0 - r * z / (double)((2 * k - 1) * (2 * k));
  return r;
}

// log(s) for 0 < s < 2^1000: s = m 2^e with m in [1/sqrt(2), sqrt(2)) by exact doublings / halvings, log m = 2 atanh((m - 1) / (m + 1))
// by its series (|z| < 0.172: thirteen terms reach 1e-20); -inf for s <= 0 (and for a NaN)
__host__ __device__ inline double poly_log(double s) {
  if (!(s > 0.0)) return -INF;
  int e = 0;
  while (s < 0.70710678118654752440 && e > -1100) { s = s * 2.0; --e; }
  while (s >= 1.41421356237309504880 && e < 1100) { s = s * 0.5; ++e; }
  const double z = (s - 1.0) / (s + 1.0), z2 = z * z;
  double r = 0.0;
#pragma unroll
  for (int k = 12; k >= 0; --k) r = r * z2 + 1.0 / (double)(2 * k + 1);
  return 2.0 * z * r + (double)e * 0.69314718055994530942;
}

__host__ __device__ inline double correlated_logprior(const double* x) {
  const double d = x[0], phi = x[1], inc = x[2], lam = x[3], beta = x[4], psi = x[5];
  if (d < D_LO || d > D_HI || d > D_CUT) return -INF;
  if (phi < 0.0 || phi > 2 * PI || lam < 0.0 || lam > 2 * PI || psi < 0.0 || psi > PI) return -INF;
  if (inc < 0.0 || inc > PI || beta < -HALF_PI || beta > HALF_PI) return -INF;
  const double u = (d - D0) / SD, v = (inc - I0) / SI;
  const double q = (u * u - 2.0 * RHO * u * v + v * v) / (1.0 - RHO * RHO);
  return poly_log(poly_cos(inc - HALF_PI)) + poly_log(poly_cos(beta)) - 0.5 * q + LOG_NORM;
}

__global__ __launch_bounds__(256) void correlated_logprior_kernel(int n, int dim, const double* __restrict__ X, double* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  out[k] = correlated_logprior(X + (size_t)k * dim);
}
}  // namespace

// the host form: the same function, compiled for the host
extern "C" double correlated_logprior_host(const double* x) { return correlated_logprior(x); }

// ptm_logprior_device_fn: enqueue on the engine's stream and return
extern "C" void correlated_logprior_device(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                           double* out_lprior_dev) {
  (void)user; (void)count_dev;
  if (n_rows <= 0 || dim < 6) return;
  hipLaunchKernelGGL(correlated_logprior_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_rows, dim, X_dev, out_lprior_dev);
}
