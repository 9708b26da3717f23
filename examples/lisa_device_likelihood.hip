// lisa_device_likelihood.hip -- the toy LISA likelihood of the reference's exampleLISA (antenna responses exampleLISA.cc:59-72,
// log-likelihood :130-142; tests/lisa_toy.py is its numpy form) as a HIP kernel for gfx950, with an extern "C" launcher of the
// ptm_loglike_device_fn shape (include/ptm_engine.h): hand it to ptm_set_target_device (C), Engine.set_target_device_c (Python) or
// call it from a device_likelihood's evaluate_log_device (examples/example_lisa_device.cc).
// Every row is evaluated (a fixed shape: rows past *count are in-support states), one lane per row; complex arithmetic in pairs of
// doubles.  Parameters per row: d, phi, inc, lambda, beta, psi.
//   build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared -ffp-contract=off -Iinclude examples/lisa_device_likelihood.hip -o liblisa_device.so
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ptm_engine.h"

namespace {
constexpr double FACTOR = 216147.866077;
constexpr double SA_RE = 0.33687296665053773, SA_IM = 0.087978055005482114;
constexpr double SE_RE = -0.12737105239204741, SE_IM = 0.21820079314765678;

// m22 + m2m2 of modes() with plus = (pr, pi), cross = (cr, ci)
__device__ void modes(double d, double phi, double inc, double psi, double pr, double pi, double cr, double ci, double& re, double& im) {
  const double pref = 0.5 / d * sqrt(5 / M_PI);
  const double c = cos(inc / 2), s = sin(inc / 2);
  const double a22 = pref * (c * c * c * c), a2m2 = pref * (s * s * s * s);
  const double t1 = 2 * (-phi - psi), t2 = 2 * (-phi + psi);
  // 0.5 * (plus + i cross), 0.5 * (plus - i cross)
  const double u_re = 0.5 * (pr - ci), u_im = 0.5 * (pi + cr);
  const double v_re = 0.5 * (pr + ci), v_im = 0.5 * (pi - cr);
  const double e1r = cos(t1), e1i = sin(t1), e2r = cos(t2), e2i = sin(t2);
  re = a22 * (e1r * u_re - e1i * u_im) + a2m2 * (e2r * v_re - e2i * v_im);
  im = a22 * (e1r * u_im + e1i * u_re) + a2m2 * (e2r * v_im + e2i * v_re);
}

__global__ __launch_bounds__(256) void lisa_loglike_kernel(int n, int dim, const double* __restrict__ X, double* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double* x = X + (size_t)k * dim;
  const double d = x[0], phi = x[1], inc = x[2], lam = x[3], beta = x[4], psi = x[5];
  const double g = 0.75 * (3 - cos(2 * beta));
  const double ap = g * cos(2 * lam - M_PI / 3), ac = 3.0 * sin(beta) * sin(2 * lam - M_PI / 3);    // a_plus = i ap, a_cross = i ac
  const double ep = -(g * sin(2 * lam - M_PI / 3)), ec = 3.0 * sin(beta) * cos(2 * lam - M_PI / 3);  // e_plus = i ep, e_cross = i ec
  double sar, sai, ser, sei;
  modes(d, phi, inc, psi, 0.0, ap, 0.0, ac, sar, sai);
  modes(d, phi, inc, psi, 0.0, ep, 0.0, ec, ser, sei);
  const double ar = sar - SA_RE, ai = sai - SA_IM, er = ser - SE_RE, ei = sei - SE_IM;
  out[k] = -0.5 * FACTOR * ((ar * ar + ai * ai) + (er * er + ei * ei));
}
}  // namespace

// ptm_loglike_device_fn: enqueue on the engine's stream and return
extern "C" void lisa_loglike_device(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                    double* out_llike_dev) {
  (void)user; (void)count_dev;
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(lisa_loglike_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_rows, dim, X_dev, out_llike_dev);
}
