// The host route's eigen leg for tools/prop_adapt_probe.py: the facade's gaussian_prop::eigen_factor over a batch of covariances, with
// the status rule and the scale of parallel_tempering_chains::adapt_gaussian_proposals.  Built by the probe:
//   g++ -std=c++11 -O2 -ffp-contract=off -shared -fPIC -I include -I ptmcmc_amd/host tools/prop_adapt_host_eigen.cc -o <dir>/libhost_eigen.so
#include <cmath>
#include <vector>

#include "ptmcmc_gpu.hh"

extern "C" void host_eigen_factors(const double* cov, int n_mat, int n, double scale, double* factors, int* status) {
  const size_t nn = (size_t)n * n;
  for (int m = 0; m < n_mat; m++) {
    std::vector<double> A(cov + m * nn, cov + (m + 1) * nn), F, lam;
    bool finite = true;
    for (size_t k = 0; k < nn; k++) finite = finite && std::isfinite(A[k]);
    ptmgpu::gaussian_prop::eigen_factor(A, n, F, &lam);
    for (size_t k = 0; k < nn; k++) factors[m * nn + k] = scale * F[k];
    status[m] = !finite ? 1 : (lam[0] > 0 ? 0 : 2);
  }
}
