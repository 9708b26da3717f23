// The facade's proposal factor of a covariance (ptmcmc_gpu.hh: gaussian_prop(covariance) -> eigen_factor, V * diag(sqrt(max(lambda,
// 0))) by its own cyclic Jacobi) and detail::jacobi_eigen's eigenvalues for matrices piped to it: no engine, no device.  Checked
// against the Python twin (tests/prop_adapt_model.py) by tests/test_prop_adapt_model_cpu.py, bit for bit.
//   stdin: "n_mat", then per matrix "n" and n * n hex doubles, row-major.  stdout per matrix: "F ..." and "lambda ..." (%a).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptmcmc_gpu.hh"

int main() {
  int n_mat = 0;
  if (scanf("%d", &n_mat) != 1 || n_mat < 1) return 2;
  for (int m = 0; m < n_mat; m++) {
    int n = 0;
    if (scanf("%d", &n) != 1 || n < 1) return 2;
    std::vector<double> cov((size_t)n * n);
    char word[64];
    for (auto& v : cov) {
      if (scanf("%63s", word) != 1) return 2;
      v = strtod(word, nullptr);
    }
    ptmgpu::gaussian_prop gp(cov, n);
    int kind = -1;
    double odf = -1;
    std::vector<double> f, lam, V;
    if (!gp.device_describe(n, kind, f, odf) || kind != PTM_PROP_DENSE || (int)f.size() != n * n) return 3;
    ptmgpu::detail::jacobi_eigen(cov, n, lam, V);
    printf("F");
    for (double v : f) printf(" %a", v);
    printf("\nlambda");
    for (double v : lam) printf(" %a", v);
    printf("\n");
  }
  return 0;
}
