// The facade's rhat_estimator (ptmcmc_gpu.hh) on series piped to it: no engine, no device.  Checked against the Python twin
// (tests/rhat_model.py) by tests/test_rhat_model_cpu.py.
//   stdin:  "n nseries nfeat nrows", then n lines of nseries * nfeat values (series s, feature f at s * nfeat + f)
//   stdout: per feature "feature <rhat> <mean> <within> <between>", then per sequence k and feature "sequence <mean> <var>" (%.17g)
#include <cstdio>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

int main() {
  int n = 0, ns = 0, nf = 0, nrows = 0;
  if (scanf("%d %d %d %d", &n, &ns, &nf, &nrows) != 4 || n < 1 || ns < 1 || nf < 1 || nrows < 4 || nrows % 2 || nrows > n) return 2;
  std::vector<double> x((size_t)n * ns * nf);
  for (size_t i = 0; i < x.size(); i++)
    if (scanf("%lf", &x[i]) != 1) return 2;
  // a plain series: row t is saved row t, the newest is n - 1 (first_row 0, one row per step)
  std::vector<long long> newest((size_t)ns, rhat_estimator::newest_row(n, 1, 0));
  const rhat_estimator::result r = rhat_estimator::estimate(ns, nf, nrows, newest.data(), [&](int s, long long row, std::vector<double>& v) {
    if (row < 0 || row >= n) return false;
    const double* at = x.data() + ((size_t)row * ns + s) * nf;
    v.assign(at, at + nf);
    return true;
  });
  if (!r.complete) return 3;
  for (int f = 0; f < nf; f++) printf("feature %.17g %.17g %.17g %.17g\n", r.rhat[f], r.mean[f], r.within[f], r.between[f]);
  for (size_t o = 0; o < r.seq_mean.size(); o++) printf("sequence %.17g %.17g\n", r.seq_mean[o], r.seq_var[o]);
  return 0;
}
