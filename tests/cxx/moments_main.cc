// The facade's moments_estimator and its covariance file reader and writer (ptmcmc_gpu.hh) on data piped to them: no engine, no
// device.  Checked against the Python twin (tests/moments_model.py) by tests/test_moments_model_cpu.py.
//   moments_fx estimate      stdin: "n nseries nfeat nrows want_cov", then n lines of nseries * nfeat values (series s, feature f at
//                            s * nfeat + f).  stdout: "count N", "mean ...", "var ...", per row "cov ...", per series "walker ..." (%.17g)
//   moments_fx write <file>  stdin: "dim count replicas rows", dim names, dim means, dim * dim matrix values: write_covariance
//   moments_fx read <file> <dim>   read_covariance: stdout "mean ...", per row "cov ..." (%.17g); a refusal exits with status 1
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

static void line(const char* tag, const double* v, size_t n) {
  printf("%s", tag);
  for (size_t i = 0; i < n; i++) printf(" %.17g", v[i]);
  printf("\n");
}

static int estimate() {
  int n = 0, ns = 0, nf = 0, nrows = 0, want_cov = 1;
  if (scanf("%d %d %d %d %d", &n, &ns, &nf, &nrows, &want_cov) != 5 || n < 1 || ns < 1 || nf < 1 || nrows < 1 || nrows > n) return 2;
  std::vector<double> x((size_t)n * ns * nf);
  for (size_t i = 0; i < x.size(); i++)
    if (scanf("%lf", &x[i]) != 1) return 2;
  // a plain series: row t is saved row t, the newest is n - 1 (first_row 0, one row per step)
  std::vector<long long> newest((size_t)ns, rhat_estimator::newest_row(n, 1, 0));
  const moments_estimator::result r = moments_estimator::estimate(ns, nf, nrows, newest.data(), [&](int s, long long row, std::vector<double>& v) {
    if (row < 0 || row >= n) return false;
    const double* at = x.data() + ((size_t)row * ns + s) * nf;
    v.assign(at, at + nf);
    return true;
  }, want_cov != 0);
  if (!r.complete) return 3;
  printf("count %lld\n", r.count);
  line("mean", r.mean.data(), r.mean.size());
  line("var", r.var.data(), r.var.size());
  for (size_t i = 0; i * nf < r.cov.size(); i++) line("cov", r.cov.data() + i * nf, (size_t)nf);
  for (int s = 0; s < ns; s++) line("walker", r.walker_sum.data() + (size_t)s * nf, (size_t)nf);
  return 0;
}

static int write_file(const char* file) {
  int dim = 0, replicas = 0, rows = 0;
  long long count = 0;
  if (scanf("%d %lld %d %d", &dim, &count, &replicas, &rows) != 4 || dim < 1) return 2;
  std::vector<std::string> names;
  char name[256];
  for (int i = 0; i < dim; i++) {
    if (scanf("%255s", name) != 1) return 2;
    names.push_back(name);
  }
  std::vector<double> mean((size_t)dim), cov((size_t)dim * dim);
  for (size_t i = 0; i < mean.size(); i++)
    if (scanf("%lf", &mean[i]) != 1) return 2;
  for (size_t i = 0; i < cov.size(); i++)
    if (scanf("%lf", &cov[i]) != 1) return 2;
  write_covariance(file, mean, cov, count, replicas, rows, names);
  return 0;
}

static int read_file(const char* file, int dim) {
  const covariance_data c = read_covariance(file, dim);
  line("mean", c.mean.data(), c.mean.size());
  for (int i = 0; i < dim; i++) line("cov", c.cov.data() + (size_t)i * dim, (size_t)dim);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "estimate")) return estimate();
  if (argc == 3 && !strcmp(argv[1], "write")) return write_file(argv[2]);
  if (argc == 4 && !strcmp(argv[1], "read")) return read_file(argv[2], atoi(argv[3]));
  return 2;
}
