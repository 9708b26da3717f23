// The facade's quantile_estimator and its quantile file writer and reader (ptmcmc_gpu.hh) on data piped to them: no engine, no
// device.  Checked against the Python twin (tests/quantiles_model.py) by tests/test_quantiles_model_cpu.py.
//   quantiles_fx estimate      stdin: "n nseries nfeat nrows nq", nq probabilities, then n lines of nseries * nfeat values (series s,
//                              feature f at s * nfeat + f).  stdout: "count N", per probability "q ...", "lo ...", "hi ..." (%.17g)
//   quantiles_fx write <file>  stdin: "dim count replicas rows nq", nq probabilities, dim names, nq * dim values ([k * dim + f]):
//                              write_quantiles
//   quantiles_fx read <file>   read_quantiles: stdout "head dim count replicas rows", "probs ...", "names ...", per probability
//                              "q ..." (%.17g); a refusal exits with status 1
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
  int n = 0, ns = 0, nf = 0, nrows = 0, nq = 0;
  if (scanf("%d %d %d %d %d", &n, &ns, &nf, &nrows, &nq) != 5 || n < 1 || ns < 1 || nf < 1 || nrows < 1 || nrows > n || nq < 1) return 2;
  std::vector<double> probs((size_t)nq);
  for (size_t i = 0; i < probs.size(); i++)
    if (scanf("%lf", &probs[i]) != 1) return 2;
  std::vector<double> x((size_t)n * ns * nf);
  for (size_t i = 0; i < x.size(); i++)
    if (scanf("%lf", &x[i]) != 1) return 2;
  // a plain series: row t is saved row t, the newest is n - 1 (first_row 0, one row per step)
  std::vector<long long> newest((size_t)ns, rhat_estimator::newest_row(n, 1, 0));
  const quantile_estimator::result r = quantile_estimator::estimate(ns, nf, nrows, newest.data(), [&](int s, long long row, std::vector<double>& v) {
    if (row < 0 || row >= n) return false;
    const double* at = x.data() + ((size_t)row * ns + s) * nf;
    v.assign(at, at + nf);
    return true;
  }, probs);
  if (!r.complete) return 3;
  printf("count %lld\n", r.count);
  for (int k = 0; k < nq; k++) {
    line("q", r.q.data() + (size_t)k * nf, (size_t)nf);
    line("lo", r.x_lo.data() + (size_t)k * nf, (size_t)nf);
    line("hi", r.x_hi.data() + (size_t)k * nf, (size_t)nf);
  }
  return 0;
}

static int write_file(const char* file) {
  int dim = 0, replicas = 0, rows = 0, nq = 0;
  long long count = 0;
  if (scanf("%d %lld %d %d %d", &dim, &count, &replicas, &rows, &nq) != 5 || dim < 1 || nq < 1) return 2;
  quantile_estimator::result r;
  r.nfeat = dim; r.count = count; r.complete = true;
  r.probs.resize((size_t)nq);
  for (size_t i = 0; i < r.probs.size(); i++)
    if (scanf("%lf", &r.probs[i]) != 1) return 2;
  std::vector<std::string> names;
  char name[256];
  for (int i = 0; i < dim; i++) {
    if (scanf("%255s", name) != 1) return 2;
    names.push_back(name);
  }
  r.q.resize((size_t)nq * dim);
  for (size_t i = 0; i < r.q.size(); i++)
    if (scanf("%lf", &r.q[i]) != 1) return 2;
  write_quantiles(file, r, replicas, rows, names);
  return 0;
}

static int read_file(const char* file) {
  const quantiles_data d = read_quantiles(file);
  printf("head %d %lld %d %d\n", d.dim, d.count, d.replicas, d.rows);
  line("probs", d.probs.data(), d.probs.size());
  printf("names");
  for (size_t i = 0; i < d.names.size(); i++) printf(" %s", d.names[i].c_str());
  printf("\n");
  for (size_t k = 0; k < d.probs.size(); k++) line("q", d.q.data() + k * (size_t)d.dim, (size_t)d.dim);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "estimate")) return estimate();
  if (argc == 3 && !strcmp(argv[1], "write")) return write_file(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "read")) return read_file(argv[2]);
  return 2;
}
