// The facade's histogram_estimator, its corner file writer and reader and the sampler's corner flags (ptmcmc_gpu.hh) on data piped to
// them: no engine, no device.  Checked against the Python twin (tests/histograms_model.py) by tests/test_histograms_model_cpu.py.
//   histograms_fx estimate      stdin: "n nseries nfeat nrows nbins pairs", nfeat lo, nfeat hi, then n lines of nseries * nfeat values
//                               (series s, feature f at s * nfeat + f).  stdout: "count N", "below ...", "above ...", per feature
//                               "h1 ...", per pair "h2 ..." (integers).  A range that cannot hold the bins: "refused <feature>", status 1
//   histograms_fx edges         stdin: "lo hi nbins": stdout "edges ..." (%.17g) and "ok 0|1"
//   histograms_fx write <file>  stdin: "dim nbins count replicas rows pairs", dim names, dim lo, dim hi, dim below, dim above, dim * nbins
//                               counts, then pairs ? npairs * nbins * nbins counts: write_corner
//   histograms_fx read <file>   read_corner: stdout "head dim nbins count replicas rows pairs", "names ...", "lo ...", "hi ..." (%.17g),
//                               "below ...", "above ...", per feature "h1 ...", per pair "h2 ..."; a refusal exits with status 1
//   histograms_fx flags <bins> <range> <lo> <hi>   the sampler's parsing of --corner_bins and --corner_range, the probabilities of the
//                               axes' ends and the widening of an equal range: stdout "bins n", "range c", "probs a b", "ends lo hi"
//                               (%.17g); a refusal exits with status 1
#include <cstdio>
#include <cstdlib>
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
static void line(const char* tag, const int64_t* v, size_t n) {
  printf("%s", tag);
  for (size_t i = 0; i < n; i++) printf(" %lld", (long long)v[i]);
  printf("\n");
}
static bool numbers(std::vector<double>& v) {
  for (size_t i = 0; i < v.size(); i++)
    if (scanf("%lf", &v[i]) != 1) return false;
  return true;
}
static bool counts(std::vector<int64_t>& v) {
  for (size_t i = 0; i < v.size(); i++) {
    long long c;
    if (scanf("%lld", &c) != 1) return false;
    v[i] = c;
  }
  return true;
}
static void print_counts(const histogram_estimator::result& r) {
  const size_t F = (size_t)r.nfeat, B = (size_t)r.nbins;
  line("below", r.below.data(), F);
  line("above", r.above.data(), F);
  for (size_t f = 0; f < F; f++) line("h1", r.h1.data() + f * B, B);
  for (size_t p = 0; p * B * B < r.h2.size(); p++) line("h2", r.h2.data() + p * B * B, B * B);
}

static int estimate() {
  int n = 0, ns = 0, nf = 0, nrows = 0, nbins = 0, pairs = 0;
  if (scanf("%d %d %d %d %d %d", &n, &ns, &nf, &nrows, &nbins, &pairs) != 6 || n < 1 || ns < 1 || nf < 1 || nrows < 1 || nrows > n || nbins < 1) return 2;
  std::vector<double> lo((size_t)nf), hi((size_t)nf), x((size_t)n * ns * nf);
  if (!numbers(lo) || !numbers(hi) || !numbers(x)) return 2;
  for (int f = 0; f < nf; f++)
    if (!histogram_estimator::edges_ok(lo[(size_t)f], hi[(size_t)f], nbins)) { printf("refused %d\n", f); return 1; }
  // a plain series: row t is saved row t, the newest is n - 1 (first_row 0, one row per step)
  std::vector<long long> newest((size_t)ns, rhat_estimator::newest_row(n, 1, 0));
  const histogram_estimator::result r = histogram_estimator::estimate(ns, nf, nrows, newest.data(), [&](int s, long long row, std::vector<double>& v) {
    if (row < 0 || row >= n) return false;
    const double* at = x.data() + ((size_t)row * ns + s) * nf;
    v.assign(at, at + nf);
    return true;
  }, lo, hi, nbins, pairs != 0);
  if (!r.complete) return 3;
  printf("count %lld\n", r.count);
  print_counts(r);
  return 0;
}

static int edges() {
  double lo = 0, hi = 0;
  int nbins = 0;
  if (scanf("%lf %lf %d", &lo, &hi, &nbins) != 3 || nbins < 1) return 2;
  const std::vector<double> e = histogram_estimator::edges(lo, hi, nbins);
  line("edges", e.data(), e.size());
  printf("ok %d\n", histogram_estimator::edges_ok(lo, hi, nbins) ? 1 : 0);
  return 0;
}

static int write_file(const char* file) {
  int dim = 0, nbins = 0, replicas = 0, rows = 0, pairs = 0;
  long long count = 0;
  if (scanf("%d %d %lld %d %d %d", &dim, &nbins, &count, &replicas, &rows, &pairs) != 6 || dim < 1 || nbins < 1) return 2;
  histogram_estimator::result r;
  r.nfeat = dim; r.nbins = nbins; r.count = count;
  std::vector<std::string> names;
  char name[256];
  for (int i = 0; i < dim; i++) {
    if (scanf("%255s", name) != 1) return 2;
    names.push_back(name);
  }
  const size_t D = (size_t)dim, B = (size_t)nbins;
  r.lo.resize(D); r.hi.resize(D); r.below.resize(D); r.above.resize(D); r.h1.resize(D * B);
  if (pairs) r.h2.resize(histogram_estimator::npairs(dim) * B * B);
  if (!numbers(r.lo) || !numbers(r.hi) || !counts(r.below) || !counts(r.above) || !counts(r.h1) || !counts(r.h2)) return 2;
  write_corner(file, r, replicas, rows, names);
  return 0;
}

static int read_file(const char* file) {
  const corner_data d = read_corner(file);
  printf("head %d %d %lld %d %d %d\n", d.dim, d.nbins, d.count, d.replicas, d.rows, d.hist.h2.empty() ? 0 : 1);
  printf("names");
  for (size_t i = 0; i < d.names.size(); i++) printf(" %s", d.names[i].c_str());
  printf("\n");
  line("lo", d.hist.lo.data(), d.hist.lo.size());
  line("hi", d.hist.hi.data(), d.hist.hi.size());
  print_counts(d.hist);
  return 0;
}

static int flags(char** a) {
  const int bins = ptmcmc_sampler::parse_corner_bins(a[0]);
  const double c = ptmcmc_sampler::parse_corner_range(a[1]);
  const std::vector<double> probs = ptmcmc_sampler::corner_probs(c);
  double lo = atof(a[2]), hi = atof(a[3]);
  ptmcmc_sampler::widen_equal_range(lo, hi);
  printf("bins %d\nrange %.17g\nprobs %.17g %.17g\nends %.17g %.17g\n", bins, c, probs[0], probs[1], lo, hi);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "estimate")) return estimate();
  if (argc == 2 && !strcmp(argv[1], "edges")) return edges();
  if (argc == 3 && !strcmp(argv[1], "write")) return write_file(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "read")) return read_file(argv[2]);
  if (argc == 6 && !strcmp(argv[1], "flags")) return flags(argv + 2);
  return 2;
}
