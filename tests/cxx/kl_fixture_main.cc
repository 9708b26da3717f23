// The facade's kl_estimator and kl_verdict (ptmcmc_gpu.hh) on data piped to them: no engine, no device.  Checked against the recorded
// answers of the real reference (tests/golden/kl_divergence.json.gz) and the Python twin (tests/kl_model.py) by
// tests/test_kl_model_cpu.py.  The first word chooses:
//   "sets ncases", then per case "dim nP nQ", dim lines "wrapped xmin xmax", nP * dim and nQ * dim coordinates
//       -> per case "kl <value>", "fkl <value>", "r <distances within P ...>", "s <distances to Q ...>" (%.17g)
//   "verdict name ncyc ntry transformed transformedX alt altX", then ntry redraw values
//       -> "verdict <Ncut> <cut_frac> <cut> <pass>" (%.17g), then the printed lines
#include <cstdio>
#include <cstring>
#include <vector>

#include "ptmcmc_gpu.hh"
using namespace ptmgpu;

static bool read_values(std::vector<double>& v) {
  for (size_t i = 0; i < v.size(); i++)
    if (scanf("%lf", &v[i]) != 1) return false;
  return true;
}

int main() {
  char mode[32];
  if (scanf("%31s", mode) != 1) return 2;
  if (!strcmp(mode, "verdict")) {
    char name[32];
    double ncyc = 0, t = 0, tX = 0, alt = 0, altX = 0;
    int ntry = 0;
    if (scanf("%31s %lf %d %lf %lf %lf %lf", name, &ncyc, &ntry, &t, &tX, &alt, &altX) != 7 || ntry < 1) return 2;
    std::vector<double> diffs((size_t)ntry);
    if (!read_values(diffs)) return 2;
    const kl_verdict v(diffs, alt);
    printf("verdict %d %.17g %.17g %d\n", v.Ncut, v.cut_frac, v.cut, v.pass ? 1 : 0);
    fputs(v.lines(name, t, tX, alt, altX, ncyc).c_str(), stdout);
    return 0;
  }
  if (strcmp(mode, "sets")) return 2;
  int ncases = 0;
  if (scanf("%d", &ncases) != 1) return 2;
  for (int c = 0; c < ncases; c++) {
    int dim = 0, nP = 0, nQ = 0;
    if (scanf("%d %d %d", &dim, &nP, &nQ) != 3 || dim < 1 || nP < 1 || nQ < 1) return 2;
    stateSpace space(dim);
    for (int d = 0; d < dim; d++) {
      int wrapped = 0;
      double xmin = 0, xmax = 0;
      if (scanf("%d %lf %lf", &wrapped, &xmin, &xmax) != 3) return 2;
      if (wrapped) space.set_bound(d, boundary(boundary::wrap, boundary::wrap, xmin, xmax));
    }
    std::vector<double> P((size_t)nP * dim), Q((size_t)nQ * dim);
    if (!read_values(P) || !read_values(Q)) return 2;
    const kl_estimator::result r = kl_estimator::kl(P.data(), nP, Q.data(), nQ, dim, &space);
    printf("kl %.17g\n", r.value);
    printf("fkl %.17g\n", kl_estimator::fake_kl(P.data(), nP, Q.data(), nQ, dim));
    printf("r");
    for (double v : r.r1sqs) printf(" %.17g", v);
    printf("\ns");
    for (double v : r.s1sqs) printf(" %.17g", v);
    printf("\n");
  }
  return 0;
}
