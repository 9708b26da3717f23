// The real reference's proposal-test statistics on sample sets piped to it: the program behind tests/golden/kl_divergence.json.gz
// (run by tests/golden/make_kl_fixture.py, by hand, where the reference is mounted; no test builds or runs it).  It includes the
// reference's test_proposal.hh where it lies and links the objects under oracle/_ref/obj: nothing of the reference is copied.
//   stdin:  "ncases", then per case "dim nP nQ", dim lines "wrapped xmin xmax", nP * dim and nQ * dim coordinates
//   stdout: per case "kl <KL_divergence(P, Q, false)>", "fkl <fake_KL_divergence(P, Q)>", "r <all_nnd2(P) ...>",
//           "s <one_nnd2(P[i], Q) ...>" (%.17g)
#include <cstdio>
#include <valarray>
#include <vector>

#include "test_proposal.hh"

static std::vector<state> read_set(const stateSpace* space, int n, int dim) {
  std::vector<state> out;
  for (int i = 0; i < n; i++) {
    std::valarray<double> x(0.0, dim);
    for (int d = 0; d < dim; d++)
      if (scanf("%lf", &x[d]) != 1) exit(2);
    state s(space, x);
    for (int d = 0; d < dim; d++)
      if (s.get_param(d) != x[d] || s.invalid()) { fprintf(stderr, "a point is changed by the space's enforcement\n"); exit(3); }
    out.push_back(s);
  }
  return out;
}

int main() {
  int ncases = 0;
  if (scanf("%d", &ncases) != 1) return 2;
  ProbabilityDist::setSeed(0.5);   // (a chain, a member of test_proposal, asks the global generator for its seed; nothing here draws)
  test_proposal tp;
  for (int c = 0; c < ncases; c++) {
    int dim = 0, nP = 0, nQ = 0;
    if (scanf("%d %d %d", &dim, &nP, &nQ) != 3) return 2;
    stateSpace space(dim);
    for (int d = 0; d < dim; d++) {
      int wrapped = 0;
      double xmin = 0, xmax = 0;
      if (scanf("%d %lf %lf", &wrapped, &xmin, &xmax) != 3) return 2;
      if (wrapped) space.set_bound(d, boundary(boundary::wrap, boundary::wrap, xmin, xmax));
    }
    std::vector<state> P = read_set(&space, nP, dim), Q = read_set(&space, nQ, dim);
    printf("kl %.17g\n", tp.KL_divergence(P, Q, false));
    printf("fkl %.17g\n", tp.fake_KL_divergence(P, Q));
    std::vector<double> r = tp.all_nnd2(P);
    printf("r");
    for (double v : r) printf(" %.17g", v);
    printf("\ns");
    for (int i = 0; i < nP; i++) printf(" %.17g", tp.one_nnd2(P[i], Q));
    printf("\n");
  }
  return 0;
}
