// The prior gate (ptmcmc_amd/csrc/ptm_devprior_kernels.hpp: prior_gate) without a GPU: the one function the host-prior path and the
// device-prior kernel both call, against a literal restatement of the rule over a table of edge values (build with
// -fsanitize=address,undefined -ffp-contract=off).  Exit status 1 and a line per broken case on stderr; prints the number of checks.
#include <cmath>
#include <cstdio>
#include <limits>

#include "ptm_devprior_kernels.hpp"

static int failures = 0, checks = 0;

// the rule as stated: every operation rounded on its own (volatile: no contraction, no reassociation, whatever the flags)
static int rule(double nl, double lprior, double llike, double beta, double min_prior) {
  volatile double bl = beta * llike;
  volatile double cur_lpost = lprior + bl;
  volatile double oldlprior = cur_lpost - bl;
  volatile double diff = nl - oldlprior;
  const bool want = nl > -1e200 || diff > min_prior;
  return 1 | (want ? 2 : 0);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double nls[] = {-inf, -1e200, std::nextafter(-1e200, 0.0), -1e3, 0.0, inf, nan};
  const double lps[] = {-inf, -5.0, 0.0};
  // beta * llike: 0, a huge negative one, and 1e17, against which an lprior of -5 is lost (cur_lpost - bl rounds to 0 or -16)
  const struct { double beta, llike; } bls[] = {{1.0, 0.0}, {0.0, -3.0}, {1.0, -1e308}, {0.5, -1.6e308}, {1.0, 1e17}, {0.25, 4e17}};
  const double mps[] = {-30.0, -inf};
  for (double nl : nls)
    for (double lp : lps)
      for (const auto& b : bls)
        for (double mp : mps) {
          const int got = ptm::prior_gate(nl, lp, b.llike, b.beta, mp), want = rule(nl, lp, b.llike, b.beta, mp);
          ++checks;
          if (got != want) {
            ++failures;
            fprintf(stderr, "BROKEN: nl %g lprior %g beta %g llike %g min_prior %g: gate %d, the rule says %d\n", nl, lp, b.beta, b.llike, mp, got, want);
          }
          ++checks;
          if ((got & 1) != 1 || (got & ~3) != 0) { ++failures; fprintf(stderr, "BROKEN: gate byte %d\n", got); }
        }
  // pinned outcomes, worked by hand
  struct { double nl, lp, ll, beta, mp; int gate; } pins[] = {
      {0.0, -5.0, 0.0, 1.0, -30.0, 3},                       // inside the support: wanted
      {-1e200, -5.0, 0.0, 1.0, -30.0, 1},                    // -1e200 is not above -1e200, and -1e200 + 5 is far below min_prior
      {std::nextafter(-1e200, 0.0), -5.0, 0.0, 1.0, -30.0, 3},   // the next double above it is
      {-inf, -5.0, 0.0, 1.0, -30.0, 1},                      // outside the support
      {-inf, -inf, 0.0, 1.0, -30.0, 1},                      // -inf - -inf = NaN: no comparison holds
      {-inf, -5.0, 0.0, 1.0, -inf, 1},                       // -inf > -inf does not hold
      {-1e3, -5.0, 0.0, 1.0, -inf, 3},
      {-1e201, -inf, 0.0, 1.0, -30.0, 3},                    // nl - (-inf) = +inf > min_prior: wanted though far below -1e200
      {-1e201, -5.0, 0.0, 1.0, -30.0, 1},
      {-1e201, -5.0, 1e17, 1.0, -30.0, 1},
      {nan, 0.0, 0.0, 1.0, -30.0, 1},                        // a NaN prior: valid, not wanted
      {inf, 0.0, 0.0, 1.0, -30.0, 3},
  };
  for (const auto& p : pins) {
    const int got = ptm::prior_gate(p.nl, p.lp, p.ll, p.beta, p.mp);
    ++checks;
    if (got != p.gate) { ++failures; fprintf(stderr, "BROKEN pin: nl %g lprior %g llike %g: gate %d, expected %d\n", p.nl, p.lp, p.ll, got, p.gate); }
  }
  // the rounding case really rounds: (-5 + 1e17) - 1e17 is not -5
  {
    volatile double bl = 1e17, s = -5.0 + bl, o = s - bl;
    ++checks;
    if (o == -5.0) { ++failures; fprintf(stderr, "BROKEN: the table's rounding case does not round\n"); }
  }
  printf("checks=%d\n", checks);
  return failures ? 1 : 0;
}
