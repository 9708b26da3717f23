// The box pre-pass's host-side decisions (ptmcmc_amd/csrc/ptm_sweep_plan.hpp) without a GPU: which sweeps are eligible for it
// (SweepPlan::prefilter) and which rungs the estimate flags (prefilter_flag).  Exit status 1 and a line per broken property on stderr.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "ptm_sweep_plan.hpp"

using namespace ptm;

static int failures = 0;
static void check(bool ok, const char* what) {
  if (!ok) { ++failures; fprintf(stderr, "BROKEN: %s\n", what); }
}
// the benchmark's sweep after an exchange phase: 32 dimensions, all-uniform prior, open bounds, a Cholesky factor, 1024+ walkers
static SweepFacts bench_facts() {
  SweepFacts f;
  memset(&f, 0, sizeof f);
  f.DP = 32; f.W = 1024; f.nloc = 12; f.chains = 12 * 1024; f.kind = PLAN_LOWER; f.all_uniform = true; f.touched = true;
  return f;
}

int main() {
  const SweepEnv autoenv = {false, true, 0}, forced = {false, true, 1}, off = {false, true, -1}, nocompact = {false, false, 1}, valu = {true, true, 1};
  SweepFacts f = bench_facts();
  check(plan_sweep(f, autoenv).prefilter && plan_sweep(f, forced).prefilter, "lower-triangular factor, lean compacted build: eligible");
  check(!plan_sweep(f, off).prefilter, "PTM_BOX_PREFILTER=0: never");
  check(!plan_sweep(f, nocompact).prefilter && !plan_sweep(f, valu).prefilter, "no compacted matrix-core sweep, no pre-pass");
  f.kind = PLAN_DIAG;
  check(plan_sweep(f, autoenv).prefilter, "a diagonal factor is a lower-triangular one");
  f.kind = PLAN_DENSE;
  check(!plan_sweep(f, forced).prefilter, "a dense factor reaches every row from every column");
  f = bench_facts(); f.touched = false;
  check(!plan_sweep(f, forced).prefilter, "a sweep without an exchange phase before it is not compacted");
  f = bench_facts(); f.has_bounds = true; f.bounds_box = true;
  check(plan_sweep(f, forced).compacted && !plan_sweep(f, forced).prefilter, "box bounds: another build (mgen 3)");
  f = bench_facts(); f.all_uniform = false;
  check(!plan_sweep(f, forced).prefilter, "a prior that is not all-uniform has no box");
  f = bench_facts(); f.has_mean = true;
  check(!plan_sweep(f, forced).prefilter, "a mean: the general build");
  f = bench_facts(); f.any_oned = true;
  check(!plan_sweep(f, forced).prefilter, "one-dimensional moves: the general build");
  f = bench_facts(); f.mix_K = 2;
  check(!plan_sweep(f, forced).prefilter, "a scale mixture: the general build");
  f = bench_facts(); f.evolving = true;
  check(plan_sweep(f, forced).compacted && plan_sweep(f, forced).mgen == 0 && !plan_sweep(f, forced).prefilter, "evolving ladders are left out");
  f = bench_facts(); f.tracked = true;
  check(!plan_sweep(f, forced).prefilter, "history or MAP tracking: nothing compacted");
  f = bench_facts(); f.W = 960; f.chains = 12 * 960;
  check(!plan_sweep(f, forced).prefilter, "fewer than 1024 walkers: nothing compacted");
  f = bench_facts(); f.DP = 64;
  check(!plan_sweep(f, forced).prefilter, "64 dimensions: another kernel family");
  {   // the name of the build does not know about the pre-pass
    char a[96], b[96];
    f = bench_facts();
    format_sweep_name(plan_sweep(f, forced), a, sizeof a); format_sweep_name(plan_sweep(f, off), b, sizeof b);
    check(strcmp(a, b) == 0 && strcmp(a, "sweep_mfma32_kernel<2, false, 0, false, true>") == 0, "the kernel's name does not change");
  }

  // ---- the estimate.  One dimension against a Monte-Carlo count, wide and narrow; the narrow limit 0.798 sigma / w
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nz;
  std::uniform_real_distribution<double> un(0.0, 1.0);
  for (double sigma : {0.05, 0.5, 2.0, 20.0}) {
    const int n = 400000;
    int out = 0;
    for (int i = 0; i < n; ++i) { const double y = un(rng) + sigma * nz(rng); out += (y < 0.0 || y > 1.0) ? 1 : 0; }
    const double mc = (double)out / n, ex = prefilter_out_1d(sigma, 1.0);
    // binomial standard error at most 0.5 / sqrt n = 8e-4: five of them
    check(std::fabs(mc - ex) < 4e-3, "the exact one-dimensional share agrees with a Monte-Carlo count");
  }
  check(std::fabs(prefilter_out_1d(1e-3, 1.0) - 0.7978845608e-3) < 1e-9, "narrow proposals: 0.798 sigma / w");
  check(prefilter_out_1d(0.0, 1.0) == 0.0 && prefilter_out_1d(1.0, INFINITY) == 0.0 && prefilter_out_1d(1.0, 0.0) == 1.0, "degenerate widths");
  // sigmas of a factor's first 16 rows: a lower-triangular factor and a diagonal one
  {
    const int D = 20;
    double T[D * D] = {0}, sg[PREFILTER_DIMS], diag[D];
    for (int i = 0; i < D; ++i) { diag[i] = 0.5 + i; for (int k = 0; k <= i; ++k) T[i * D + k] = (k == i) ? 3.0 : 4.0; }
    prefilter_sigmas(false, T, D, sg);
    check(std::fabs(sg[0] - 3.0) < 1e-14 && std::fabs(sg[1] - 5.0) < 1e-14 && std::fabs(sg[15] - std::sqrt(9.0 + 16.0 * 15)) < 1e-12, "sigma_d^2 = sum_k T[d][k]^2");
    prefilter_sigmas(true, diag, D, sg);
    check(sg[0] == 0.5 && sg[15] == 15.5, "a diagonal factor's sigmas are its entries");
    double few[3] = {1.0, 2.0, 3.0};
    prefilter_sigmas(true, few, 3, sg);
    check(sg[2] == 3.0 && sg[3] == 0.0 && sg[15] == 0.0, "dimensions past D propose nothing");
  }
  // a factor far inside the box is not flagged, one comparable to it is; the switches override the estimate
  {
    double width[PREFILTER_DIMS], narrow[PREFILTER_DIMS], wide[PREFILTER_DIMS];
    for (int d = 0; d < PREFILTER_DIMS; ++d) { width[d] = 200.0; narrow[d] = 1.0; wide[d] = 60.0; }
    const double sn = prefilter_out_share(narrow, width, PREFILTER_DIMS), sw = prefilter_out_share(wide, width, PREFILTER_DIMS);
    check(sn > 0.05 && sn < 0.07, "16 dimensions of sigma = w / 200: 1 - (1 - 0.00399)^16 = 0.062");
    check(sw > 0.97, "16 dimensions of sigma = 0.3 w: nearly every proposal leaves");
    check(!prefilter_flag(narrow, width, PREFILTER_DIMS, 0) && prefilter_flag(wide, width, PREFILTER_DIMS, 0), "the estimate flags the wide rung only");
    check(prefilter_flag(narrow, width, PREFILTER_DIMS, 1) && !prefilter_flag(wide, width, PREFILTER_DIMS, -1), "=1 flags every rung, =0 none");
    check(PTM_PREFILTER_THRESHOLD > 0.0 && PTM_PREFILTER_THRESHOLD < 1.0, "the threshold is a share");
  }
  if (failures) fprintf(stderr, "%d broken properties\n", failures);
  else printf("ok\n");
  return failures ? 1 : 0;
}
