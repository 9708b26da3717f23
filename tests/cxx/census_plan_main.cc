// The sweep plan (ptmcmc_amd/csrc/ptm_sweep_plan.hpp) of given facts: reads one SweepFacts per line, its fields in the struct's
// order followed by the environment's two (force_valu, compact_ok), all as integers, and prints the name of the build the plan
// chooses.  tests/test_build_census_cpu.py holds every sweep case of tests/build_census.py to the name it is listed under.
#include <cstdio>

#include "ptm_sweep_plan.hpp"

using namespace ptm;

int main() {
  long long v[21];
  for (;;) {
    int got = 0;
    for (; got < 21; ++got)
      if (scanf("%lld", &v[got]) != 1) break;
    if (got == 0) return 0;
    if (got != 21) { fprintf(stderr, "a line of %d fields (21 wanted)\n", got); return 1; }
    SweepFacts f;
    f.DP = (int)v[0]; f.W = (int)v[1]; f.chains = v[2]; f.nloc = (int)v[3]; f.kind = (int)v[4];
    f.has_bounds = v[5]; f.bounds_box = v[6]; f.all_uniform = v[7]; f.has_mean = v[8]; f.any_oned = v[9];
    f.mix_K = (int)v[10];
    f.evolving = v[11]; f.tracked = v[12]; f.user_like = v[13]; f.host_prop = v[14]; f.de = v[15]; f.ada = v[16];
    f.mode = (int)v[17]; f.touched = v[18];
    const SweepEnv env = {v[19] != 0, v[20] != 0};
    char b[96];
    format_sweep_name(plan_sweep(f, env), b, sizeof b);
    printf("%s\n", b);
  }
}
