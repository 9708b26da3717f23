// de_mfma_applies (ptmcmc_amd/csrc/ptm_sweep_plan.hpp) over the cross product of facts that tests/cxx/sweep_plan_main.cc walks, with the
// two facts and the switch it added: when differential evolution goes to the matrix cores (de_mfma32_kernel) in place of the plan's
// kernel.  The conditions are restated here one by one, from the kernel's own limits, and held against the predicate; the plan itself
// must not see the new fields.  Exit status 1 and a line per broken property on stderr; prints the number of facts that were eligible
// under each value of the switch.
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <initializer_list>

#include "ptm_sweep_plan.hpp"

using namespace ptm;

static int failures = 0;
static void check(bool ok, const char* what, const SweepFacts& f, const SweepEnv& env) {
  if (ok || ++failures > 20) return;
  fprintf(stderr, "BROKEN: %s (DP %d W %d chains %lld kind %d bounds %d box %d uniform %d mix %d evolving %d tracked %d user_like %d host_prop %d de %d ada %d "
                  "mode %d prior_draw %d history %d force_valu %d de_mfma %d)\n",
          what, f.DP, f.W, f.chains, f.kind, f.has_bounds, f.bounds_box, f.all_uniform, f.mix_K, f.evolving, f.tracked, f.user_like, f.host_prop, f.de, f.ada,
          f.mode, f.prior_draw, f.history, env.force_valu, env.de_mfma);
}
static uint64_t key_of(const SweepPlan& s) {
  return (uint64_t)s.family | (uint64_t)s.DP << 3 | (uint64_t)s.kind << 14 | (uint64_t)s.uni << 16 | (uint64_t)s.simple << 17 | (uint64_t)s.ada << 18 | (uint64_t)s.gen << 19 |
         (uint64_t)s.hist << 20 | (uint64_t)s.mgen << 21 | (uint64_t)s.ev << 23 | (uint64_t)s.bnd << 24 | (uint64_t)s.compacted << 25 | (uint64_t)s.prefilter << 26;
}

int main() {
  const int DPs[] = {4, 8, 16, 32, 64, 128, 256, 512, 1024}, Ws[] = {1, 4, 63, 64, 320, 1024};
  const int kinds[] = {PLAN_DENSE, PLAN_DIAG, PLAN_LOWER};
  const int NB = 14;   // boolean facts
  long long eligible[3] = {0, 0, 0};
  for (int DP : DPs)
    for (int W : Ws) {
      const long long edges[] = {4096ll, 4096ll * DP, (1ll << 20) / DP, (1ll << 19) / DP, (1ll << 21) / DP};
      for (long long edge : edges)
        for (long long chains : {edge, edge + 1})
          for (int kind : kinds)
            for (int mix_K : {0, 2})
              for (int envbits = 0; envbits < 4; ++envbits)
                for (int bits = 0; bits < (1 << NB); ++bits) {
                  SweepFacts f;
                  memset(&f, 0, sizeof f);
                  f.DP = DP; f.W = W; f.chains = chains; f.kind = kind; f.mix_K = mix_K;
                  f.nloc = (int)((chains + W - 1) / W < 4096 ? (chains + W - 1) / W : 4096);
                  f.has_bounds = bits & 2; f.bounds_box = bits & 4; f.all_uniform = bits & 8; f.has_mean = bits & 16; f.any_oned = bits & 32;
                  f.evolving = bits & 64; f.tracked = bits & 128; f.user_like = bits & 256; f.host_prop = bits & 512; f.de = bits & 1024; f.ada = bits & 2048;
                  f.mode = (bits & 4096) ? 1 : 0;
                  if (f.mode && !f.user_like) continue;   // (the propose / accept passes exist around a user likelihood only)
                  f.prior_draw = bits & 1; f.history = bits & 8192;
                  if (f.history && !f.tracked) continue;  // (a history ring is tracking)
                  f.touched = true;
                  // the kernel's limits, one by one
                  const bool shape = f.DP == 32 && f.W % 64 == 0 && f.mode == 0;
                  const bool device = !f.user_like && !f.host_prop && !f.ada;
                  const bool set = f.de && !f.prior_draw && f.mix_K > 0;
                  const bool box = f.all_uniform && (!f.has_bounds || f.bounds_box);
                  const bool may = shape && device && set && box && f.history;
                  const bool big = f.chains * f.DP > (1ll << 21);
                  SweepFacts g = f;
                  g.prior_draw = false; g.history = false;
                  for (int sw = -1; sw <= 1; ++sw) {
                    const SweepEnv env = {(envbits & 1) != 0, (envbits & 2) != 0, 0, 0, sw};
                    const bool a = de_mfma_applies(f, env);
                    if (a) eligible[sw + 1] += 1;
                    check(!a || may, "the predicate holds only where every eligibility condition does", f, env);
                    check(!a || !env.force_valu, "PTM_FORCE_VALU keeps everything off the matrix cores", f, env);
                    check(sw >= 0 || !a, "PTM_DE_MFMA=0: never", f, env);
                    check(sw != 1 || a == (may && !env.force_valu), "PTM_DE_MFMA=1: every eligible population", f, env);
                    check(sw != 0 || a == (may && !env.force_valu && big), "unset: chains x DP > 2^21", f, env);
                    const SweepPlan s = plan_sweep(f, env);
                    check(sw != 0 || !a || s.family == FAM_GENERAL, "unset: the kernel takes over from the general kernel only", f, env);
                    check(!a || (s.family != FAM_MFMA32 && !s.compacted && !reads_ladder_major_beta(s)),
                          "the plan beside it prepares a sweep that is not compacted and reads the chain-indexed temperatures", f, env);
                    // the plan does not see the new fields, nor the switch
                    const SweepEnv old = {(envbits & 1) != 0, (envbits & 2) != 0};
                    check(key_of(plan_sweep(g, old)) == key_of(s), "plan_sweep does not depend on the new fields", f, env);
                  }
                }
    }
  printf("eligible off=%lld unset=%lld on=%lld\n", eligible[0], eligible[1], eligible[2]);
  if (failures) fprintf(stderr, "%d broken properties\n", failures);
  return failures ? 1 : 0;
}
