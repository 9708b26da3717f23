// The sweep kernel's choice (ptmcmc_amd/csrc/ptm_sweep_plan.hpp) over the cross product of the facts it depends on: prints every
// distinct kernel name the plan can produce (tests/test_sweep_plan_cpu.py holds each to a kernel that was built) and checks what the
// launch, the engine's preparations and the reported name rely on.  Exit status 1 and a line per broken property on stderr.
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <set>
#include <string>
#include <unordered_set>

#include "ptm_sweep_plan.hpp"

using namespace ptm;

static int failures = 0;
static void check(bool ok, const char* what, const SweepFacts& f, const SweepEnv& env, const char* name) {
  if (ok || ++failures > 20) return;
  fprintf(stderr, "BROKEN: %s -- %s (DP %d W %d chains %lld nloc %d kind %d bounds %d box %d uniform %d mean %d oned %d mix %d evolving %d tracked %d "
                  "user_like %d host_prop %d de %d ada %d mode %d touched %d force_valu %d compact_ok %d)\n",
          what, name, f.DP, f.W, f.chains, f.nloc, f.kind, f.has_bounds, f.bounds_box, f.all_uniform, f.has_mean, f.any_oned, f.mix_K, f.evolving, f.tracked,
          f.user_like, f.host_prop, f.de, f.ada, f.mode, f.touched, env.force_valu, env.compact_ok);
}
// every field of a plan, packed: two plans are the same build iff their keys are equal
static uint64_t key_of(const SweepPlan& s) {
  return (uint64_t)s.family | (uint64_t)s.DP << 3 | (uint64_t)s.kind << 14 | (uint64_t)s.uni << 16 | (uint64_t)s.simple << 17 | (uint64_t)s.ada << 18 | (uint64_t)s.gen << 19 |
         (uint64_t)s.hist << 20 | (uint64_t)s.mgen << 21 | (uint64_t)s.ev << 23 | (uint64_t)s.bnd << 24 | (uint64_t)s.compacted << 25;
}
static std::set<std::string> names;
static void note(const SweepPlan& s, char* b, size_t n, const SweepFacts& f, const SweepEnv& env) {
  static std::unordered_set<uint64_t> seen;
  b[0] = 0;
  if (!seen.insert(key_of(s)).second) return;
  const int len = format_sweep_name(s, b, n);
  check(len > 0 && len < (int)n, "the name fits its buffer", f, env, b);
  names.insert(b);
}
static bool mfma(const SweepPlan& s) { return s.family == FAM_MFMA32 || s.family == FAM_MFMA64 || s.family == FAM_MFMA128; }

int main() {
  const int DPs[] = {4, 8, 16, 32, 64, 128, 256, 512, 1024}, Ws[] = {1, 4, 63, 64, 320, 1024};
  const int kinds[] = {PLAN_DENSE, PLAN_DIAG, PLAN_LOWER};
  const int NB = 13;   // boolean facts
  for (int DP : DPs)
    for (int W : Ws) {
      // chain counts on both sides of every threshold of the lanes kernel's rule
      const long long edges[] = {4096ll, 4096ll * DP, (1ll << 20) / DP, (1ll << 19) / DP, (1ll << 21) / DP};
      for (long long edge : edges)
        for (long long chains : {edge, edge + 1})
          for (int kind : kinds)
            for (int mix_K : {0, 2})
              for (int envbits = 0; envbits < 4; ++envbits)
                for (int bits = 0; bits < (1 << NB); ++bits) {
                  const SweepEnv env = {(envbits & 1) != 0, (envbits & 2) != 0};
                  SweepFacts f;
                  memset(&f, 0, sizeof f);
                  f.DP = DP; f.W = W; f.chains = chains; f.kind = kind; f.mix_K = mix_K;
                  f.nloc = (bits & 1) ? 4097 : (int)((chains + W - 1) / W < 4096 ? (chains + W - 1) / W : 4096);
                  f.has_bounds = bits & 2; f.bounds_box = bits & 4; f.all_uniform = bits & 8; f.has_mean = bits & 16; f.any_oned = bits & 32;
                  f.evolving = bits & 64; f.tracked = bits & 128; f.user_like = bits & 256; f.host_prop = bits & 512; f.de = bits & 1024; f.ada = bits & 2048;
                  f.mode = (bits & 4096) ? 1 : 0;
                  if (f.mode && !f.user_like) continue;   // (the propose / accept passes exist around a user likelihood only)
                  f.touched = true;
                  const SweepPlan s = plan_sweep(f, env);
                  char b[96];   // (the name of a build's first appearance; empty afterwards)
                  note(s, b, sizeof b, f, env);
                  check(!s.compacted || (s.family == FAM_MFMA32 && f.touched && f.W >= 1024 && f.nloc <= 4096 && !f.tracked),
                        "compacted: the 32-D matrix-core kernel after an exchange phase, W >= 1024, at most 4096 local rungs, no history", f, env, b);
                  check(!env.force_valu || (!mfma(s) && !s.compacted), "PTM_FORCE_VALU: no matrix-core kernel, nothing compacted", f, env, b);
                  check(env.compact_ok || !s.compacted, "PTM_COMPACT=0: nothing compacted", f, env, b);
                  check(!f.host_prop || s.family == FAM_LANES, "host-side proposals: the lanes kernel", f, env, b);
                  check(!(f.ada && !f.host_prop) || s.family == FAM_LANES_ADA || (s.family == FAM_GENERAL && s.ada), "an adaptive set: the two adaptive builds only", f, env, b);
                  check(f.DP <= 32 || s.family != FAM_GENERAL, "the general kernel is built up to 32 dimensions", f, env, b);
                  // a plain sweep (no exchange phase before it) runs the same build but for the compaction -- and, with it, the build of
                  // bounds and nothing else (3), which exists compacted only, in place of the box-bounds build (1)
                  f.touched = false;
                  SweepPlan u = plan_sweep(f, env);
                  note(u, b, sizeof b, f, env);
                  check(!u.compacted, "an untouched sweep is not compacted", f, env, b);
                  u.compacted = s.compacted;
                  if (s.family == FAM_MFMA32 && s.mgen == 3 && u.mgen == 1) u.mgen = 3;
                  check(key_of(u) == key_of(s), "touched changes nothing but the compaction", f, env, b);
                }
    }
  for (const std::string& n : names) printf("%s\n", n.c_str());
  if (failures) fprintf(stderr, "%d broken properties\n", failures);
  return failures ? 1 : 0;
}
