// The horizon's arithmetic (ptmcmc_amd/csrc/ptm_count_limit.hpp) without a GPU: the refusal rule at its edges, re-basing, ptm_restore's
// range check, and no signed overflow in the bound itself (build with -fsanitize=undefined,address -fno-sanitize-recover: an overflow
// ends the program).  Exit status 1 and a line per broken property on stderr; prints the number of checks made.
#include <climits>
#include <cstdio>
#include <vector>

#include "ptm_count_limit.hpp"

using namespace ptm;

static int failures = 0, checks = 0;
#define CHECK(ok) do { ++checks; if (!(ok)) { ++failures; fprintf(stderr, "BROKEN (line %d): %s\n", __LINE__, #ok); } } while (0)

// the rule as the issue states it, restated with a wider type: refused iff max + A n > limit
static bool rule(long long max_count, long long n) { return n > 0 && (__int128)max_count + (__int128)2 * n > (__int128)2147483647; }

int main() {
  const int64_t L = PTM_COUNT_MAX, A = PTM_ADDS_PER_STEP;
  CHECK(L == 2147483647ll && L == (int64_t)INT_MAX);
  CHECK(A == 2);

  // the exact rule at the edges: a true maximum at limit - A n passes, one more is refused
  for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)63, (int64_t)64, (int64_t)1024, (int64_t)1 << 24, ((int64_t)1 << 24) + 1, ((int64_t)1 << 30) - 1}) {
    for (int64_t off = -3; off <= 3; ++off) {
      const int64_t m = L - A * n + off;
      if (m < 0) continue;
      CHECK(count_exceeds(m, n) == (off > 0));
      CHECK(count_exceeds(m, n) == rule(m, n));
      CountHorizon h;
      h.rebase(m);
      const bool ok = h.admit(n);
      CHECK(ok == (off <= 0));
      CHECK(h.bound == (ok ? m + A * n : m));          // a refusal books nothing
      if (ok) CHECK(h.bound <= L);
    }
  }
  // n <= 0 asks for nothing and books nothing, wherever the bound stands
  for (int64_t m : {(int64_t)0, (int64_t)1, L - 1, L, L + 1, (int64_t)0xFFFFFFFFll}) {
    CountHorizon h;
    h.rebase(m);
    CHECK(h.admit(0) && h.admit(-1) && h.admit(INT_MIN) && h.bound == m);
    CHECK(h.admit(1) == (m + A <= L));
  }
  // every n, small maxima: against the wide restatement
  for (int64_t m = L - 40; m <= L + 2; ++m)
    for (int64_t n = -1; n <= 24; ++n) CHECK(count_exceeds(m, n) == rule(m, n));

  // no signed overflow in the bound at n = INT_MAX, from the smallest and from the largest bound there can be (ptm_restore refuses what
  // is past the limit; the device's unsigned Nhist could read 2^32 - 1 on a build without that check)
  for (int64_t m : {(int64_t)0, (int64_t)1, L, (int64_t)0xFFFFFFFFll}) {
    CountHorizon h;
    h.rebase(m);
    CHECK(!h.admit(INT_MAX) && h.bound == m);
    CHECK(count_exceeds(m, INT_MAX) && count_exceeds(m, INT64_C(1) << 31));
  }

  // a fresh engine: Ntries = 1.  The bound is an upper bound of the true maximum as long as every step adds at most A
  {
    CountHorizon h;
    CHECK(h.bound == 1);
    int64_t truth = 1, steps = 0;
    // walk by calls of 2^24 steps whose chains add ONE per step (plain sweeps): the bound runs ahead of the truth, trips early,
    // is re-based, and the calls go on until the rule itself refuses
    int rebases = 0;
    for (;;) {
      const int64_t n = (int64_t)1 << 24;
      if (!h.admit(n)) {
        CHECK(h.bound >= truth);
        h.rebase(truth); ++rebases;
        if (!h.admit(n)) { CHECK(rule(truth, n)); break; }
      }
      CHECK(!rule(truth, n));
      truth += n; steps += n;
      CHECK(h.bound >= truth && truth <= L);
    }
    CHECK(rebases >= 2);                       // (the bound tripped before the rule did, and re-basing let the run go on)
    CHECK(truth + A * ((int64_t)1 << 24) > L);  // it went as far as the rule allows
    // the rest in single steps: to limit - 1 or limit - 2 exactly, never past
    while (true) {
      if (!h.admit(1)) { h.rebase(truth); if (!h.admit(1)) break; }
      truth += 1;
    }
    CHECK(truth == L - 1 && rule(truth, 1));
  }

  // re-basing to a maximum read from the arrays: signed Ntries, unsigned Nhist
  {
    std::vector<int32_t> nt = {1, 5, INT_MAX - 7, 0};
    std::vector<uint32_t> nh = {0u, 9u, 3u, (uint32_t)INT_MAX - 5u};
    CHECK(count_true_max(nt.data(), nh.data(), nt.size()) == L - 5);
    nh[1] = 0xFFFFFFF0u;   // (an Nhist past the limit reads as what it is, not as a negative number)
    CHECK(count_true_max(nt.data(), nh.data(), nt.size()) == (int64_t)0xFFFFFFF0ll);
    CHECK(count_true_max(nt.data(), nh.data(), 0) == 0);
  }

  // ptm_restore's check
  CHECK(count_restore_error(1, 1, 0) == nullptr);
  CHECK(count_restore_error(0, 0, 0) == nullptr);
  CHECK(count_restore_error(L, L, L) == nullptr);
  CHECK(count_restore_error(L, 0, L) == nullptr);
  CHECK(count_restore_error(5, 6, 0) != nullptr);
  CHECK(count_restore_error(-1, -1, 0) != nullptr);
  CHECK(count_restore_error(3, -1, 0) != nullptr);
  CHECK(count_restore_error(3, 1, -1) != nullptr);
  CHECK(count_restore_error(3, 1, L + 1) != nullptr);
  CHECK(count_restore_error(3, 1, 0xFFFFFFFFll) != nullptr);
  CHECK(count_restore_error(L + 1, 1, 0) != nullptr);
  CHECK(count_restore_error(INT64_MIN, 0, 0) != nullptr && count_restore_error(0, 0, INT64_MAX) != nullptr);

  printf("checks=%d\n", checks);
  if (failures) fprintf(stderr, "%d broken properties\n", failures);
  return failures ? 1 : 0;
}
