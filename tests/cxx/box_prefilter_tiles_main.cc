// The box pre-pass's tile-to-rung lookup (ptmcmc_amd/csrc/ptm_sweep_plan.hpp: prefilter_slice) without a GPU: on prefix arrays with
// empty rungs at the start, in the middle and at the end every tile below ntiles must map to the rung, tile number, first entry and
// entry count a linear walk over the rungs gives, for each of the four waves; ntiles itself and everything past it is past the end.
// Exit status 1 and a line per broken property on stderr.
#include <cstdio>
#include <random>
#include <vector>

#include "ptm_sweep_plan.hpp"

using namespace ptm;

static int failures = 0;
static void check(bool ok, const char* what, int a = 0, int b = 0) {
  if (!ok) { ++failures; fprintf(stderr, "BROKEN: %s (%d, %d)\n", what, a, b); }
}

// the kernel's prologue: inclusive prefix of ceil(cnt / 256)
static int prefix(const std::vector<int>& cnt, std::vector<int>& tpre) {
  int run = 0;
  tpre.resize(cnt.size());
  for (size_t r = 0; r < cnt.size(); ++r) { run += (cnt[r] + 255) >> 8; tpre[r] = run; }
  return run;
}

static void walk(const std::vector<int>& cnt, const char* name) {
  std::vector<int> tpre;
  const int nrung = (int)cnt.size(), ntiles = prefix(cnt, tpre);
  int tile = 0;
  long long entries = 0, total = 0;
  for (int r = 0; r < nrung; ++r) {
    total += cnt[r];
    for (int kb = 0; kb * 256 < cnt[r]; ++kb, ++tile) {
      for (int wave = 0; wave < 4; ++wave) {
        const PrefilterSlice s = prefilter_slice(tpre.data(), cnt.data(), nrung, ntiles, tile, wave);
        const int start = (kb * 4 + wave) * 64, left = cnt[r] - start, nact = left <= 0 ? 0 : (left < 64 ? left : 64);
        check(s.nact == nact, name, tile, wave);
        if (nact) check(s.r == r && s.kb == kb && s.start == start && s.start + s.nact <= cnt[r], name, tile, wave);
        entries += s.nact;
      }
      // (the first wave of a tile always has work: a rung has a tile only for entries it holds)
      check(prefilter_slice(tpre.data(), cnt.data(), nrung, ntiles, tile, 0).nact > 0, "a tile's first wave has entries", tile, r);
    }
  }
  check(tile == ntiles, "the linear walk visits ntiles tiles", tile, ntiles);
  check(entries == total, "the slices cover every entry exactly once", (int)entries, (int)total);
  for (int past : {ntiles, ntiles + 1, ntiles + 1000, -1})
    for (int wave = 0; wave < 4; ++wave)
      check(prefilter_slice(tpre.data(), cnt.data(), nrung, ntiles, past, wave).nact == 0, "past the end: nothing to do", past, wave);
}

int main() {
  walk({0, 0, 819, 0, 1024, 1, 0, 0, 256, 257, 0}, "empty rungs at the start, in the middle and at the end");
  walk({1025}, "one rung");
  walk({0, 0, 0}, "nothing listed at all");
  walk({0, 64, 0}, "a single wave's worth");
  walk({870, 903, 1088, 1030, 1024, 5}, "partial last tiles");
  std::mt19937 rng(11);
  for (int k = 0; k < 200; ++k) {
    std::vector<int> cnt(1 + rng() % 40);
    for (int& c : cnt) c = (rng() % 3 == 0) ? 0 : (int)(rng() % 1400);
    walk(cnt, "random lists");
  }
  if (failures) fprintf(stderr, "%d broken properties\n", failures);
  else printf("ok\n");
  return failures ? 1 : 0;
}
