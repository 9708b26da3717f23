// ptm_count_limit.hpp -- the engine's horizon: how far a chain's counters may run, as plain C++ (no HIP: the engine's entry points
// and a stand-alone test program, tests/cxx/count_limit_main.cc, read the same arithmetic).
//
// Ntries, Naccept and Nhist are the reference's `int` (chain.hh:151-152,  MH_chain::Nhist): 32 bits on the device, and the saved row
// number, the rings' slot arithmetic and every history row's meta are made from them.  PTM_COUNT_MAX (include/ptm_engine.h) is the
// largest value the engine represents; the host refuses the call that could take a chain's counter past it, so that no kernel ever
// sees one beyond it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/ptm_engine.h"

namespace ptm {

// The most add_state calls ONE chain can make in one PT step.  A rung the exchange phase leaves alone makes its Metropolis move: one
// add_state (chain.cc:1544-1559, 916-949; Ntries + 1 too).  A rung named by an exchange trial makes an add_state per trial, accepted or
// not (chain.cc:1487-1490, 1531-1534), and no Metropolis move.  Rung r can be in the trial of pair (r-1, r) and in that of pair
// (r, r+1), each pair at most once per step: the candidate selection drops a pick that repeats an earlier one or sits one above it
// (chain.cc:1417-1418), which still lets pair (r, r+1) be picked BEFORE pair (r-1, r).  So: 2 (the checker counts them in `touched`).
constexpr int64_t PTM_ADDS_PER_STEP = 2;

// would `n` more steps possibly take a counter that stands at `max_count` past the limit?  (max_count <= 2^32, n <= INT_MAX: the sum
// stays far inside an int64_t)
inline bool count_exceeds(int64_t max_count, int64_t n) { return n > 0 && max_count + PTM_ADDS_PER_STEP * n > (int64_t)PTM_COUNT_MAX; }

// what ptm_restore accepts for one chain; nullptr = fine
inline const char* count_restore_error(int64_t ntries, int64_t naccept, int64_t nhist) {
  if (ntries < 0 || ntries > (int64_t)PTM_COUNT_MAX) return "ntries";
  if (naccept < 0 || naccept > (int64_t)PTM_COUNT_MAX) return "naccept";
  if (nhist < 0 || nhist > (int64_t)PTM_COUNT_MAX) return "nhist";
  if (naccept > ntries) return "naccept > ntries";
  return nullptr;
}

// max over chains of max(ntries, nhist), from the device arrays' images (nhist is unsigned there)
inline int64_t count_true_max(const int32_t* ntries, const uint32_t* nhist, size_t n) {
  int64_t m = 0;
  for (size_t c = 0; c < n; ++c) {
    if ((int64_t)ntries[c] > m) m = ntries[c];
    if ((int64_t)nhist[c] > m) m = nhist[c];
  }
  return m;
}

// A host-side upper bound of max over chains of max(Ntries, Nhist): every admitted call raises it by the most its steps can add, so the
// hot path pays one add and one compare.  When the bound trips the caller reads the two arrays once, re-bases the bound to the true
// maximum (count_true_max) and asks again: with the true maximum, admit() IS the refusal rule.
struct CountHorizon {
  int64_t bound = 1;   // (Ntries starts at 1, chain.cc:649)
  bool admit(int64_t n) {
    if (n <= 0) return true;
    if (count_exceeds(bound, n)) return false;
    bound += PTM_ADDS_PER_STEP * n;
    return true;
  }
  void rebase(int64_t true_max) { bound = true_max; }
};

}  // namespace ptm
