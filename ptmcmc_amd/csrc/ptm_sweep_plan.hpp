// ptm_sweep_plan.hpp -- which kernel a sweep (and a whole step) runs on: the decision, once, as plain C++ (no HIP: the
// launches in ptm_sweep_inst.inc, the engine's preparations for them and the names it reports all read the same plan).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace ptm {

enum { PLAN_DENSE = 0, PLAN_DIAG = 1, PLAN_LOWER = 2 };   // the proposal factor's storage: KIND_* of ptm_kernels.hpp

// everything the choice of a sweep kernel depends on
struct SweepFacts {
  int DP, W;            // padded dimension, walkers per rung
  long long chains;     // the chains of this launch (c_end - c_begin)
  int nloc;             // local rungs
  int kind;             // PLAN_*
  bool has_bounds, bounds_box, all_uniform, has_mean, any_oned;
  int mix_K;
  bool evolving;        // evolving ladders: per-chain temperatures (betaC)
  bool tracked;         // history or MAP tracking
  bool user_like;       // a user likelihood, on the host or on the device (propose / accept passes)
  bool host_prop;       // host-side proposals: they take over from every device proposal
  bool de, ada;         // differential evolution drawn on the device; an adaptive proposal set
  int mode;             // 0: a whole sweep, 1 / 2: the propose / accept pass around a user likelihood
  bool touched;         // an exchange phase ran since the last sweep
  // (read by de_mfma_applies alone -- plan_sweep does not look at them; zero: as before they existed)
  bool prior_draw;      // a member of the set draws from the prior (`de` is set for it too: it routes as differential evolution does)
  bool history;         // the history ring records every local rung (what differential evolution draws from)
};

// the environment's say: PTM_FORCE_VALU set, non-empty and not "0" keeps every workload off the matrix cores and off the lanes
// kernel's population rules (A/B measurements, tests); PTM_COMPACT=0 switches the compacted sweep off; PTM_BOX_PREFILTER=0 switches
// the box pre-pass (ptm_box_prefilter.hpp) off, =1 gives it every rung of a sweep it is eligible for, unset: the estimate decides
// (prefilter_flag below); PTM_PREFILTER_GRID=n (n >= 1) caps the pre-pass's grid at n blocks, so that a small population walks many
// tiles per block as a big one does (tests; the results do not depend on it); PTM_DE_MFMA=0 keeps differential evolution off the
// matrix cores, =1 gives de_mfma32_kernel every population it is eligible for, unset: its population rule decides (de_mfma_applies
// below); PTM_BOX_PREFILTER_EXACT=1 runs the pre-pass on its double-precision kernel.  Read once per process.
struct SweepEnv {
  bool force_valu, compact_ok;
  int prefilter;        // 0: the estimate decides, 1: every eligible rung, -1: off
  int prefilter_grid;   // 0: the blocks the device holds at once, n >= 1: at most n blocks
  int de_mfma;          // PTM_DE_MFMA -- 0 (unset): the population rule of de_mfma_applies decides, 1: every eligible population, -1 ("0"): off
  int prefilter_exact;  // PTM_BOX_PREFILTER_EXACT -- 0 (unset, "0"): the pre-pass draws in single precision behind a margin (box_prefilter_f32_kernel),
                        // 1: in the sweep's double precision (box_prefilter_kernel: A/B runs inside one library, and a fallback).  The chains are the same
};
inline const SweepEnv& sweep_env() {
  static const SweepEnv v = [] {
    const char* f = getenv("PTM_FORCE_VALU");
    const char* c = getenv("PTM_COMPACT");
    const char* b = getenv("PTM_BOX_PREFILTER");
    const char* g = getenv("PTM_PREFILTER_GRID");
    const char* d = getenv("PTM_DE_MFMA");
    const char* x = getenv("PTM_BOX_PREFILTER_EXACT");
    const long gn = (g && *g) ? strtol(g, nullptr, 10) : 0;
    return SweepEnv{f && *f && *f != '0', !(c && *c == '0'), (b && *b) ? (*b == '0' ? -1 : 1) : 0, gn >= 1 ? (int)(gn < (1 << 20) ? gn : (1 << 20)) : 0,
                    (d && *d) ? (*d == '0' ? -1 : 1) : 0, (x && *x && *x != '0') ? 1 : 0};
  }();
  return v;
}

enum SweepFamily { FAM_GENERAL, FAM_LANES, FAM_LANES_ADA, FAM_MFMA32, FAM_MFMA64, FAM_MFMA128 };

// the chosen build: the family's kernel template and every argument of it
struct SweepPlan {
  SweepFamily family;
  int DP, kind;          // all families (the matrix-core kernels take a diagonal factor as a Cholesky factor)
  bool uni, simple, ada; // sweep_kernel<DP, KIND, UNI, SIMPLE, ADA>
  bool gen;              // sweep_lanes_kernel<DP, KIND, GEN>   (sweep_lanes_ada_kernel<DP, KIND>)
  bool hist;             // sweep_mfma32_kernel<KIND, HIST, MGEN, EV, compacted>
  int mgen;
  bool ev;
  bool bnd;              // sweep_mfma{64,128}_kernel<KIND, BND, EV>
  bool compacted;        // the moving chains' lists are to be built (partition_kernel) before the launch
  bool prefilter;        // the box pre-pass (ptm_box_prefilter.hpp) may take rungs of this sweep: not an argument of the build, and not in its name
};
// the lean matrix-core build of evolving ladders reads the ladder-major temperatures, every other build the chain-indexed image
inline bool reads_ladder_major_beta(const SweepPlan& s) { return s.family == FAM_MFMA32 && s.mgen == 0 && s.ev; }

// the lanes kernel (ptm_lanes_kernel.hpp) takes launches of at most this many lanes (chains x padded dimension)
#define PTM_LANES_MAX (1ll << 20)

inline SweepPlan plan_sweep(const SweepFacts& f, const SweepEnv& env) {
  SweepPlan s = {};
  s.DP = f.DP;
  s.kind = f.host_prop ? PLAN_DIAG : f.kind;                 // (host-side proposals read no factor: any instantiation serves)
  const bool uni = (f.W % 64) == 0;                          // whole waves per rung
  const bool ada = f.ada && !f.host_prop;                    // (host-side proposals take over from an adaptive set)
  const bool box = f.all_uniform && (!f.has_bounds || f.bounds_box);   // uniform priors, open / `limit` bounds
  const bool recipe = f.has_mean || f.any_oned || f.mix_K != 0;         // a mean, one-dimensional moves, a scale mixture
  // open bounds, all-uniform prior, zero mean, no 1-D moves, no mixture, fixed ladder, device target and proposals
  const bool plain = !f.has_bounds && f.all_uniform && !recipe && !f.user_like && !ada && !f.evolving && !f.host_prop;
  const bool simple = uni && plain;
  // ... plain but for evolving ladders, untracked: the lean matrix-core build that reads per-chain temperatures
  const bool lean_ev = uni && f.evolving && !f.has_bounds && f.all_uniform && !recipe && !f.user_like && !ada && !f.host_prop && !f.tracked;
  const bool mfma_ok = uni && f.mode == 0 && !f.user_like && !f.host_prop && !ada && !env.force_valu;
  const int mk = s.kind == PLAN_DIAG ? PLAN_LOWER : s.kind;  // a diagonal factor is a (very sparse) Cholesky factor

  if (f.DP == 32 && mfma_ok && !f.de) {
    // both matrix products on the f64 matrix cores (ptm_mfma_kernel.hpp).  Compacted: after an exchange phase ~1/6 of a long ladder's
    // chains make no move, and the untracked builds of a big population visit the moving chains only (the same answer for every
    // partial sweep of a step)
    s.family = FAM_MFMA32; s.kind = mk;
    s.compacted = env.compact_ok && f.touched && box && !f.tracked && f.W >= 1024 && f.nloc <= 4096;
    s.hist = f.tracked;
    // 0 lean; 1 uniform priors and box bounds with the recipe's code, 3 without it (built compacted only); 2 everything
    s.mgen = (simple || lean_ev) ? 0 : !box ? 2 : (s.compacted && !recipe) ? 3 : 1;
    s.ev = !simple && box && f.evolving;
    // The box pre-pass settles proposals that have left an all-uniform prior's box in dimensions 0..15: the compacted lean build of a
    // fixed ladder (open bounds, no mean, no one-dimensional moves, no mixture -- `simple`), with a lower-triangular or diagonal factor
    // (a dense factor reaches every row from every column).  Evolving ladders are left out: nothing tests them with it.
    s.prefilter = env.prefilter >= 0 && s.compacted && s.mgen == 0 && !s.ev && (f.kind == PLAN_LOWER || f.kind == PLAN_DIAG);
    return s;
  }
  if ((f.DP == 64 || f.DP == 128) && mfma_ok && box && !recipe && !f.tracked) {
    // 33..128 dimensions, whole waves per rung, the plain workload (or open / `limit` bounds and / or evolving ladders on top of it)
    // without history (ptm_mfma64_kernel.hpp, ptm_mfma128_kernel.hpp); everything else at these dimensions keeps the lanes kernel
    s.family = f.DP == 64 ? FAM_MFMA64 : FAM_MFMA128; s.kind = mk;
    s.bnd = f.has_bounds; s.ev = f.evolving;
    return s;
  }
  // A lane per dimension instead of a lane per chain -- a sixteenth of the latency, twice the lane-work per chain: small populations
  // (fewer than 64 walkers per rung) until the chip is full of waves; up to 8 dimensions a chain is little work for one lane, and the
  // lanes kernel is the choice of the latency regime only.  Differential evolution keeps a population with whole waves per rung off
  // the matrix cores: from 9 dimensions on its moderate sizes are better off here than with a lane walking a chain
  // (measured, tools/de_probe_walkers.sh, us per step lanes / lane-per-chain: 12 dimensions x 4096 chains 40 / 57, x 16384 50 / 62,
  //  x 65536 96 / 75; 32 dimensions x 8192 chains 49 / 131)
  const long long lanes = f.chains * f.DP;
  const long long lanes_max = f.DP >= 16 ? PTM_LANES_MAX : 4096ll * f.DP, lanes_max_de = f.DP >= 32 ? (1ll << 21) : (1ll << 19);
  if (f.DP >= 64 || f.host_prop ||
      (!env.force_valu && ((!uni && lanes <= lanes_max) || (uni && f.de && f.DP >= 16 && lanes <= lanes_max_de)))) {
    s.family = ada ? FAM_LANES_ADA : FAM_LANES;
    s.gen = !plain;
    return s;
  }
  s.family = FAM_GENERAL;
  s.uni = uni; s.simple = simple; s.ada = ada;
  return s;
}

// Differential evolution on the matrix cores (de_mfma32_kernel, ptm_de_mfma_kernel.hpp): asked next to the plan, which stays what it
// was -- where this holds, the engine launches that kernel in place of the plan's and prepares as for the plan's (a general sweep
// that is not compacted).  The kernel is the box-bounds build of the 32-D matrix-core sweep with history, so: 32 padded dimensions,
// whole waves per rung, a whole sweep on device target and proposals, a fixed set with differential evolution in it and no draw from
// the prior, an all-uniform prior with open / `limit` bounds, history on.
// Population: unset, PTM_DE_MFMA leaves it to chains x DP > 2^21 -- exactly where plan_sweep leaves the lanes kernel for the general
// one with differential evolution, so the kernel only ever takes over from sweep_kernel<32, ...>; 1 takes every eligible population
// (tests, measurements), 0 none.
inline bool de_mfma_applies(const SweepFacts& f, const SweepEnv& env) {
  if (env.de_mfma < 0 || env.force_valu) return false;
  if (f.DP != 32 || (f.W % 64) != 0 || f.mode != 0) return false;
  if (f.user_like || f.host_prop || f.ada) return false;
  if (!f.de || f.prior_draw || f.mix_K <= 0 || !f.history) return false;
  if (!(f.all_uniform && (!f.has_bounds || f.bounds_box))) return false;
  return env.de_mfma > 0 || f.chains * f.DP > (1ll << 21);
}

// ---- which rungs the box pre-pass takes -------------------------------------------------------------------------------------
// It pays on a rung where the share of proposals it settles exceeds its own cost per chain relative to the sweep's (both kernels are
// bound by instruction issue, so cost is per listed chain).  The share is estimated for a state uniform in the box -- which is what
// the hot rungs of a ladder hold, and the cold ones, deep inside the box, settle next to nothing either way.  A heuristic: a wrong
// flag changes which kernel does the work and nothing in the results.
constexpr int PREFILTER_DIMS = 16;
#ifndef PTM_PREFILTER_THRESHOLD
#define PTM_PREFILTER_THRESHOLD 0.70   // measured break-even 0.40-0.43 with the pipelined pass (what a pre-pass chain costs of a sweep chain, DESIGN 3.1;
                                       // 0.50-0.57 before it) + a margin: on the rungs between cold and hot the state is not yet uniform in
                                       // the box and the estimate reads high (0.60 estimated where a model of the sampler counts 0.22), at
                                       // 0.70 it is within 0.1.  Re-measured with the cheaper pass: 0.50 / 0.57 / 0.63 / 0.70 give the same
                                       // step within the noise (the rungs in between sit at the break-even): it stays
#endif
// the standard deviations of the first 16 coordinates of a rung's proposal: sigma_d^2 = sum_k T[d][k]^2 (factor: row-major D x D, or D sigmas)
inline void prefilter_sigmas(bool diag, const double* factor, int D, double* sigma) {
  for (int d = 0; d < PREFILTER_DIMS; ++d) {
    double s2 = 0.0;
    if (d < D) {
      if (diag) s2 = factor[d] * factor[d];
      else for (int k = 0; k < D; ++k) s2 += factor[(size_t)d * D + k] * factor[(size_t)d * D + k];
    }
    sigma[d] = std::sqrt(s2);
  }
}
// ---- the single-precision pre-pass's margin (box_prefilter_f32_kernel) ------------------------------------------------------------
// That kernel forms a_d = sum_k float(T[d][k]) z32_k in float where the sweep forms A_d = sum_k T[d][k] z_k in double, and settles a
// chain only where x_d + a_d is outside the box by more than m_d >= |a_d - A_d|.  Two terms, per unit of S_d = sum_k |T[d][k]|:
//   PTM_BP_DZ          |z32 - z| per normal: the float radius, sine and cosine against the sweep's and the rounding of their product.
//                      Scanned over all 2^32 arguments of either half on the device (tests/test_gpu_box_prefilter_f32.py; the maxima
//                      are in DESIGN 3.1): max |dr| = 2.45e-4 where float(k1) rounds to 2^32, 6.76 max |dtrig| and 2^-22 for the
//                      product add a few 1e-6.  The constant is more than twice their sum; the test holds it to that.
//   PTM_BP_F32_SLACK   the rounding of T to float and of the float products and sums.  With u = 2^-24: float(T) = T (1 + e0), |e0| <= u,
//                      and in ANY order of summation (chained fused multiply-adds, plain products, partial sums added in a tree) a
//                      term of a 16-term sum passes through at most one product rounding and 15 additions, so what it arrives as is
//                      T z32 (1 + e0)(1 + e1)...(1 + e16), and |prod (1 + e) - 1| <= 17 u / (1 - 17 u) = 1.0133e-6 (Higham, Accuracy
//                      and Stability of Numerical Algorithms, lemma 3.1).  Times |z32| <= 6.7637 + PTM_BP_DZ: 6.86e-6 S_d, rounded up.
//                      (The sweep's own double-precision sum is off by 17 2^-53 6.77 S_d = 1.3e-14 S_d: inside the rounding up.)
//   Under- and overflow of float: a product or a factor entry below 2^-126 loses at most 2^-126 absolutely whether the hardware
//   flushes it or not -- 16 terms and their 16 factor entries times 6.77: PTM_BP_F32_TINY for every row that is not zero; a row with
//   S_d > 1e37 could pass FLT_MAX in a partial sum (16 x 6.77 x ...), and gets an infinite margin: it settles nothing.
// A zero row has a = A = 0 and the margin 0.  The double-precision roundings of x + a and of lo - m, hi + m are no part of this
// function: prefilter_face_slack covers them from the faces they happen at.
#define PTM_BP_DZ 6.0e-4
#define PTM_BP_F32_SLACK 7.0e-6
#define PTM_BP_F32_TINY 3.0e-36
inline double prefilter_margin(double sumabs) {
  if (sumabs == 0.0) return 0.0;
  if (!(sumabs <= 1e37)) return INFINITY;   // (a NaN too)
  return (PTM_BP_DZ + PTM_BP_F32_SLACK) * sumabs + PTM_BP_F32_TINY;
}
// the margins of a rung's first 16 dimensions (factor: row-major D x D, or D sigmas); a lower-triangular factor's rows d < 16 end at column d
inline void prefilter_margins(bool diag, const double* factor, int D, double* margin) {
  for (int d = 0; d < PREFILTER_DIMS; ++d) {
    double s = 0.0;
    if (d < D) {
      if (diag) s = std::fabs(factor[d]);
      else for (int k = 0; k < D; ++k) s += std::fabs(factor[(size_t)d * D + k]);
    }
    margin[d] = prefilter_margin(s);
  }
}
// x + double(a) is rounded in the pre-pass, x + A in the sweep, lo - m and hi + m on their way into the comparison: four roundings of
// numbers next to a face, each at most 2^-53 of it (the part of them that scales with m sits in the half of PTM_BP_DZ the scan leaves
// free).  Only a factor some 1e13 times narrower than the box's coordinates makes this the larger term.  An open face needs nothing.
inline double prefilter_face_slack(double lo, double hi) {
  const double a = std::fabs(lo) < INFINITY ? std::fabs(lo) : 0.0, b = std::fabs(hi) < INFINITY ? std::fabs(hi) : 0.0;
  return 0x1p-50 * (a > b ? a : b);
}
// the kernel reads a margin as a float (four registers per lane instead of eight): the smallest normal float that is not below m
inline float prefilter_margin_f32(double m) {
  if (!(m > 0.0)) return m == 0.0 ? 0.0f : INFINITY;   // (a NaN: nothing settles)
  if (m < 1.17549435e-38) return 1.17549435e-38f;
  float f = (float)m;
  if ((double)f < m) f = std::nextafterf(f, INFINITY);
  return f;
}

// P(x + sigma z leaves [0, w]) for x uniform in [0, w], z standard normal: 1 - erf(u / sqrt 2) + (2 / u)(phi(0) - phi(u)), u = w / sigma
// (for a narrow proposal 0.798 sigma / w: a half-normal's mean step out of each of the two faces)
inline double prefilter_out_1d(double sigma, double w) {
  if (!(sigma > 0.0) || !(w < INFINITY)) return 0.0;
  if (!(w > 0.0)) return 1.0;
  const double u = w / sigma, phi0 = 0.3989422804014327;
  const double in = std::erf(u * 0.7071067811865476) - (2.0 / u) * (phi0 - phi0 * std::exp(-0.5 * u * u));
  return in < 0.0 ? 1.0 : (in > 1.0 ? 0.0 : 1.0 - in);
}
// the share of a rung's proposals that leave the box in its first nd dimensions (independent faces: 1 - prod (1 - P_d))
inline double prefilter_out_share(const double* sigma, const double* width, int nd) {
  double in = 1.0;
  for (int d = 0; d < nd; ++d) in *= 1.0 - prefilter_out_1d(sigma[d], width[d]);
  return 1.0 - in;
}
inline bool prefilter_flag(const double* sigma, const double* width, int nd, int env_prefilter) {
  if (env_prefilter < 0) return false;
  if (env_prefilter > 0) return true;
  return prefilter_out_share(sigma, width, nd) > PTM_PREFILTER_THRESHOLD;
}

// The pre-pass's tiles (256 listed walkers of one rung, four waves of 64) are enumerated rung by rung.  tpre[0..nrung): the inclusive
// prefix of the rungs' tile counts ceil(cnt[r] / 256), cnt[0..nrung): the rungs' list lengths, ntiles = tpre[nrung - 1].  Which rung
// and which slice of its list wave `wave` of tile `tile` works on: a binary search for the first rung whose prefix exceeds the tile
// (an empty rung never does), the tile's number kb within the rung, the first entry of the wave's 64 and how many of them exist.
// nact == 0: nothing to do -- the tile is past the end, or the wave's slice of a rung's last tile is empty.  The kernel asks this
// one function for the tile it works on and for every tile it loads ahead (ptm_box_prefilter.hpp), so the two cannot disagree.
#ifdef __HIPCC__
#define PTM_PLAN_HD __host__ __device__
#else
#define PTM_PLAN_HD
#endif
struct PrefilterSlice { int r, kb, start, nact; };
PTM_PLAN_HD inline PrefilterSlice prefilter_slice(const int* tpre, const int* cnt, int nrung, int ntiles, int tile, int wave) {
  PrefilterSlice s = {0, 0, 0, 0};
  if (tile < 0 || tile >= ntiles) return s;
  int lo = 0, hi = nrung - 1;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (tpre[mid] > tile) hi = mid; else lo = mid + 1; }
  s.r = lo;
  s.kb = tile - (lo ? tpre[lo - 1] : 0);
  s.start = (s.kb * 4 + wave) * 64;
  const int left = cnt[lo] - s.start;
  s.nact = left <= 0 ? 0 : (left < 64 ? left : 64);
  return s;
}

// the kernel's name as rocprofv3 prints it (sweep_kernel without its last, defaulted argument unless that is set); returns snprintf's count
inline int format_sweep_name(const SweepPlan& s, char* b, size_t n) {
  const auto tf = [](bool v) { return v ? "true" : "false"; };
  switch (s.family) {
    case FAM_MFMA32: return snprintf(b, n, "sweep_mfma32_kernel<%d, %s, %d, %s, %s>", s.kind, tf(s.hist), s.mgen, tf(s.ev), tf(s.compacted));
    case FAM_MFMA64:
    case FAM_MFMA128: return snprintf(b, n, "sweep_mfma%d_kernel<%d, %s, %s>", s.DP, s.kind, tf(s.bnd), tf(s.ev));
    case FAM_LANES: return snprintf(b, n, "sweep_lanes_kernel<%d, %d, %s>", s.DP, s.kind, tf(s.gen));
    case FAM_LANES_ADA: return snprintf(b, n, "sweep_lanes_ada_kernel<%d, %d>", s.DP, s.kind);
    default: break;
  }
  if (s.ada) return snprintf(b, n, "sweep_kernel<%d, %d, %s, false, true>", s.DP, s.kind, tf(s.uni));
  return snprintf(b, n, "sweep_kernel<%d, %d, %s, %s>", s.DP, s.kind, tf(s.uni), tf(s.simple));
}

// Small ladders (rungs x padded dimensions <= 256 lanes, device target and proposals): whole PT steps in one launch, a block per
// walker-ladder (ptm_fused_kernel.hpp).  decide_lds: DecideLds' bytes of the engine's exchange phase, which shares the block's LDS.
struct StepFacts {
  int DP, Nt, W;
  bool user_like, host_prop, ada, time_kernels;
  bool evolving, evolve_cut;   // evolving ladders; ... with a posterior-ordering cut
  size_t decide_lds;
};
inline bool fused_applies(const StepFacts& f, bool fused_ok) {
  if (!fused_ok || f.DP > 16 || (long long)f.Nt * f.DP > 256 || f.user_like || f.host_prop || f.ada || f.time_kernels) return false;
  if (f.evolving && (f.W > 64 || f.evolve_cut)) return false;   // (the new temperatures' chain-indexed image is then a separate launch)
  return f.decide_lds <= 96 * 1024;
}

}  // namespace ptm
