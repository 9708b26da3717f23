/* include/ptm_engine.h -- C ABI of the MI355X parallel-tempering step engine.
 *
 * This is the drop-in boundary for ONE hot path of JohnGBaker/ptmcmc: chain::step()
 *   MH_chain::step                       chain.cc:966-1022
 *   MH_chain::add_state                  chain.cc:916-949
 *   parallel_tempering_chains::step      chain.cc:1393-1571
 * behind the reference's plug-in surface (bayes_likelihood / probability_function /
 * proposal_distribution, ptmcmc_sampler).  Plain C: pointers and sizes only, no C++ or
 * torch types.  All HOST pointers unless a parameter says "device".
 *
 * Conventions
 *   - every function returns PTM_OK (0) or a negative ptm_status; ptm_last_error() gives text.
 *   - a "chain" is one (rung, walker) pair.  Walkers are W independent ladders batched together
 *     (the reference's nearest notion is Nchain independent repeats, testMH.cpp:17,206).
 *   - an engine holds the contiguous rung block [rung_begin, rung_begin+rung_count) of a global ladder
 *     of n_rungs rungs, for all W walkers.  Local chain index  c = (rung - rung_begin) * W + walker.
 *     Host-visible arrays are chain-major in that order; states are [chain][dim] row-major.
 *   - random streams are keyed by GLOBAL identities (seed, global rung, walker, step), so results do
 *     not depend on how the ladder is sharded or how kernels are launched.
 */
#ifndef PTM_ENGINE_H
#define PTM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTM_ABI_VERSION 3   /* 2: ptm_config.walker_begin (a v1 caller's shorter struct is still accepted: walker_begin = 0); 3: ptm_calibrate, ptm_get_counter_sums, ptm_get_ladder_stats (additions only) */

typedef struct ptm_engine ptm_engine;

/* The horizon.  The largest value of any chain's Ntries, Naccept or Nhist that the engine represents: the reference's own `int`
 * (chain.hh:151-152).  ptm_restore refuses counters outside [0, PTM_COUNT_MAX]; every call that advances chains refuses
 * (PTM_ERR_UNSUPPORTED, nothing queued, the engine stays usable) when it could take a counter past it: a call of n PT steps is
 * refused if and only if  max over this engine's chains of max(Ntries, Nhist) + 2 n > PTM_COUNT_MAX  -- 2 being the most add_state
 * calls one chain can make in one step (a rung in two exchange trials, chain.cc:1410-1537).  A step made in pieces (ptm_exchange_decide*,
 * ptm_exchange_install, ptm_sweep_rungs, ptm_exchange_finish_and_sweep) is one step: its first call is the one that is asked.
 * The remedy is a checkpoint that shifts the counters down: INTEGRATION.md, "The horizon".  The step count itself is 64 bits
 * (56 of them reach the random streams) and has no limit a run can meet. */
#define PTM_COUNT_MAX 2147483647

typedef enum {
  PTM_OK = 0,
  PTM_ERR_INVALID = -1,      /* bad argument / call order */
  PTM_ERR_UNSUPPORTED = -2,  /* feature not available on the device path (caller must use the host path) */
  PTM_ERR_HIP = -3,          /* HIP runtime error (text in ptm_last_error) */
  PTM_ERR_NO_DEVICE = -4,    /* no gfx950 device / code object cannot load */
  PTM_ERR_FAR_MOVE = -5,     /* neighbour-exchange mode saw a state cross more than one shard boundary in one step */
  PTM_ERR_CALLBACK = -6
} ptm_status;

/* boundary types -- values of boundary::{open,limit,reflect,wrap}, states.hh:34-37 */
enum { PTM_BOUND_OPEN = 0, PTM_BOUND_LIMIT = 1, PTM_BOUND_REFLECT = 2, PTM_BOUND_WRAP = 3 };
/* per-dimension prior types -- values of mixed_dist_product::{uniform,gaussian,polar,copolar,log},
 * probability_function.hh:151-155; 0 = flat (base probability_function, probability_function.hh:40) */
enum { PTM_PRIOR_FLAT = 0, PTM_PRIOR_UNIFORM = 1, PTM_PRIOR_GAUSSIAN = 2, PTM_PRIOR_POLAR = 3, PTM_PRIOR_COPOLAR = 4,
       PTM_PRIOR_LOG = 5 };
/* Gaussian step proposal storage (gaussian_prop, proposal_distribution.hh:145-227) */
enum {
  PTM_PROP_DENSE = 0, /* offset = M z, M dense D x D (e.g. eigenvectors * sqrt(eigenvalues), hh:173-176,207-213) */
  PTM_PROP_DIAG = 1,  /* offset_i = sigma_i z_i  (identity_trans, hh:155-163) */
  PTM_PROP_LOWER = 2  /* offset = L z, L lower triangular (Cholesky factor); same numbers as DENSE with zeros */
};

typedef struct ptm_config {
  uint32_t struct_size;   /* sizeof(ptm_config), for ABI evolution */
  int32_t dim;            /* D, 1..1024 (PTM_ERR_UNSUPPORTED above; 33..1024: functional, not tuned) */
  int32_t n_rungs;        /* global ladder length (Ntemps) */
  int32_t rung_begin;     /* first global rung held by this engine */
  int32_t rung_count;     /* rungs held by this engine (== n_rungs on one GPU) */
  int32_t n_walkers;      /* W independent ladders */
  uint64_t seed;          /* Philox key */
  double swap_rate;       /* parallel_tempering_chains ctor arg (chain.cc:1163); maxswapsperstep = 1+2*swap_rate*n_rungs */
  int32_t add_every_n;    /* history stride (save_every), >= 1 */
  double min_prior;       /* dpriormin / minPrior, MH_chain ctor (chain.cc:647); sampler default -30 */
  int32_t device;         /* HIP device ordinal, -1 = current device */
  void* stream;           /* hipStream_t to launch on; NULL = the engine creates its own */
  int32_t time_kernels;   /* !=0: bracket every sweep-kernel launch with HIP events (ptm_get_kernel_times) */
  int32_t swap_log_steps; /* reserved, must be 0 (the per-candidate swap log of the LAST step is always kept: ptm_get_last_swaps) */
  int32_t exchange_row_capacity; /* row slots per boundary message (multi-GPU); 0 = automatic:
                                  * min(n_walkers, n_walkers*swap_rate + 8 sigma + 64).  More rows crossing one boundary in
                                  * one step than this is reported as PTM_ERR_FAR_MOVE by ptm_sync, never silently dropped */
  int32_t history_rungs;    /* >0: keep the history MH_chain::add_state pushes (chain.cc:935-946) for the first
                             * history_rungs rungs held by this engine; 0 = off */
  int32_t history_capacity; /* rows per chain kept on the device (a ring: saved row s sits in slot s % capacity) */
  int32_t map_rungs;        /* >0: track the MAP state MH_chain::add_state keeps (chain.cc:931-934) for the first map_rungs
                             * rungs held by this engine (the ladder's MAP is rung 0's, chain.cc:1570-1571); 0 = off */
  int32_t walker_begin;     /* (ABI 2) GLOBAL index of this engine's first walker: the engine holds walkers [walker_begin,
                             * walker_begin + n_walkers) of a larger population of independent ladders, and every random stream
                             * is keyed by the global walker -- so a population split by WALKERS over several engines / GPUs
                             * (whole ladders each: no exchange between engines at all, evolving ladders included) gives the
                             * very chains of one engine holding them all.  0 for a single engine. */
} ptm_config;

/* user plug-in likelihood, batched: the C shape of bayes_likelihood::register_evaluate_log
 * (bayesian.hh:536-552: double(*)(void* object, const state& s)).  X is [n][dim] row-major. */
typedef void (*ptm_loglike_batch_fn)(void* user, const double* X, int n, int dim, double* out_llike);

/* A proposal evaluated on the HOST: the C shape of proposal_distribution::draw(state&, chain*) + log_hastings_ratio() +
 * type() (proposal_distribution.hh:65-87), batched over the chains that make a Metropolis move this step (rungs touched by
 * an exchange attempt make none, chain.cc:1553-1557).  In: current states X_cur[n][dim] row-major, each chain's GLOBAL rung
 * and walker, the PT step number (ptm_step_count).  Out: proposed states X_prop[n][dim] -- whole states, not offsets; the
 * engine enforces the boundaries, prices prior and likelihood and takes the Metropolis test on the device with
 * logH = log_hastings + newlpost - current_lpost (chain.cc:976-1002; a NaN log_hastings rejects, :990-993) --,
 * log_hastings[n], type[n] (what MH_chain::last_type becomes on acceptance) and valid[n] (preset to 1; 0 = the proposed
 * state is invalid as state::invalid() says, e.g. state::add on a space whose origin violates a `limit` bound). */
typedef void (*ptm_propose_batch_fn)(void* user, int n, int dim, const double* X_cur, const int32_t* rung, const int32_t* walker,
                                     uint64_t step, double* X_prop, double* log_hastings, int32_t* type, int32_t* valid);
/* proposal_distribution::accept() / reject() (proposal_distribution.hh:70-71; MH_chain::step, chain.cc:1009,1015): the
 * outcome of the moves proposed by the last ptm_propose_batch_fn call, same n / order; accepted[i] in {0, 1} */
typedef void (*ptm_proposal_result_fn)(void* user, int n, const int32_t* rung, const int32_t* walker, const int32_t* accepted);

const char* ptm_last_error(void);
int ptm_abi_version(void);
/* number of usable gfx950 devices (0 if none); never fails */
int ptm_device_count(void);

int ptm_engine_create(const ptm_config* cfg, ptm_engine** out);
int ptm_engine_destroy(ptm_engine* e);

/* ---- problem description (what bayes_likelihood::basic_setup + stateSpace describe) ---------------- */
/* stateSpace::set_bound per dimension (states.hh:70-76) */
int ptm_set_bounds(ptm_engine* e, const int32_t* lower_type, const int32_t* upper_type, const double* xmin,
                   const double* xmax);
/* mixed_dist_product(space, types, centers, halfwidths) (probability_function.cc:219-262) */
int ptm_set_prior(ptm_engine* e, const int32_t* types, const double* centers, const double* halfwidths);
/* llike(x) = like0 - 1/2 (x-mean)^T P (x-mean);  P row-major D x D symmetric; mean may be NULL
 * (cython/exampleGaussian.py:53-54,61,103-109) */
int ptm_set_target_gaussian(ptm_engine* e, const double* mean, const double* precision, double like0);
/* user likelihood evaluated on the host between a propose and an accept kernel */
int ptm_set_target_callback(ptm_engine* e, ptm_loglike_batch_fn fn, void* user);
/* A PRIOR evaluated on the host: the C shape of probability_function::evaluate_log(state&) (probability_function.hh:31-44,59)
 * for priors ptm_set_prior cannot describe -- independent_dist_product, transformed_dist, chain_distribution
 * (probability_function.hh:184-246) or a user's own subclass.  Batched like the likelihood (X [n][dim] row-major, one log-prior
 * each; -inf = outside the support).  The engine calls it for the VALID proposals of a step (stateSpace::enforce stays on the
 * device, and an invalid state has probability 0 without asking: probability_function.cc:283) before the likelihood, applies the
 * reference's prior gate (chain.cc:980) to the answer, and for every state it is handed by ptm_set_states / ptm_restore.  Needs
 * the host-callback likelihood (ptm_set_target_callback): the step is then propose kernel -> prior -> likelihood -> accept kernel.
 * The device-side prior (ptm_set_prior) is ignored while a prior callback is set, and ptm_init_from_prior refuses: draw the start
 * states with the prior's own drawSample and hand them over with ptm_set_states.  fn = NULL removes it. */
typedef void (*ptm_logprior_batch_fn)(void* user, const double* X, int n, int dim, double* out_lprior);
int ptm_set_prior_callback(ptm_engine* e, ptm_logprior_batch_fn fn, void* user);
/* A user likelihood evaluated ON THE DEVICE: called on the HOST once per sweep (and by the state set-up calls), in stream order;
 * it enqueues its work on `stream` (a hipStream_t) and may return before that work has run.  X_dev [n_rows][dim] row-major,
 * natural dimension order; rows [0, *count_dev) are the proposals MH_chain::step would evaluate, in local-chain order; rows past
 * the count hold states inside the prior's support (so a fixed-shape evaluation of all n_rows rows is safe); out_llike_dev
 * [n_rows].  The step is then exchange kernel -> propose pass -> pack -> the user's work -> scatter -> accept pass, all queued:
 * ptm_step(n) returns without waiting, as it does for the Gaussian target.
 * x_batch_dev [n_rows * dim] / llike_batch_dev [n_rows] are device buffers the engine hands to fn (NULL: the engine allocates
 * them).  n_rows is ptm_target_device_rows.  The last of ptm_set_target_gaussian / _callback / _device called wins.  Refused
 * (PTM_ERR_UNSUPPORTED) with a prior callback, host-side proposals, rung-sharded steps and partial sweeps. */
typedef void (*ptm_loglike_device_fn)(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                      double* out_llike_dev);
int ptm_set_target_device(ptm_engine* e, ptm_loglike_device_fn fn, void* user, double* x_batch_dev, double* llike_batch_dev);
/* n_rows of the device likelihood: this engine's local chain count */
int ptm_target_device_rows(ptm_engine* e);
/* the best log-posterior (lprior + llike) among the states the device likelihood evaluated since the last state set-up
 * (ptm_set_states / ptm_init_from_prior_k), and that state x[dim]: bayes_likelihood::bestPost / bestState.  Ties go to the
 * earliest (step, local chain), a NaN never becomes the best; before any evaluation -inf and the zero state. */
int ptm_get_best_evaluated(ptm_engine* e, double* lpost, double* x);
/* A user PRIOR evaluated ON THE DEVICE, beside the device likelihood: what ptm_set_prior_callback is to ptm_set_target_callback.  The
 * calling convention is ptm_loglike_device_fn's: fn is called on the HOST once per sweep (and by ptm_set_states / ptm_restore /
 * ptm_debug_evaluate), in stream order; it enqueues its work on `stream` (a hipStream_t) and may return before that work has run.
 * X_dev [n_rows][dim] row-major, natural dimension order, n_rows = ptm_target_device_rows.  Rows [0, *count_dev) are the VALID
 * proposals -- those that passed stateSpace::enforce, what a host prior is shown -- in local-chain order; rows past the count hold the
 * other chains' current states (set-up calls: copies of row 0), so a fixed-shape evaluation of all n_rows rows is safe.
 * out_lprior_dev [n_rows]; -inf = outside the support.  The batch buffers are the engine's own, apart from the likelihood's.
 * The step is then exchange kernel -> propose pass -> count + pack of the valid proposals -> the user's prior work -> prior gate
 * (chain.cc:980, on the device) -> count + pack of the wanted proposals -> the user's likelihood work -> scatter (+ best) -> accept
 * pass, all queued: ptm_step(n) returns without waiting.  The device-side prior (ptm_set_prior) is ignored for valid states while a
 * device prior is set; ptm_set_states / ptm_restore hand it the valid states, and the kept best (ptm_get_best_evaluated) uses its values.
 * Works with device proposals, differential evolution, mixtures, adaptive sets, evolving ladders, history, MAP and walker splits.
 * Refused (PTM_ERR_UNSUPPORTED): without the device likelihood (at ptm_set_states, ptm_restore and every stepping call -- the setters may
 * come in either order), beside a prior callback (the later call), with host-side proposals, on a rung shard, in partial sweeps and
 * exchange phases, and by everything that draws from the prior (ptm_init_from_prior*, ptm_draw_prior_rows,
 * ptm_set_proposal_prior_draw): draw the start states on the host.  fn = NULL removes it; the chains' log-priors are made anew by the
 * next ptm_set_states / ptm_restore. */
typedef void (*ptm_logprior_device_fn)(void* user, void* stream, int n_rows, int dim, const double* X_dev, const int32_t* count_dev,
                                       double* out_lprior_dev);
int ptm_set_prior_device(ptm_engine* e, ptm_logprior_device_fn fn, void* user);
/* inverse temperatures of the GLOBAL ladder, beta[n_rungs] (chain.cc:1181-1183,1340) */
int ptm_set_ladder(ptm_engine* e, const double* beta);
/* parallel_tempering_chains::evolve_temps(rate, lpost_cut) (chain.hh:302-307; default-on in the sampler with rate 0.01,
 * lpost_cut -1: ptmcmc.cc:389-390,512).  After every accepted exchange of rungs (i, i+1) the reference widens that gap of
 * inverse temperatures by (1 + rate), renormalises all gaps and resets every rung's temperature (pry_temps,
 * chain.cc:1501-1518,1809-1846).  Each of the n_walkers ladders then owns its temperatures.  The engine keeps a ladder's
 * gaps lazily normalised inside a step (same values up to rounding, pinned against the reference by tests/golden traces
 * 5 and 6) and rebuilds the temperatures once per step.  Call after ptm_set_ladder.  History rows and MAP values taken
 * during an exchange phase carry the temperature their rung had at that add_state, between two pries of the step, as in
 * the reference (chain.cc:1487-1490,1531-1534).  lpost_cut >= 0 (chain.cc:1819-1827): every pry also widens each gap whose two
 * chains' current log-posteriors are out of order by more than lpost_cut * invtemp; the exchange kernel then decides a
 * ladder's picks one after the other and goes over all its gaps after every accepted exchange (pinned against the reference by
 * traces 11 and 12).  On a rung shard (no history / MAP there): the exchange phase must then be fed the whole ladder's llikes,
 * ptm_exchange_decide_gathered. */
int ptm_set_evolve_temps(ptm_engine* e, double rate, double lpost_cut);
/* every ladder's inverse temperatures, beta[n_walkers][n_rungs] (the common ladder repeated while nothing evolves);
 * ptm_set_invtemps puts them back (checkpoint / resume of an evolving run; needs ptm_set_evolve_temps first) */
int ptm_get_invtemps(ptm_engine* e, double* beta);
int ptm_set_invtemps(ptm_engine* e, const double* beta);
/* proposals of the LOCAL rungs: factors[rung_count][D*D] row-major (DENSE/LOWER) or [rung_count][D] (DIAG);
 * one_d_frac[rung_count] (gaussian_prop oneDfrac) may be NULL (= 0).  One clone per rung as
 * parallel_tempering_chains::set_proposal does (chain.cc:1367-1386). */
int ptm_set_proposals(ptm_engine* e, int kind, const double* factors, const double* one_d_frac);
/* Replace ONE rung's factor between steps (same kind and layout as given to ptm_set_proposals; one_d_frac < 0 keeps the
 * rung's value): the engine side of user_gaussian_prop::check_update / reset_dist (proposal_distribution.cc:406-441,
 * 340-403), whose user callback hands a chain a new covariance during the run. */
int ptm_set_proposal_rung(ptm_engine* e, int local_rung, const double* factor, double one_d_frac);
/* Scale mixture on top of the rungs' factors: a proposal_distribution_set (proposal_distribution.cc:99-129) of K Gaussian
 * members that are scalar multiples of the rung's factor -- the sampler's default Gaussian recipe (ptmcmc.cc:117-139).
 * Arrays [rung_count][K]: cumulative shares (the set's bin_max: one uniform x picks the first member with x < share),
 * scales, oneDfracs.  offset = scale_k * (factor z); last_type = k + 10 * (1 if the move was one-dimensional).
 * K = 0 removes the mixture. */
int ptm_set_proposal_mixture(ptm_engine* e, int K, const double* cum_shares, const double* scales, const double* one_d_fracs);
/* ADAPTIVE proposal set: a proposal_distribution_set whose shares move with the members' outcomes (adapt_rate,
 * proposal_distribution.cc:131-166) -- the sampler's recipe with --prop_adapt_rate (ptmcmc.cc:60-143): the top set {members ...}
 * of which ONE member (`nested`) may itself be a set of K_inner Gaussians with its own rate.  Drawn and adapted on the device:
 *   draw    a set of more than one member takes one uniform x and picks the first member that is ready with x < threshold
 *           (differential evolution not ready yet: the next member); the top set's x is slot 3 of block 0 of the chain's
 *           Metropolis stream, the nested set's slot 0 of block 0 of tag 3 (the same stream and step).  type = i + 10 t for
 *           a top member i of type t, i + 10 (j + 10 t) for member j of the nested set.
 *   update  after every Metropolis move of a rung the exchange phase left alone (rejections as invalid or by the prior cut
 *           included), for a set of rate != 0: a member whose outcome repeats its last one has its weight multiplied by
 *           1 - rate/4; its last outcome is stored and the set's outcome count goes up; from 10 x members outcomes on (the count
 *           is never reset) the weights are renormalised and the thresholds rebuilt after EVERY outcome (reset_bins, Tpow = 0).
 *           The outcome is then handed to the picked member: a picked nested set adapts the same way.
 * Leaves [rung_count][K + K_inner]: top members 0..K-1, then the nested set's members; scale < 0 = differential evolution
 * (ptm_set_proposal_de; top level only, at most one, not the last top member); the nested member's own top entry is not read.
 * Initial state per LOCAL chain (chain c = r * n_walkers + w): weights and thresholds [Nc][K + K_inner] (thresholds non-decreasing,
 * each set's last exactly 1: the engine derives none itself, so a host-side copy and the device start from the same bits),
 * repeat bits [Nc][2] (bit i: member i's last outcome was an accept; top set, nested set) and outcome counts [Nc][2].
 * Replaces the mixture of ptm_set_proposal_mixture; a later ptm_set_proposal_mixture (any K) switches adaptation off, a non-NULL
 * ptm_set_proposal_callback takes over.  The state is per chain and is not part of ptm_restore: read it with
 * ptm_get_proposal_adapt_state, put it back with ptm_set_proposal_adapt_state.  Every argument is checked before the current
 * configuration is touched (PTM_ERR_INVALID: it keeps working); rung shards: PTM_ERR_UNSUPPORTED.  Steps of such an engine take
 * the exchange kernel and the lanes or the general sweep kernel (never the matrix-core, fused small-ladder or persistent kernels: the
 * persistent kernel is out of scope for adaptive sets). */
typedef struct ptm_adaptive_set {
  int K;              /* members of the top set, 1..8 */
  int nested;         /* top member that is itself a set of K_inner Gaussians, or -1 */
  int K_inner;        /* 0, or 1..8 when nested >= 0 */
  double rate;        /* the top set's adapt_rate, in [0, 1) (0: its shares stay fixed) */
  double rate_inner;  /* the nested set's, in [0, 1) */
} ptm_adaptive_set;
int ptm_set_proposal_adaptive(ptm_engine* e, const ptm_adaptive_set* set, const double* scales, const double* one_d_fracs, const double* weights,
                              const double* thresholds, const int32_t* repeat_bits, const int32_t* outcomes);
/* the per-chain state of the adaptive set, layouts as ptm_set_proposal_adaptive's initial state (queued inside ptm_batch_begin / _end) */
int ptm_get_proposal_adapt_state(ptm_engine* e, double* weights, double* thresholds, int32_t* repeat_bits, int32_t* outcomes);
int ptm_set_proposal_adapt_state(ptm_engine* e, const double* weights, const double* thresholds, const int32_t* repeat_bits, const int32_t* outcomes);

/* Host-side proposals -- the "host fallback step" for everything that is not a Gaussian the device can draw itself
 * (involutions, draws from a distribution other than the engine's prior, temperature-dependent shares of a set that adapts, user
 * proposals with callbacks ...; draws from the prior itself are a device member: ptm_set_proposal_prior_draw):
 * every sweep fetches the current states, calls `propose` once for all moving chains, and runs the rest of
 * MH_chain::step on the device.  `result` (may be NULL) is told the outcomes after the accept kernel.  Replaces the
 * proposals of ptm_set_proposals; propose == NULL goes back to them.  Whole-shard sweeps only (ptm_sweep, ptm_step,
 * ptm_exchange_finish_and_sweep; not ptm_sweep_rungs).  Clears device proposals (ptm_set_proposal_device, below): the last of the two
 * setters called wins. */
int ptm_set_proposal_callback(ptm_engine* e, ptm_propose_batch_fn propose, ptm_proposal_result_fn result, void* user);
/* The same proposals ON THE DEVICE: ptm_propose_batch_fn's contract with every array in device memory and no host round trip.
 * `propose` is called on the HOST once per sweep, in stream order; it enqueues its work on `stream` (a hipStream_t) and may return
 * before that work has run: ptm_step(n) returns without waiting, as it does for the engine's own proposals.  n_rows is the local
 * chain count; `step` is ptm_step_count at the sweep (a host value: the call is made when the sweep is queued).
 * Rows [0, *count_dev) are the chains that make a Metropolis move this step (touch flag 0: rungs touched by an exchange attempt
 * make none, chain.cc:1553-1557), in local-chain order -- the set and order ptm_propose_batch_fn is handed.  X_cur_dev
 * [n_rows][dim] row-major, natural dimension order; rung_dev / walker_dev [n_rows] the GLOBAL rung and walker of each row.  Rows
 * past the count hold the other chains' current states and ids, so a fixed-shape evaluation of all n_rows rows is safe; their
 * outputs are never read.
 * Before the call the engine presets log_hastings = 0, type = 0, valid = 1 for every row; X_prop_dev [n_rows][dim] is undefined on
 * entry, and the function writes whole states (not offsets) for every row below the count.  The outputs mean what
 * ptm_propose_batch_fn's mean: a NaN ratio rejects, valid = 0 is state::invalid(), type becomes last_type on acceptance.
 * `result` (may be NULL) is called once per sweep after the accept pass has been queued, with accepted_dev[k] in {0, 1} for
 * k < *count_dev: the rows and order of the propose call.
 * propose == NULL goes back to the engine's own proposals.  Setting device proposals clears host-side proposals and the reverse
 * (the last call wins); every argument is checked before anything changes.  Works with the Gaussian target, the host-callback
 * likelihood (and a prior callback), the device likelihood (ptm_set_target_device: the step then stays on the device end to end),
 * evolving ladders, history, MAP and populations split by walkers.  Refused (PTM_ERR_UNSUPPORTED) where host-side proposals are:
 * ptm_sweep_rungs on part of a shard, rung-sharded steps.  While set, ptm_set_proposal_de, _prior_draw and the like answer as they
 * do with host-side proposals, and the sweep is the lanes kernel's general build. */
typedef void (*ptm_propose_device_fn)(void* user, void* stream, int n_rows, int dim,
        const double* X_cur_dev,            /* [n_rows][dim] row-major, natural dimension order */
        const int32_t* rung_dev, const int32_t* walker_dev,   /* [n_rows] GLOBAL rung / walker of each row */
        const int32_t* count_dev, uint64_t step,
        double* X_prop_dev, double* log_hastings_dev, int32_t* type_dev, int32_t* valid_dev);
typedef void (*ptm_proposal_result_device_fn)(void* user, void* stream, int n_rows,
        const int32_t* rung_dev, const int32_t* walker_dev, const int32_t* count_dev, const int32_t* accepted_dev);
int ptm_set_proposal_device(ptm_engine* e, ptm_propose_device_fn propose, ptm_proposal_result_device_fn result, void* user);
/* Differential evolution (ter Braak & Vrugt 2008) drawn ON THE DEVICE from each chain's own saved history -- the reference's
 * differential_evolution (proposal_distribution.cc:476-801) as the reference sampler configures it by default (ptmcmc.cc:81-91: no
 * temperature mixing, unlikely_alpha = 0).  It becomes the member of the rungs' proposal sets (ptm_set_proposal_mixture) whose SCALE
 * IS NEGATIVE: the set's uniform picks the first ready member whose cumulative share it falls below
 * (proposal_distribution_set::draw, proposal_distribution.cc:99-129; differential evolution is ready once the chain has saved
 * 10 * dim rows, and is passed over until then -- give it a member behind it); type code = member + 10 * (0 parallel move, 1 snooker).
 * The engine must have been created with history_rungs = rung_count and a history_capacity that holds EVERY row of the run (a row the
 * ring has lost is reported by ptm_sync).  init_rows [n_init_extra][n_local_chains][dim], chain (local rung r, walker w) at
 * r * n_walkers + w: the states MH_chain::initialize(n) saved in FRONT of the start state (chain.cc:846-876: n_init_extra = n - 1,
 * oldest first), or NULL with n_init_extra = 0.  Needs dim <= 128 and the whole ladder on this engine (rung_count == n_rungs; populations
 * split by walkers are fine: PTM_ERR_UNSUPPORTED on a rung shard, whose top rung's history cannot be complete).  q == NULL switches it off.  Host-side draws with temperature
 * mixing or unlikely_alpha stay possible through ptm_set_proposal_callback.
 * Which kernel draws it: the persistent ladder, fused small-ladder, lanes and general kernels, and for 17..32 dimensions with whole
 * waves per rung, an all-uniform prior and open / `limit` bounds also the matrix cores (de_mfma32_kernel: the Gaussian members' products
 * on the f64 matrix cores, the evolution's states formed in the same layout) -- by default for populations of more than 2^21 lanes
 * (chains x 32), where the lanes kernel used to hand over to the general one; PTM_DE_MFMA=1 in the environment gives it every
 * eligible population, PTM_DE_MFMA=0 none.  The chains are the same bit for bit whichever kernel draws. */
typedef struct ptm_de_params {
  double snooker;         /* probability of a snooker move (differential_evolution's first constructor argument; sampler: 0.1) */
  double gamma_one_frac;  /* probability of gamma = 1 in a parallel move (de_g1_frac: 0.3) */
  double reduce_gamma;    /* differential_evolution::reduce_gamma (de_reduce_gamma: 4) */
  double ignore_frac;     /* early fraction of a long history that is not drawn from (sampler: 0) */
} ptm_de_params;
int ptm_set_proposal_de(ptm_engine* e, const ptm_de_params* q, int n_init_extra, const double* init_rows);
/* INDEPENDENT DRAWS FROM THE PRIOR as a member of the current proposal set, drawn ON THE DEVICE -- the reference's draw_from_dist over
 * the prior (proposal_distribution.hh:119-132; the sampler's --prior_draw_frac, ptmcmc.cc:93-104).  `member` names the member of the
 * set given to ptm_set_proposal_mixture, or of the TOP level of ptm_set_proposal_adaptive, that proposes this way; -1 switches it off.
 * A new set (either call) forgets the member: name it again.  A chain whose pick lands on the member
 *   draws   dimension d from block d of its own stream (global walker and rung) under tag 4 at the PT step, the block's words used as
 *           ptm_init_from_prior uses them for the dimension's prior type; one draw, no redraw;
 *   is      a state of its own (valid unless enforcing the boundaries fails), not a sum on the current one;
 *   weighs  log_hastings = lprior(current) - lprior(proposed) into the Metropolis test (a NaN ratio rejects);
 *   reports type code = member (no one-dimensional moves: the member's oneDfrac is not read; its scale is not read either).
 * Differential evolution that is not ready hands its pick to the member behind it, which may be this one (the sampler's order).
 * Temperature-dependent shares (--prior_draw_Tpow) of a set that does not adapt need nothing more: give every rung its own cumulative
 * shares (mixture) or initial thresholds (adaptive set with top rate 0).
 * Unlike differential evolution it needs no history: rung shards (mixture), walker splits, ptm_sweep_rungs and the propose / accept
 * passes of user likelihoods all carry it (the accept pass makes member and ratio anew).  Steps of such an engine take the exchange
 * kernel and the lanes or the general sweep kernel, as with an adaptive set: never the matrix-core, fused small-ladder or persistent
 * kernels -- a 32-dimensional population of whole waves per rung runs where it ran with differential evolution before that moved to
 * the matrix cores (de_mfma32_kernel, see ptm_set_proposal_de): on the lanes kernel, past 2^21 lanes on the general one.
 * Every argument is checked before anything changes.  PTM_ERR_INVALID: member out of range, the nested set, or a member of negative
 * scale (differential evolution); host-side proposals are set.  PTM_ERR_UNSUPPORTED: a flat prior dimension, or a prior callback
 * (ptm_set_prior_callback) -- also reported by the next step if the prior changes to one of these afterwards. */
int ptm_set_proposal_prior_draw(ptm_engine* e, int member);

/* ---- state ------------------------------------------------------------------------------------------ */
/* X[n_local_chains][D]; llike may be NULL (the device target evaluates it).  Resets counters the way
 * MH_chain::initialize(1) leaves them (chain.cc:649,846-876). */
int ptm_set_states(ptm_engine* e, const double* X, const double* llike);
/* MH_chain::initialize(1): draw each chain's start from the prior until valid and of finite likelihood (chain.cc:846-876);
 * every mixed_dist_product type but the flat one can be drawn (PTM_ERR_UNSUPPORTED for a flat dimension) */
int ptm_init_from_prior(ptm_engine* e);
/* MH_chain::initialize(n) draws n states per chain (chain.cc:846-876); each of them is add_state'd, the last is where the chain
 * starts.  ptm_init_from_prior_k draws the k-th of them (k = 0: what ptm_init_from_prior draws) from its own slice of the
 * chain's initialisation stream, so a caller that wants n initial samples (the history seed of differential evolution,
 * ptmcmc.cc:86) calls it for k = n-1 .. 0, reading the states back in between.  Resets the counters like ptm_set_states. */
int ptm_init_from_prior_k(ptm_engine* e, int k);
/* Draws k_begin .. k_begin + n - 1 of every chain into host arrays -- x_out [n][n_local_chains][dim], ll_out / lp_out
 * [n][n_local_chains], chain (local rung r, walker w) at r * n_walkers + w: exactly the states, log-likelihoods and log-priors that
 * ptm_init_from_prior_k(e, k) would leave in the engine, whose own state stays untouched.  MH_chain::initialize(n)'s n - 1 rows in
 * front of the start state (chain.cc:846-876) in one call (then ptm_init_from_prior_k(e, 0) for the start state itself). */
int ptm_draw_prior_rows(ptm_engine* e, int k_begin, int n, double* x_out, double* ll_out, double* lp_out);

/* ---- the hot path ------------------------------------------------------------------------------------- */
/* n x { MH_chain::step for every chain } -- no exchange phase.  (This and every other call that advances chains:
 * PTM_ERR_UNSUPPORTED at the horizon, see PTM_COUNT_MAX.) */
int ptm_sweep(ptm_engine* e, int n);
/* n x parallel_tempering_chains::step (chain.cc:1393-1571; single-shard engines: rung_count == n_rungs).  ASYNCHRONOUS: the call
 * queues work on the engine's stream and returns; results are there when a getter, a setter or ptm_sync looks.  On the persistent
 * ladder kernel's path (populations whose workgroups are all resident at once, 1024 at the most; ptm_step_kernel_name) calls of fewer than 64 steps are only COUNTED and launched
 * together at that next look (or when 1024 have gathered) -- nothing can observe the difference, and a loop of ptm_step(1) calls, the
 * reference sampler's own (ptmcmc.cc:563-599), then costs what ptm_step(n) costs per step.  PTM_LADDER_DEFER=0 launches every call. */
int ptm_step(ptm_engine* e, int n);
/* wait for all queued work */
int ptm_sync(ptm_engine* e);

/* ---- multi-GPU building blocks (one engine per GPU; the caller moves bytes with RCCL) ---------------- */
/* Exchanges only ever propagate DOWN the ladder within one step (a candidate one above an earlier pick is dropped,
 * chain.cc:1417-1418), so a shard can replay every decision that concerns its rungs from: its own llikes, the llike
 * of the top rung of the shard below (W doubles) and the llikes of the bottom `halo_rungs` rungs of the shard above
 * ([halo_rungs][W]).  A chain of accepted exchanges longer than the halo sets PTM_ERR_FAR_MOVE (reported by ptm_sync). */
/* copy n_rungs rungs of the local llike array (current step), starting at local rung first_local_rung, to a device
 * buffer ([n_rungs][W] doubles) -- the halo a neighbour needs; asynchronous on the engine's stream */
int ptm_copy_llike(ptm_engine* e, int first_local_rung, int n_rungs, void* dst_dev);
/* device pointer to the local llike array of the CURRENT step, [rung_count*W] doubles, chain-major */
int ptm_llike_device_ptr(ptm_engine* e, void** dev_ptr);
/* exchange phase, part 1: decide all exchanges that concern this shard, move the rows that stay inside it and pack the
 * rows that leave it into the boundary messages send_up / send_down (device buffers of ptm_exchange_buffer_doubles()
 * doubles each; ignored at the ladder's ends).  A message is opaque to the caller: it is delivered whole to the
 * neighbour's ptm_exchange_finish_and_sweep.  (Layout: int32 row count, then ptm_exchange_row_capacity() slots of
 * {state[padded dim], llike, lprior, walker, 0}.)
 * ll_below_dev: [W] (ignored on the first shard); ll_above_dev: [halo_rungs][W] (ignored on the last shard). */
int ptm_exchange_decide(ptm_engine* e, const void* ll_below_dev, const void* ll_above_dev, int halo_rungs, void* send_up_dev,
                        void* send_down_dev);
/* The exchange phase of a shard from the WHOLE ladder's llikes -- what the reference's MPI ranks work from (gather_llikes /
 * gather_lposts: an MPI_Allgather per step, chain.cc:1433-1435,1905-1972).  ll_all_dev: [n_rungs][W] doubles, every shard's llike
 * array in rung order (the caller gathers them: ptm_copy_llike of each shard, an all-gather); lp_all_dev: the lpriors the same way
 * (ptm_copy_lprior), needed only with a posterior-ordering cut (else NULL).  No halo, no run of picks can reach past the view --
 * and it is the form EVOLVING ladders need on rung shards (ptm_set_evolve_temps): every accepted exchange renormalises all gaps
 * and every later trial of the step sees it, so every shard replays the whole ladder's trials and keeps the whole ladder's
 * temperatures.  Costs an all-gather of n_rungs x W doubles per step instead of two neighbour messages: for populations, prefer
 * splitting by walkers (ptm_config.walker_begin).  Boundary rows travel as with ptm_exchange_decide. */
int ptm_exchange_decide_gathered(ptm_engine* e, const void* ll_all_dev, const void* lp_all_dev, void* send_up_dev, void* send_down_dev);
/* RECOVERY of a run of surviving picks longer than a halo (instead of PTM_ERR_FAR_MOVE).  Whether some shard of a ladder is blind
 * in a step is a property of the step's candidate draws, which every shard replays: told the whole shard map (every shard's rung
 * count, in order, and the halo depth all of them ask for), ptm_exchange_decide leaves such a ladder alone ON EVERY SHARD -- the same
 * ladders everywhere, no message needed to agree -- and counts it.  The caller asks for the count after the decide pass
 * (ptm_exchange_redo_count: one wait on the device); if it is not zero -- on every rank alike -- it gathers the whole ladder's llikes
 * as for ptm_exchange_decide_gathered (the arrays of the ladders left alone are untouched) and ptm_exchange_redo decides those ladders
 * from the full view, appending their boundary rows to the same messages.  Then the step goes on as ever.  The reference never
 * fails here: its ranks gather everything every step (chain.cc:1905-1967).  ptmcmc_amd.parallel.ShardedLadder(recover=True) is the
 * driver; without a shard map a blind shard still says so loudly (PTM_ERR_FAR_MOVE). */
int ptm_set_shard_map(ptm_engine* e, int n_shards, const int32_t* rung_counts, int halo_rungs);
int ptm_exchange_redo_count(ptm_engine* e, int* n_ladders);
int ptm_exchange_redo(ptm_engine* e, const void* ll_all_dev, const void* lp_all_dev, void* send_up_dev, void* send_down_dev);
/* ptm_copy_llike's twin for the lpriors */
int ptm_copy_lprior(ptm_engine* e, int first_local_rung, int n_rungs, void* dst_dev);
/* exchange phase, part 2 + MH sweep: lands the rows of the neighbours' messages (device buffers of the same size; the
 * message from below is required unless this is the first shard, the one from above unless it is the last) */
int ptm_exchange_finish_and_sweep(ptm_engine* e, const void* recv_from_below_dev, const void* recv_from_above_dev);
/* The same in pieces, for callers that overlap the messages with arithmetic: the Metropolis moves of a step do not
 * depend on the rows in flight (their landing slots are exchanged rungs, which make no move), only the llike halo of
 * the NEXT step does.  ptm_sweep_rungs sweeps local rungs [first_local_rung, first_local_rung + n_rungs); every local
 * rung must be swept exactly once per step and the last call passes closes_step != 0. */
int ptm_exchange_install(ptm_engine* e, const void* recv_from_below_dev, const void* recv_from_above_dev);
int ptm_sweep_rungs(ptm_engine* e, int first_local_rung, int n_rungs, int closes_step);
/* size of one boundary message in doubles: 2 + row capacity * (padded dim + 4) */
int ptm_exchange_buffer_doubles(ptm_engine* e);
int ptm_exchange_row_capacity(ptm_engine* e);

/* ---- the same, driven natively over RCCL (for hosts that stay C/C++; ptmcmc_amd/parallel.py is the torch.distributed twin) --
 * One engine per process and GPU holds a contiguous rung block (rung_begin / rung_count); ptm_shard_step runs the whole sharded
 * PT step: llike halos and boundary rows travel as ncclSend / ncclRecv pairs between NEIGHBOUR ranks on a side stream, hidden
 * behind the sweep of the interior rungs (halos of the next step behind the second half).  RCCL is loaded at run time
 * (dlopen "librccl.so.1") by the first of these calls; nothing else in the library needs it.
 *   rank 0:   ptm_shard_unique_id(id)  -> hand the 128 bytes to every rank (file, socket, MPI, a launcher's environment ...)
 *   all:      ptm_shard_init(e, id, rank, world, rung_counts, halo)   rung_counts[world]: every rank's block length
 *             (rank r holds the block after rank r-1's; must agree with this engine's rung_begin / rung_count); halo <= 0: 12
 *             ptm_shard_step(e, n) ... ptm_sync(e) ...   ptm_shard_finalize(e) before ptm_engine_destroy
 * Replaces the reference's MPI layer for this path: rank/size `chain.cc:1199-1209`, the cyclic rung map `:1298-1309` and the
 * three MPI_Allgathers of every step `:1433-1435,1879-1972`. */
#define PTM_SHARD_ID_BYTES 128
int ptm_shard_unique_id(void* id_out);
int ptm_shard_init(ptm_engine* e, const void* id, int rank, int world, const int32_t* rung_counts, int halo_rungs);
int ptm_shard_step(ptm_engine* e, int n);
int ptm_shard_finalize(ptm_engine* e);

/* ---- read-back ------------------------------------------------------------------------------------------ */
enum {
  PTM_ARR_LLIKE = 0,  /* double */
  PTM_ARR_LPRIOR = 1, /* double */
  PTM_ARR_LPOST = 2,  /* double: lprior + beta*llike (chain.cc:928) */
  PTM_ARR_NTRIES = 3, /* int32: MH_chain::Ntries (starts at 1, chain.cc:649) */
  PTM_ARR_NACCEPT = 4,/* int32 */
  PTM_ARR_LAST_TYPE = 5, /* int32 */
  PTM_ARR_NHIST = 6,  /* int64: add_state calls */
  PTM_ARR_NSIZE = 7,  /* int64: history rows (chain.cc:935-946) */
  PTM_ARR_ROW_LABELS = 8 /* int32, a debug view: the rung slot of the device's row array that holds each chain's row.  Big populations
                          * exchange these labels instead of 256-byte rows; every call that reads or writes the states puts the rows
                          * back first (then: the chain's own rung).  This call reads the table as it stands. */
};
int ptm_get_states(ptm_engine* e, double* X);
int ptm_get_array(ptm_engine* e, int which, void* out);
/* per walker, per adjacent pair: attempts and accepts (swap_count / swap_accept_count, chain.hh:244-245);
 * each [W][n_rungs-1] int64 */
int ptm_get_swap_counts(ptm_engine* e, int64_t* tries, int64_t* accepts);
/* candidates of the most recent step: pairs[W][maxswaps] (lower rung or -2), accepted[W][maxswaps] */
int ptm_get_last_swaps(ptm_engine* e, int32_t* pairs, int32_t* accepted);
/* Several reads with one wait.  Every ptm_get_* call is an asynchronous copy on the engine's stream plus a wait; a host that
 * reads several arrays after every step (the facade's history mirror for host-side proposals: chain.cc:935-946 rows, the
 * swap log, the temperatures) brackets them: between ptm_batch_begin and ptm_batch_end the ptm_get_* calls only queue
 * their copies and return at once; the output buffers are filled when ptm_batch_end returns (possibly earlier).  Only
 * reads go between the two (ptm_step there is refused).  Brackets nest.  No counterpart in the reference (its arrays are host
 * memory); it exists because a wait on the device costs what ~10 small copies do. */
int ptm_batch_begin(ptm_engine* e);
int ptm_batch_end(ptm_engine* e);
/* Checkpoint / resume.  Everything a run's future depends on is: the states and their llikes (ptm_get_states,
 * PTM_ARR_LLIKE), the MH_chain counters (PTM_ARR_NTRIES / NACCEPT / LAST_TYPE / NHIST), the step count (the random
 * streams are counters of it) and, for the bookkeeping, the swap counters.  ptm_restore puts them back into an engine
 * configured like the one they came from (same seed, ladder, proposals, target); the run then continues bit for bit.
 * swap_tries / swap_accepts may be NULL (counters restart at 0).  An engine that keeps a history ring or a MAP starts
 * them afresh from the restored state; ptm_set_history / ptm_set_map (below) put saved ones back, and for an evolving
 * run ptm_set_evolve_temps + ptm_set_invtemps the ladders.
 * The states are taken as they were saved: a saved state went through stateSpace::enforce when it was proposed, and ptm_restore does
 * not enforce it again (ptm_set_states does; the reference's two-sided reflection, states.cc:31-45, is not idempotent).
 * PTM_ERR_INVALID, with nothing touched: a chain's ntries, naccept or nhist outside [0, PTM_COUNT_MAX], or naccept > ntries. */
int ptm_restore(ptm_engine* e, const double* X, const double* llike, const int32_t* ntries, const int32_t* naccept,
                const int32_t* last_type, const int64_t* nhist, uint64_t step_count, const int64_t* swap_tries,
                const int64_t* swap_accepts);
int ptm_max_swaps_per_step(ptm_engine* e);
/* History of the recorded rungs (ptm_config.history_rungs): for chain (local rung r, walker w) at index r*W + w and ring
 * slot k: X[(k*HC + index)*dim ..], llike / lprior [k*HC + index], meta [4*(k*HC + index)] = {Naccept, Ntries,
 * last_type, saved row number} as MH_chain::add_state saw them (acceptance_ratio = Naccept/Ntries, lpost = lprior +
 * beta*llike); HC = history_rungs * n_walkers.  Saved row s is in slot s % history_capacity; row 0 is the initial state
 * and a chain has saved Nsize rows (PTM_ARR_NSIZE).  Any output pointer may be NULL. */
int ptm_get_history(ptm_engine* e, double* X, double* llike, double* lprior, int32_t* meta);
/* the inverse temperature each saved row was saved at (MH_chain::invtemps, chain.cc:943), beta[k*HC + index]: the
 * ladder's value while the ladder is fixed, the chain's own once the ladders evolve */
int ptm_get_history_invtemps(ptm_engine* e, double* beta);
/* The ring entries of history chains [chain_begin, chain_begin + chain_count) only (chain = local rung * n_walkers + walker), written into
 * host arrays of ptm_get_history's FULL layout -- [capacity][history chains][..] -- whose other entries stay untouched; any of the five
 * pointers may be NULL.  What a chain-file writer needs (chain::dumpChain, chain.cc:1110-1140, for the rungs it dumps) without reading
 * every rung's ring: with differential evolution on the device the ring holds all rungs for the whole run. */
int ptm_get_history_chains(ptm_engine* e, int chain_begin, int chain_count, double* X, double* llike, double* lprior, int32_t* meta, double* invtemps);
/* put a saved ring / MAP back (after ptm_restore): the arrays exactly as ptm_get_history (+ ptm_get_history_invtemps;
 * invtemps may be NULL while the ladder is fixed) and ptm_get_map returned them */
int ptm_set_history(ptm_engine* e, const double* X, const double* llike, const double* lprior, const int32_t* meta,
                    const double* invtemps);
int ptm_set_map(ptm_engine* e, const double* X, const double* lpost, const double* llike, const double* lprior);
/* MAP of the tracked rungs (ptm_config.map_rungs): chain (local rung r, walker w) at index r*W + w: X[index*dim ..], its
 * log-posterior at the rung's temperature (MH_chain::getMAPlpost / getMAPstate, chain.hh:116-117), llike, lprior.
 * lpost is -1e200 while no valid state was seen.  Any output pointer may be NULL. */
int ptm_get_map(ptm_engine* e, double* X, double* lpost, double* llike, double* lprior);
uint64_t ptm_step_count(ptm_engine* e);

/* ---- measurement ---------------------------------------------------------------------------------------- */
/* HIP events on the engine's stream */
int ptm_timer_start(ptm_engine* e);
int ptm_timer_stop(ptm_engine* e, float* elapsed_ms); /* synchronises on the stop event */
/* per-launch durations of the fused sweep kernel recorded since the last call (cfg.time_kernels); ms == NULL: the records are
 * dropped unread (no event query: a measurement that discards its warm-up records must not leave the device idle meanwhile) */
int ptm_get_kernel_times(ptm_engine* e, float* ms, int capacity, int* count);
/* name of the sweep kernel variant in use (for matching rocprofv3 traces) */
const char* ptm_sweep_kernel_name(ptm_engine* e);
/* what a ptm_step call of this engine launches: one kernel for many steps -- "ladder_steps_kernel<..>" (small ladders, a block per
 * ladder) or "ladder_persistent_kernel<..>" (populations whose workgroups are all resident at once, 1024 at the most; chains in registers) -- or
 * "decide_kernel + <sweep kernel>" per step */
const char* ptm_step_kernel_name(ptm_engine* e);

/* Long ladders of few walkers step through ONE persistent kernel per ptm_step(n) call ("ladder_persistent_kernel<..>" in
 * ptm_step_kernel_name).  A launch of it commits all of its steps or none: if its workgroups cannot all be resident (a shared device)
 * one of them gives up waiting, nothing of the launch is kept, and the engine repeats the steps on the two-launch path at its
 * next look at the device (any getter, setter, ptm_sync) and keeps that path from then on.  out[0] launches of that kernel,
 * out[1] launches that gave up and were repeated, out[2] steps that took its whole-ladder exchange form (counted in diagnostics
 * runs only), out[3] 1 if the kernel is switched off for this engine.  No reference counterpart. */
int ptm_get_ladder_stats(ptm_engine* e, int64_t out[4]);
/* Sums of MH_chain::Ntries and ::Naccept (chain.hh:151-152) over this engine's chains, reduced on the device: a measurement
 * that wants "Metropolis moves made so far" reads 16 bytes instead of two arrays (and leaves the GPU no idle gap to drop
 * its clocks in).  Waits for the engine's stream. */
int ptm_get_counter_sums(ptm_engine* e, int64_t* ntries_sum, int64_t* naccept_sum);
/* The box pre-pass of big-population steps: before the compacted 32-dimension sweep a kernel of its own draws the first 16
 * coordinates of each proposal on the rungs flagged for it and settles the chains whose proposal has left the uniform prior's box
 * there already (a rejection: Ntries + 1); the sweep sees the others.  Results do not depend on it.  out[0] chains it has seen so
 * far, out[1] chains it settled, out[2] local rungs flagged at the last such sweep (out[0..2] are zero until the first sweep that
 * launches the pass, whatever out[3] says: the flags are made then), out[3] 1 if a whole step's sweep of this engine
 * is eligible (all-uniform prior, open bounds, lower-triangular or diagonal factor, fixed ladder, no history).  PTM_BOX_PREFILTER=0
 * in the environment switches the pass off, =1 flags every rung of an eligible sweep; PTM_PREFILTER_GRID=n (n >= 1) caps the pass's
 * grid at n blocks (tests: results and counters do not depend on it).  Waits for the engine's stream.  No reference counterpart. */
int ptm_get_prefilter_counts(ptm_engine* e, int64_t out[4]);
/* What this device gives a plain streaming copy and an f64 fma issue loop right now, on the engine's stream (bench.py prints it
 * beside its roofline: devices of one pool differ by several per cent in the clock they hold under load, and a line without it
 * cannot tell a slow box from a slow kernel).  copy_GBs: bytes read + written by a 16-byte-per-lane copy of copy_bytes / 2 bytes,
 * best of 5; f64_fma_TFs: 2 flops x v_fma_f64 issued by four waves per SIMD on every CU; sclk_MHz: the shader clock held during
 * that loop (s_memtime ticks per s_memrealtime tick x 100 MHz, median over workgroups).  A measurement aid like ptm_timer_*: it
 * reads and writes scratch buffers of its own and touches nothing of the engine's state.  No reference counterpart. */
typedef struct ptm_calibration {
  double copy_GBs, copy_bytes, copy_ms;
  double f64_fma_TFs, fma_ms, sclk_MHz;
  int32_t compute_units, reserved;
} ptm_calibration;
int ptm_calibrate(ptm_engine* e, ptm_calibration* out);

/* ---- effective sample size on the device ------------------------------------------------------------------------------
 * chain::report_effective_samples (chain.cc:126-643) as the facade's ess_estimator restates it (ptmcmc_amd/host/ptmcmc_gpu.hh), for
 * every walker of a recorded rung at once: a series is one chain's saved history, its first nfeat parameters are the features, and
 * the sample of nominal step s is saved row 1 + s / add_every_n if the ring still holds it.  The kernels keep the host
 * estimator's order of operations: ess and nwin / length carry its very bits.  The table of nfeat x windows x lags cells per series is
 * built for chunks of series that fit a workspace of PTM_ESS_WORKSPACE_MB MiB (read per call; default 256), which the engine allocates
 * at the first call and frees when it is destroyed.  The engine calls run on the engine's stream and wait for it.
 * A series' length is its chain's own count of add_state calls (PTM_ARR_NHIST; a rung exchanged twice in a step makes one more, so
 * the walkers of a rung differ): every series gets the windows of its own length, in the same launches; ptm_ess_report groups the
 * series whose lengths lead to the same widths and strides (esslimit < 0: as good as always all of them).
 * PTM_ERR_INVALID: no history ring, rung >= history_rungs, nfeat < 1 or > dim.  PTM_ERR_UNSUPPORTED: a chain of the rung has made more than
 * 2e9 add_state calls ("more than 2e9 steps": the kernels count samples in an int).  No reference counterpart for the population form. */
/* one pass with fixed windows (ess_estimator::windowed) over the saved history of local rung `rung` (< history_rungs), every walker at once */
int ptm_ess_windowed(ptm_engine* e, int rung, int nfeat, int width, int every, int burn, double* ess /*[W]*/, int32_t* nwin /*[W]*/);
/* ess_estimator::report (width doubling / coarse-to-fine stride search of esslimit >= 0), width >= 1, every >= 1 */
int ptm_ess_report(ptm_engine* e, int rung, int nfeat, int width, int every, double esslimit, double* ess /*[W]*/, int32_t* length /*[W]*/);
/* the same on a caller's series, host array series[(t*nseries + s)*nfeat + f], t < n: no engine needed */
int ptm_ess_series_windowed(int device, const double* series, int64_t n, int nseries, int nfeat, int width, int every, int burn, double* ess, int32_t* nwin);
int ptm_ess_series_report(int device, const double* series, int64_t n, int nseries, int nfeat, int width, int every, double esslimit, double* ess, int32_t* length);
/* 1 if the last ptm_ess_* call of this engine ran the device kernels (0 also where the series were too short for one window: nothing to launch) */
int ptm_ess_last_on_device(ptm_engine* e);

/* ---- log-evidence by thermodynamic integration on the device -------------------------------------------------------------
 * parallel_tempering_chains::log_evidence_ratio and the total of the statistics block (chain.cc:1984-2012, 1585-1597) as the
 * facade's evidence_estimator restates them (ptmcmc_amd/host/ptmcmc_gpu.hh), for every walker's ladder at once, on the saved
 * llikes of the history ring.  Chain (rung r, walker w) looks at the last `ilen` of its own add_state calls (PTM_ARR_NHIST):
 * saved rows [1 + (Nhist - ilen) / add_every_n, 1 + (Nhist - 1) / add_every_n) -- the newest saved row is left out and a chain
 * shorter than ilen has no row (count 0, NaN: the reference's 0 / 0).  up[i*W + w] = mean of llike * (beta_i - beta_i+1) over
 * rung i+1's window, down[i*W + w] = -mean of llike * (beta_i+1 - beta_i) over rung i's, with the chains' CURRENT inverse
 * temperatures (the ladder's, or the walker's own once the ladders evolve); log_evidence[w] = sum_i (up_i + down_i) / 2 plus
 * the last pair's term / (beta_Nt-2 / beta_Nt-1 - 1).  Every sum is sequential in the host's order: the host estimator's bits.
 * Runs on the engine's stream and waits for it.  up / down / count may be NULL.
 * PTM_ERR_INVALID: a null engine or output, ilen < 1, no history ring, history_rungs < n_rungs, n_rungs < 2, or a window row
 * the ring no longer holds ("history_capacity must hold the evidence window": the outputs are left untouched).
 * PTM_ERR_UNSUPPORTED: a rung shard (the reference has no MPI form either, chain.cc:1592); walker splits are ordinary engines; a chain
 * that has made more than 2e9 add_state calls ("more than 2e9 steps"; the outputs are left untouched). */
int ptm_log_evidence(ptm_engine* e, int ilen, double* log_evidence /*[W]*/, double* up /*[(Nt-1)*W] or NULL*/,
                     double* down /*[(Nt-1)*W] or NULL*/, int32_t* count /*[Nt*W] or NULL*/);

/* ---- split R-hat across the walkers of a rung on the device ----------------------------------------------------------------
 * The Gelman-Rubin diagnostic on split chains: do the W independent replicas of one rung agree with each other?  As the facade's
 * rhat_estimator states it (ptmcmc_amd/host/ptmcmc_gpu.hh), on the saved rows of the history ring where they lie.  The reference
 * runs one ladder: no reference counterpart.
 *  - The first nfeat parameters are the features; nrows (even, >= 4) saved rows per chain are looked at.
 *  - Walker w's window is its own newest nrows saved rows: newest_w = 1 + (Nhist_w - 1) / add_every_n (PTM_ARR_NHIST: the row the
 *    effective-sample-size calls assign to nominal step Nhist - 1, the exclusive end of the evidence window), rows
 *    newest_w - nrows + 1 .. newest_w in ascending order.  Row 0, the start state, is never part of it.  The walkers of a rung may
 *    differ in Nhist; each uses its own window, all of one length.
 *  - The window's first and second half, n = nrows / 2 rows each, are sequences 2w and 2w + 1: m = 2W sequences.
 *  - Per sequence k and feature f, sequentially in row order: mean_k = (sum x) / n; then, in a second walk over the same rows,
 *    var_k = (sum (x - mean_k) * (x - mean_k)) / (n - 1).
 *  - Per feature, sequentially over k = 0 .. m - 1: M = (sum mean_k) / m; between = n * (sum (mean_k - M)^2) / (m - 1);
 *    within = (sum var_k) / m; var_plus = ((n - 1) / n) * within + between / n; rhat = sqrt(var_plus / within).
 * Operations run as written (multiply, then add; no contraction), so the answers carry the host estimator's bits.  A constant
 * feature gives the formula's IEEE result (NaN or infinity): nothing is special-cased.
 * Outputs: rhat[nfeat]; mean (M), within, between [nfeat] or NULL; seq_mean, seq_var [(2*W)*nfeat] ([k*nfeat + f]) or NULL -- with
 * them a caller can pool walker splits that run as separate engines.
 * ptm_rhat runs on the engine's stream and waits for it.  ptm_rhat_series is the same on a caller's series, host array
 * series[(t*nseries + s)*nfeat + f], t < n, with nseries in place of W and the newest nrows of the n rows as every window: no engine needed.
 * PTM_ERR_INVALID: a null engine or rhat, no history ring, rung >= history_rungs, nfeat < 1 or > dim, nrows odd or < 4, a chain with
 * fewer than nrows saved rows behind the start state, or a window row the ring no longer holds ("history_capacity must hold the
 * window": the outputs are left untouched).  PTM_ERR_UNSUPPORTED: a chain of the rung has made more than 2e9 add_state calls. */
int ptm_rhat(ptm_engine* e, int rung, int nfeat, int nrows, double* rhat /*[nfeat]*/, double* mean, double* within, double* between /*[nfeat] or NULL*/,
             double* seq_mean, double* seq_var /*[2*W*nfeat] or NULL*/);
int ptm_rhat_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, double* rhat /*[nfeat]*/, double* mean, double* within,
                    double* between /*[nfeat] or NULL*/, double* seq_mean, double* seq_var /*[2*nseries*nfeat] or NULL*/);

/* ---- pooled posterior mean and covariance of a rung on the device ----------------------------------------------------------
 * What the posterior is: the mean and the covariance of the first nfeat parameters, pooled over the W independent replicas of one
 * recorded rung, from the saved rows of the history ring where they lie.  As the facade's moments_estimator states it
 * (ptmcmc_amd/host/ptmcmc_gpu.hh).  The reference's write_covariance / read_covariance are empty (ptmcmc.cc:761-768): no counterpart.
 *  - Walker w's window is its own newest nrows saved rows in ascending row order, ptm_rhat's rule: newest_w = 1 + (Nhist_w - 1) /
 *    add_every_n, rows newest_w - nrows + 1 .. newest_w; row 0, the start state, is never part of it; each walker uses its own Nhist.
 *    nrows >= 1; N = W * nrows samples, N >= 2.
 *  - G = 64 walkers form a block: block b holds walkers 64 b .. min(64 b + 63, W - 1).
 *  - Sums, in this order, every one sequential:
 *      s_w[f] = sum over the window's rows of x[f];  S_b[f] = sum over block b's walkers of s_w[f];  S[f] = sum over the blocks of S_b[f];
 *      mean[f] = S[f] / N;
 *      for each pair i <= j, with d_i = x[i] - mean[i]:  c_w[i,j] = sum over the rows of d_i * d_j;  C_b[i,j] = sum over the block's
 *      walkers of c_w[i,j];  C[i,j] = sum over the blocks of C_b[i,j];
 *      cov[i,j] = cov[j,i] = C[i,j] / (N - 1).
 *    The two-level order over the walkers is part of the definition: it lets the reduction run in parallel with defined bits.
 * Operations run as written (multiply, then add; no contraction), so the answers carry the host estimator's bits.  A constant
 * feature gives an exact zero row and column: nothing is special-cased.  Correlations and standard deviations are the caller's to
 * form from cov.
 * Outputs: mean[nfeat]; cov[nfeat*nfeat] (row-major, both triangles) or NULL; var[nfeat] (the diagonal of cov: the diagonal pairs'
 * sums / (N - 1)) or NULL; walker_sum[W*nfeat] (s_w, [w*nfeat + f]) or NULL and count (N) or NULL -- with them a caller can pool
 * walker splits that run as separate engines.  The covariance is offered for nfeat <= 128; above that cov must be NULL.
 * ptm_moments runs on the engine's stream and waits for it; its workspace is kept between calls.  ptm_moments_series is the same on
 * a caller's series, host array series[(t*nseries + s)*nfeat + f], t < n, with nseries in place of W and the newest nrows of the
 * n rows as every window: no engine needed.
 * PTM_ERR_INVALID: a null engine, series or mean, no history ring, rung >= history_rungs, nfeat < 1 or > dim, nrows < 1, N < 2, a
 * chain with fewer than nrows saved rows behind the start state, or a window row the ring no longer holds ("history_capacity must
 * hold the window").  PTM_ERR_UNSUPPORTED: a chain of the rung has made more than 2e9 add_state calls; cov with nfeat > 128.
 * The outputs are left untouched on every failure.  Not between ptm_batch_begin and ptm_batch_end.  The per-walker pair sums pass
 * through the workspace a group of whole blocks of walkers at a time (256 MiB at most); PTM_MOMENTS_GROUP=n in the environment forces
 * the walkers of a group (tests): the bits do not depend on it. */
int ptm_moments(ptm_engine* e, int rung, int nfeat, int nrows, double* mean /*[nfeat]*/, double* cov /*[nfeat*nfeat] or NULL*/,
                double* var /*[nfeat] or NULL*/, double* walker_sum /*[W*nfeat] or NULL*/, int64_t* count /*N, or NULL*/);
int ptm_moments_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, double* mean /*[nfeat]*/,
                       double* cov /*[nfeat*nfeat] or NULL*/, double* var /*[nfeat] or NULL*/, double* walker_sum /*[nseries*nfeat] or NULL*/,
                       int64_t* count /*N, or NULL*/);
/* the rows of a window one staging tile of the covariance kernel holds (what a test builds its edge sizes around); 0: nfeat outside 1..128 */
int ptm_moments_tile_rows(int nfeat);

/* ---- every rung's Gaussian proposal from its own sampled covariance, on the device -------------------------------------------
 * What user_gaussian_prop::check_update / reset_dist do for one chain in the reference (proposal_distribution.cc:340-441), for a
 * range of recorded rungs at once: the moments and the eigen-decompositions do not leave the device.
 *
 * ptm_moments_rungs is ptm_moments for the local rungs first_rung .. first_rung + n_rungs - 1, all below history_rungs: rung r's
 * answers at mean[r*nfeat], cov[r*nfeat*nfeat], var[r*nfeat] are the bits ptm_moments gives for that rung (the same window rule, the
 * same three-level sequential sums, the same two passes: the same kernels, one rung after the other on the engine's stream), and the
 * call waits once.  It refuses what ptm_moments refuses, for the whole call: when one rung's window is not there every output is
 * left untouched.  count: N = W * nrows, the same for every rung.
 *
 * ptm_eigen_factors restates the facade's gaussian_prop::eigen_factor (ptmcmc_amd/host/ptmcmc_gpu.hh) for n_mat symmetric n x n
 * matrices, row-major, one after the other in cov; no engine needed.  For every matrix:
 *  - detail::jacobi_eigen as written there: Q = 1; at most 100 sweeps; a sweep begins with off = the sequential sum over p < q, in that
 *    order, of A[p][q]^2 and ends the iteration when off < 1e-300; then for every p < q in that order, unless |A[p][q]| < 1e-300:
 *      theta = (A[q][q] - A[p][p]) / (2 A[p][q]);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta^2 + 1));  c = 1 / sqrt(t^2 + 1);
 *      s = t c;  for every k: (A[k][p], A[k][q]) <- (c a - s b, s a + c b);  then for every k the same on (A[p][k], A[q][k]);  then for
 *      every k the same on (Q[k][p], Q[k][q]).  Both triangles of the full matrix are rotated: nothing is mirrored.
 *  - its swap sort: order = 0 .. n-1; for i, for j > i: if A[order[j]][order[j]] < A[order[i]][order[i]] swap the two entries;
 *    lambda[j] = A[order[j]][order[j]], V[i][j] = Q[i][order[j]].
 *  - factors[i*n + j] = V[i][j] * sqrt(lambda[j] > 0 ? lambda[j] : 0).
 * Operations run as written (correctly rounded roots and quotients, multiply then add, no contraction): factors and lambda carry the
 * host's bits, NaN where the host has NaN.  sweeps: the sweeps that rotated (100: the limit was reached).  1 <= n <= 128, n_mat >= 1.
 * PTM_ERR_INVALID: a null cov or factors, n or n_mat out of range.
 *
 * ptm_adapt_proposals replaces the Gaussian factor of every rung of the range by one made from that rung's own samples: every walker's
 * newest nrows saved rows, all D parameters, pooled as ptm_moments pools them.
 *  - PTM_PROP_DENSE: factor = scale * F, one multiply per element after F is formed, F the eigen factor (above) of the rung's pooled
 *    covariance.  D <= 128.
 *  - PTM_PROP_DIAG: sigma_d = scale * sqrt(var_d), ptm_moments' variances; no covariance is formed: any D.
 * status[r]: 0: installed; 1: kept, an entry of the covariance (DIAG: a variance) is not finite; 2: kept, the smallest eigenvalue
 * (DIAG: a variance) is not above 0.  A kept rung goes on with the factor it had.  An installed rung is in exactly the state
 * ptm_set_proposal_rung(e, r, factor, -1) leaves it in (the two share their packing).  factors_out, when given, receives what was
 * computed for every rung, kept ones included: [n_rungs][D*D] row-major (DENSE) or [n_rungs][D] (DIAG).  one_d_frac, mixtures, adaptive
 * sets' state, differential evolution and the prior-draw member are untouched.  A common choice of scale is 2.38 / sqrt(D).
 * PTM_ERR_INVALID: a null engine or status; no ptm_set_proposals yet; a range that is not inside history_rungs; scale not finite or not
 * above 0; nrows < 1 or W * nrows < 2; whatever ptm_moments refuses about windows; user proposals, host-side or device, are set (the
 * factors are not read then).  PTM_ERR_UNSUPPORTED: PTM_PROP_LOWER; DENSE with D > 128; a call between ptm_batch_begin and
 * ptm_batch_end.  Everything is checked before anything changes: after a failure the engine steps on as before (but for a failed copy of
 * the device runtime during the install itself, PTM_ERR_HIP: rungs installed before it stay installed and status is not written).  On a rung shard the
 * rungs are the local ones; on a walker split every engine adapts to its own walkers. */
int ptm_moments_rungs(ptm_engine* e, int first_rung, int n_rungs, int nfeat, int nrows, double* mean /*[n_rungs*nfeat]*/,
                      double* cov /*[n_rungs*nfeat*nfeat] or NULL*/, double* var /*[n_rungs*nfeat] or NULL*/, int64_t* count /*N, or NULL*/);
int ptm_eigen_factors(int device, const double* cov /*[n_mat][n*n] row-major*/, int n_mat, int n, double* factors /*[n_mat][n*n] row-major*/,
                      double* lambda /*[n_mat][n] or NULL*/, int32_t* sweeps /*[n_mat] or NULL*/);
int ptm_adapt_proposals(ptm_engine* e, int first_rung, int n_rungs, int nrows, double scale, int32_t* status /*[n_rungs]*/,
                        double* factors_out /*[n_rungs][D*D | D] or NULL*/);

/* ---- exact posterior quantiles of a rung on the device ----------------------------------------------------------------------
 * What every user writes down at the end of a run: the median and the credible interval of each parameter -- the right summary of
 * a skewed or two-humped marginal, where the mean and the variance are not.  As the facade's quantile_estimator states it
 * (ptmcmc_amd/host/ptmcmc_gpu.hh).  The reference runs one ladder and writes no quantiles: no counterpart.
 *  - Sample.  The sample of feature f (f < nfeat, the first nfeat parameters) of one recorded rung is pooled over its W walkers:
 *    walker w contributes its own newest nrows saved rows, ptm_moments' window: newest_w = 1 + (Nhist_w - 1) / add_every_n, rows
 *    newest_w - nrows + 1 .. newest_w; row 0, the start state, is never part of it; each walker uses its own Nhist.  nrows >= 1;
 *    N = W * nrows >= 1 samples.  A single sample is its own every quantile.
 *  - Order.  Values are ordered by the 64-bit key  u ^ (u >> 63 ? ~0 : 1 << 63)  of their bit pattern u: the usual order of the
 *    reals, with -0 before +0 and -inf / +inf at the ends.  The sorted sample is s_0 <= ... <= s_{N-1}.  Equal keys are equal bits,
 *    so ties are no problem.
 *  - Quantile.  For a probability p in [0, 1], in double arithmetic as written:
 *      h = (double)(N - 1) * p;  lo = floor(h);  hi = min(lo + 1, N - 1);  g = h - lo;
 *      q = (g == 0) ? s_lo : s_lo + g * (s_hi - s_lo)      (multiply, then add; no contraction)
 *    the linear rule, numpy's default (Hyndman and Fan type 7).  x_lo = s_lo and x_hi = s_hi are returned beside it: the exact
 *    order statistics are x_lo, and the bracket is what a caller needs to pool or to check.  p = 0 and p = 1 give the minimum and
 *    the maximum.  Nothing is special-cased: an infinite bracket gives the formula's IEEE result.
 * nq in 1..32; probs need not be sorted or distinct.  Outputs: q[nq*nfeat] ([k*nfeat + f]); x_lo, x_hi [nq*nfeat] or NULL; count
 * (N) or NULL.  Every output carries the bits of quantile_estimator, which sorts the keys with std::sort and applies the formula;
 * the device selects by radix digits (ptm_quantiles_kernels.hpp) -- the definition has no summation order in it, an order statistic
 * is a value of the sample, so the algorithm is free.  Counts and ranks are 64-bit everywhere.
 * ptm_quantiles runs on the engine's stream and waits for it; its workspace is kept between calls.  ptm_quantiles_series is the
 * same on a caller's series, host array series[(t*nseries + s)*nfeat + f], t < n, with nseries in place of W and the newest nrows
 * of the n rows as every window: no engine needed.
 * PTM_ERR_INVALID: a null engine, series, probs or q, no history ring, rung >= history_rungs, nfeat < 1 or > dim, nrows < 1, nq
 * outside 1..32, a p outside [0, 1] or NaN, a chain with fewer than nrows saved rows behind the start state, a window row the ring
 * no longer holds ("history_capacity must hold the window"), and for the series call a NaN in the series (looked for on the host
 * before anything is queued; infinities are allowed).  PTM_ERR_UNSUPPORTED: a chain of the rung has made more than 2e9 add_state
 * calls.  The outputs are left untouched on every failure.  Not between ptm_batch_begin and ptm_batch_end.
 * In the environment (tests, tools/quantiles_probe.py), PTM_QUANTILES_PATH=ring|packed chooses whether every pass walks the ring (the default)
 * or the remaining candidates are copied into the workspace once they fit, PTM_QUANTILES_PACK_BYTES=n bounds that copy (256 MiB at
 * most; candidates that do not fit keep the passes on the ring) and PTM_QUANTILES_TILE=n sets the features of an LDS tile: the
 * bits do not depend on them. */
int ptm_quantiles(ptm_engine* e, int rung, int nfeat, int nrows, int nq, const double* probs /*[nq]*/,
                  double* q /*[nq*nfeat], [k*nfeat + f]*/, double* x_lo, double* x_hi /*[nq*nfeat] or NULL*/, int64_t* count /*N, or NULL*/);
int ptm_quantiles_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, int nq, const double* probs,
                         double* q, double* x_lo, double* x_hi, int64_t* count);
/* the passes of the last call that walked the ring and that walked the packed copy (what a test of a forced path looks at);
 * returns 1 if the call packed */
int ptm_quantiles_last_path(int* ring_passes, int* packed_passes);

/* ---- corner-plot histograms of a rung on the device ---------------------------------------------------------------------------
 * What every user looks at at the end of a run: the corner plot -- the 1-D marginal histogram of every parameter and the 2-D
 * histogram of every pair of parameters.  As the facade's histogram_estimator states it (ptmcmc_amd/host/ptmcmc_gpu.hh).  The
 * reference bins on the host (python/corner_with_covar.py: np.histogram, np.histogram2d); the counts here are numpy's.
 *  - Sample.  ptm_quantiles' sample: the first nfeat parameters of one recorded rung, pooled over its W walkers; walker w
 *    contributes its own newest nrows saved rows: newest_w = 1 + (Nhist_w - 1) / add_every_n, rows newest_w - nrows + 1 .. newest_w;
 *    row 0, the start state, is never part of it; each walker uses its own Nhist.  nrows >= 1; N = W * nrows >= 1 samples.
 *  - Edges.  For feature f with lo[f] < hi[f], in double arithmetic as written (multiply, then add; no contraction):
 *      step = (hi - lo) / (double)nbins;   edge_k = lo + (double)k * step  for k < nbins;   edge_nbins = hi
 *    np.linspace(lo, hi, nbins + 1) bit for bit.  The edges must be finite and strictly increasing: otherwise "the range cannot
 *    hold nbins bins" (numpy's own refusal).
 *  - Bin.  x lies in bin k if and only if edge_k <= x < edge_{k+1}, the last bin closed: x == hi lies in bin nbins - 1.  -0.0
 *    compares as 0.  x < lo adds to below[f], x > hi to above[f], a NaN to neither.  The definition is the edges: any algorithm
 *    that lands every double in the bin the edges give is correct.
 *  - h1[f*nbins + k]: the samples of feature f in bin k.
 *  - h2.  Pairs i < j in row-major order of the upper triangle: p = i*nfeat - i*(i+1)/2 + (j - i - 1), npairs = nfeat*(nfeat-1)/2.
 *    h2[(p*nbins + ki)*nbins + kj]: the rows whose feature i lies in bin ki and whose feature j lies in bin kj.  A row with
 *    either of the two values outside its range is left out of that pair only (np.histogram2d's rule).  nfeat == 1 has no pairs:
 *    h2 is not touched.
 * Counts are 64-bit.  They are integers, so there is no order of summation in the definition and every output is the host
 * estimator's to the last unit; counts from walker splits that run as separate engines with the same lo, hi and nbins simply add.
 * Outputs: h1[nfeat*nbins]; h2[npairs*nbins*nbins] or NULL (no pairs asked for); below, above [nfeat] or NULL; count (N) or NULL.
 * ptm_histograms runs on the engine's stream and waits for it; its workspace is kept between calls.  ptm_histograms_series is the
 * same on a caller's series, host array series[(t*nseries + s)*nfeat + f], t < n, with nseries in place of W and the newest nrows
 * of the n rows as every window: no engine needed.
 * PTM_ERR_INVALID: a null engine, series, lo, hi or h1, no history ring, rung >= history_rungs, nfeat < 1 or > dim, nrows < 1,
 * nbins outside 1..128, a range that is not finite or not lo < hi, edges that are not finite and strictly increasing, a chain with
 * fewer than nrows saved rows behind the start state, a window row the ring no longer holds ("history_capacity must hold the
 * window"), and for the series call a NaN in the series (looked for on the host before anything is queued; infinities are
 * allowed).  PTM_ERR_UNSUPPORTED: npairs * nbins * nbins > 2^25 with h2 asked for (256 MiB of counters), a chain of the rung with
 * more than 2e9 add_state calls.  The outputs are left untouched on every failure.  Not between ptm_batch_begin and ptm_batch_end.
 * In the environment (tests, tools/histograms_probe.py), PTM_HIST_TILE=n sets the pairs of an LDS tile of the 2-D kernel and
 * PTM_HIST_MAP=pairs|rows how its adds are dealt to the lanes (ptm_histograms_kernels.hpp): the counts do not depend on them. */
int ptm_histograms(ptm_engine* e, int rung, int nfeat, int nrows, int nbins, const double* lo /*[nfeat]*/, const double* hi /*[nfeat]*/,
                   int64_t* h1 /*[nfeat*nbins]*/, int64_t* h2 /*[npairs*nbins*nbins] or NULL*/,
                   int64_t* below, int64_t* above /*[nfeat] or NULL*/, int64_t* count /*N, or NULL*/);
int ptm_histograms_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, int nbins, const double* lo, const double* hi,
                          int64_t* h1, int64_t* h2, int64_t* below, int64_t* above, int64_t* count);
/* the pairs of a tile, the tiles and the mapping (0: pairs, 1: rows) of the 2-D kernel in the last call (what a test of a forced
 * tile looks at); returns the tiles, 0 if the call counted no pairs */
int ptm_histograms_last_launch(int* tile_pairs, int* tiles, int* map);

/* ---- exact nearest-neighbour squared distances on the device --------------------------------------------------------------
 * The search inside the k-NN Kullback-Leibler estimator of Perez-Cruz with which the reference tests a proposal's invariance
 * (test_proposal.hh:350-464), as the facade's kl_estimator states it (ptmcmc_amd/host/ptmcmc_gpu.hh): for every point i of P the
 * smallest squared distance to a point of Q.  The reference turns to approximate neighbours at the sampler's sizes; this search is
 * exact, brute force, O(nP nQ dim).
 *  - The distance is state::dist2 (states.cc:207-233): per dimension diff = |b - a|; in a wrapped dimension also the same with both
 *    points shifted down by (xmax - xmin) / 2 and wrap-enforced, the smaller of the two; the diff * diff are summed in dimension
 *    order, multiply, then add (no contraction): nnd2[i] carries the bits of kl_estimator's one_nnd2 / all_nnd2.
 *  - same_set = 1: Q is P and index i is skipped for query i (all_nnd2); a duplicate of point i elsewhere still gives 0.
 *  - Host arrays, row-major [n][dim]; no engine needed.  wrapped NULL: no dimension is wrapped; xmin, xmax are read where wrapped.
 * PTM_ERR_INVALID (nnd2 is left untouched): a null P, Q or nnd2, nP < 1 or nQ < 1, same_set with nQ != nP or nP < 2, dim < 1, a wrapped
 * dimension without finite xmin < xmax, a non-finite coordinate (looked for on the host before anything is queued).
 * PTM_ERR_UNSUPPORTED: dim > 128 (the host estimator serves there).  The call works in one device allocation and on a stream of its
 * own, both kept for the next call (an allocation above 256 MiB is given back), and waits for that stream only; calls are serialised.  PTM_KL_SPLITS=n in the environment forces the number of
 * parts the searched set is split into (tests). */
int ptm_nn_dist2(int device, const double* P, int64_t nP, const double* Q, int64_t nQ, int dim, const int32_t* wrapped /*[dim] or NULL*/,
                 const double* xmin, const double* xmax /*[dim], read where wrapped*/, int same_set /*1: Q is P, index i is skipped for query i*/,
                 double* nnd2 /*[nP]*/);
/* the points of the searched set one tile of the search holds (what a test builds its edge sizes around) */
int ptm_nn_dist2_tile(void);

/* ---- verification hooks (used by tests/ only; evaluate device functions on arrays) ---------------------- */
enum { PTM_FN_LOG = 0, PTM_FN_EXP = 1, PTM_FN_SIN_0_PI = 2, PTM_FN_COS_HPI = 3, PTM_FN_SQRT = 4, PTM_FN_DIV = 5,
       PTM_FN_SQRT_RAW = 6 };
int ptm_debug_eval(int device, int fn, const double* a, const double* b, double* out, int n);
int ptm_debug_philox(int device, uint64_t seed, int tag, uint32_t stream, uint64_t step, uint32_t block, uint32_t out[4]);
int ptm_debug_boxmuller(int device, const uint32_t* k1, const uint32_t* k2, double* z0, double* z1, int n);
/* exhaustive scan of all 2^32 Box-Muller radius arguments a = -2 ln((k+.5)/2^32): for how many is the hot path's
 * unscaled Newton square root NOT the correctly rounded one (or a outside its domain).  Must be 0. */
int ptm_debug_sqrt_scan(int device, uint64_t* mismatches);
/* exhaustive scans of the box pre-pass's single-precision Box-Muller against the sweep's: out[0] max |r_f32 - r| over all 2^32 first
 * arguments, out[1] the largest r_f32, out[2] how many gave a NaN; out[3] max |sin_f32 - sin|, |cos_f32 - cos| over all 2^32 second
 * arguments, out[4] how many gave a NaN; out[5], out[6] the margin's constants PTM_BP_DZ and PTM_BP_F32_SLACK; out[7] 0. */
int ptm_debug_boxmuller_f32_scan(int device, double out[8]);
/* evaluate lprior / llike of arbitrary states with the engine's problem description: X[n][D] */
/* device-memory helpers for callers without a GPU array library (tests, tools) */
int ptm_dev_alloc(size_t bytes, void** out);
int ptm_dev_free(void* p);
int ptm_dev_copy(void* dst, const void* src, size_t bytes); /* any direction, synchronous */
int ptm_debug_evaluate(ptm_engine* e, const double* X, int n, int32_t* valid, double* X_enforced, double* lprior,
                       double* llike);

#ifdef __cplusplus
}
#endif
#endif /* PTM_ENGINE_H */
