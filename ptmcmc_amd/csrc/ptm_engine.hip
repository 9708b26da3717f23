// ptm_engine.hip -- host side of the C ABI declared in include/ptm_engine.h.
//
// Thin by design: it owns device memory, packs the problem description the way the kernels want it,
// and enqueues kernels on one HIP stream.  No algorithmic work happens on the host; there is no CPU
// fallback -- without a gfx950 device every entry point that computes returns PTM_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ptm_engine.h"
#include "ptm_aux_kernels.hpp"
#include "ptm_box_prefilter.hpp"
#include "ptm_count_limit.hpp"
#include "ptm_de_mfma_kernel.hpp"
#include "ptm_devlike_kernels.hpp"
#include "ptm_devprior_kernels.hpp"
#include "ptm_devprop_kernels.hpp"
#include "ptm_eigen_kernels.hpp"
#include "ptm_ess_kernels.hpp"
#include "ptm_evidence_kernels.hpp"
#include "ptm_histograms_kernels.hpp"
#include "ptm_kl_kernels.hpp"
#include "ptm_launch.hpp"
#include "ptm_moments_kernels.hpp"
#include "ptm_quantiles_kernels.hpp"
#include "ptm_rhat_kernels.hpp"
#include "ptm_shard_rccl.hpp"

using namespace ptm;

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(x)                                                                                         \
  do {                                                                                                    \
    hipError_t _e = (x);                                                                                  \
    if (_e != hipSuccess) return fail(PTM_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// host staging buffers of the callback path live in pinned memory: a hipMemcpyAsync from / to pageable memory is staged
// by the runtime (22 us per copy measured against ~5)
template <class T>
struct PinnedAlloc {
  typedef T value_type;
  PinnedAlloc() {}
  template <class U> PinnedAlloc(const PinnedAlloc<U>&) {}
  T* allocate(size_t n) {
    void* p = nullptr;
    if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) throw std::bad_alloc();
    return (T*)p;
  }
  void deallocate(T* p, size_t) { (void)hipHostFree(p); }
  template <class U> bool operator==(const PinnedAlloc<U>&) const { return true; }
  template <class U> bool operator!=(const PinnedAlloc<U>&) const { return false; }
};
template <class T> using pinned_vector = std::vector<T, PinnedAlloc<T>>;

struct ptm_engine {
  ptm_config cfg;
  int D = 0, DP = 0, Nt = 0, r0 = 0, nloc = 0, W = 0, Nc = 0, ms = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  uint64_t step = 0;
  // device state
  double *xdev = nullptr, *ll = nullptr, *lp = nullptr;   // rows [Nc][DP] (read and written through xrows(), below) and per-chain scalars, updated in place
  int *ntries = nullptr, *naccept = nullptr, *last_type = nullptr, *err = nullptr;
  int *arr_below = nullptr, *arr_above = nullptr;
  int *mv_src = nullptr, *mv_dst = nullptr, *mv_n = nullptr;   // per-ladder move lists (exchange kernel -> move kernel)
  unsigned int* nhist = nullptr;
  long long* swap_cnt = nullptr;   // [W][Nt-1][2] {tries, accepts}
  unsigned char* touch = nullptr;
  Hist hist = {0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};   // optional history ring (ptm_config.history_rungs)
  MapT map = {0, 0, nullptr, nullptr, nullptr, nullptr};       // optional MAP tracking (ptm_config.map_rungs)
  int* swap_log = nullptr;   // [PTM_LOG_RING][W][ms] candidate logs of the last steps; the swap counters lag behind by
  int log_head = 0, log_pending = 0;   //  the `log_pending` newest of them (fold_swap_log)
  int row_cap = 0;           // row slots per boundary message
  // device problem description
  int *blo = nullptr, *bhi = nullptr, *ptype = nullptr;
  double *bmin = nullptr, *bmax = nullptr, *plo = nullptr, *phi = nullptr, *pcoef = nullptr;
  double *P2 = nullptr, *mean = nullptr, *beta = nullptr, *prop = nullptr, *prop_tiles = nullptr, *P2_tiles = nullptr, *box_row = nullptr, *onedfrac = nullptr, *mix = nullptr;
  int mix_K = 0;
  // differential evolution on the device (ptm_set_proposal_de)
  bool de_on = false;
  ptm_de_params de = {0, 0, 0, 0};
  int de_init_extra = 0;
  double *de_init = nullptr, *de_hast = nullptr;
  int* de_type = nullptr;
  // adaptive proposal set (ptm_set_proposal_adaptive): the set's shape and rates; one device allocation each for the leaves
  // [nloc][L][2], the per-chain doubles (weights | thresholds, [L][Nc] each) and ints (repeat bits | outcome counts, [2][Nc] each)
  bool ada_on = false;
  ptm_adaptive_set ada = {0, -1, 0, 0, 0};
  double *ada_leaf = nullptr, *ada_dbl = nullptr;
  int* ada_int = nullptr;
  // the member of the current set that draws from the prior (ptm_set_proposal_prior_draw), or -1; which (top) members of the current set
  // have a negative scale on some rung -- differential evolution's mark
  int prior_member = -1;
  std::vector<char> set_neg;
  // evolving ladders (ptm_set_evolve_temps): per-ladder inverse temperatures [W][Nt] and their chain-indexed image [Nc]
  double evolve_rate = 0, evolve_cut = -1;
  double *beta_w = nullptr, *betaC = nullptr, *beta_add = nullptr;
  bool betaC_stale = false;   // the chain-indexed image of evolving temperatures lags the ladder-major one (ensure_betaC)
  // host copies / flags
  int has_bounds = 0, origin_valid = 1, all_uniform = 1, has_mean = 0, have_target = 0, have_ladder = 0,
      have_prop = 0, have_state = 0, prop_kind = KIND_DIAG, prop_stride = 0, any_oned = 0, bounds_box = 1;
  double lprior_const = 0, like0 = 0, thresh = 0;
  bool lp_is_const = false;   // every chain's lprior equals lprior_const (checked when states are set; sweeps keep it so)
  std::vector<double> h_beta;
  std::vector<int> h_ptype;
  std::vector<double> h_plo, h_phi;
  ptm_loglike_batch_fn cb = nullptr;
  void* cb_user = nullptr;
  ptm_logprior_batch_fn prior_cb = nullptr;   // host-evaluated prior (ptm_set_prior_callback)
  void* prior_user = nullptr;
  // host-side proposals (ptm_set_proposal_callback)
  ptm_propose_batch_fn pcb = nullptr;
  ptm_proposal_result_fn pres = nullptr;
  void* pcb_user = nullptr;
  // device proposals (ptm_set_proposal_device; ptm_devprop_kernels.hpp): the user's functions, and buffers that belong to this path
  // alone (the device likelihood's pack runs later in the same step with its own count and row -> chain index).  By row: the packed
  // current states and the proposals in natural order [Nc][D], ids, log-Hastings ratios, types, validity, outcomes, the count, the
  // row -> chain index and the pack's chunk totals; by chain: what the sweep kernel reads under host_prop
  ptm_propose_device_fn dpfn = nullptr;
  ptm_proposal_result_device_fn dpres = nullptr;
  void* dp_user = nullptr;
  double *dp_xcur = nullptr, *dp_xnew = nullptr, *dp_hast_k = nullptr;
  int32_t *dp_rung = nullptr, *dp_walker = nullptr, *dp_type_k = nullptr, *dp_valid_k = nullptr, *dp_acc_k = nullptr, *dp_count = nullptr;
  int *dp_rows = nullptr, *dp_chunks = nullptr;
  double *dp_xprop = nullptr, *dp_hastings = nullptr;
  int* dp_htype = nullptr;
  unsigned char *dp_hvalid = nullptr, *dp_acc_out = nullptr;
  // device likelihood (ptm_set_target_device): the user's function enqueues on the stream; its batch buffers (owned or the
  // caller's), the count, the row -> chain index, the chunk totals of the pack, hand-over buffers in device memory whatever the
  // population, and the best log-posterior seen with its state {lpost, x[D]}
  ptm_loglike_device_fn dfn = nullptr;
  void* dfn_user = nullptr;
  double *dl_x = nullptr, *dl_ll = nullptr;
  bool dl_own_x = false, dl_own_ll = false;
  int32_t* dl_count = nullptr;
  int *dl_rows = nullptr, *dl_chunks = nullptr;
  double *dl_xprop = nullptr, *dl_lprior_new = nullptr, *dl_llike_new = nullptr, *dl_best = nullptr;
  unsigned char* dl_gate = nullptr;
  // device prior (ptm_set_prior_device; ptm_devprior_kernels.hpp): the user's function and this path's own batch (the likelihood's pack
  // runs later in the same step with its own count and row -> chain index, and its batch may be the caller's memory): the packed valid
  // proposals [Nc][D], their log-priors, the count, the row -> chain index and the pack's chunk totals
  ptm_logprior_device_fn dprior = nullptr;
  void* dprior_user = nullptr;
  double *pr_x = nullptr, *pr_lp = nullptr;
  int32_t* pr_count = nullptr;
  int *pr_rows = nullptr, *pr_chunks = nullptr;
  // compacted sweep (partition_kernel): per-rung lists of the walkers that move, their counts; touched = an exchange phase
  // ran since the last sweep
  int *cidx = nullptr, *ccnt = nullptr;
  // box pre-pass (ptm_box_prefilter.hpp): the lists of the flagged rungs (partition_kernel writes them there instead), the rungs'
  // flags, {chains seen, chains settled}; on the host the standard deviations of the first 16 coordinates of each rung's proposal,
  // from which -- with the prior box -- the flags are made when any of the two has changed (pf_dirty)
  int *pidx = nullptr, *pcnt = nullptr;
  unsigned char *pf_flag = nullptr, *h_pf_flag = nullptr;   // (h_pf_flag: pinned, so that the flags' upload waits for nothing)
  unsigned long long* pf_counts = nullptr;
  std::vector<double> pf_sigma;
  // ... and for the single-precision kernel the margins of those coordinates (ptm_sweep_plan.hpp: prefilter_margins), made beside the
  // sigmas; their image for the kernel, the faces' slack added and rounded up to float, is uploaded with the flags (pf_margin, staged in
  // pinned h_pf_margin)
  std::vector<double> pf_margin_nat;
  float *pf_margin = nullptr, *h_pf_margin = nullptr;
  bool pf_dirty = true;
  int pf_flagged = 0, pf_grid = 0;
  bool touched = false;
  bool compact_step = false;   // this step's (partial) sweeps are compacted
  // row labels (ptm_decide.hpp): [Nc] the rung slot of xdev that holds each chain's row.  Only the exchange kernel and the compacted
  // sweep of a labelled step know them; everybody else reaches the rows through xrows(), which puts them back first (flush_rows).
  unsigned short* rowof = nullptr;
  bool rows_labelled = false;   // the labels may differ from the identity
  bool label_step = false;      // this step's exchange phase went by labels: its sweep must be the compacted one
  ShardComm* shard = nullptr;   // native RCCL sharding (ptm_shard_*)
  // recovery of runs longer than a halo (ptm_set_shard_map): the shards' ends, the nominal halo, per-ladder flags | count
  int* shard_ends = nullptr;
  int nshards = 0, halo_nominal = 0;
  int* redo_flag = nullptr;     // [W] flags, then [1] the count
  long long redo_total = 0;     // ladders decided by the gathered second pass so far
  // persistent ladder kernel (ptm_ladder_kernel.hpp): published rows / llikes / lpriors by step parity, the workgroups' flags
  double *pub_x = nullptr, *pub_ll = nullptr, *pub_lp = nullptr;   // (one allocation: pub_x)
  int *lad_flags = nullptr, *lad_ctl = nullptr;                     // (one allocation: lad_flags)
  long long* lad_prof = nullptr;
  int lad_capacity[2][32] = {{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
                             {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};   // workgroups of each build of that kernel [diagonal][FL] the device holds at once (-1: not asked yet)
  long long ladder_launches = 0, ladder_whole_steps = 0;   // launches of that kernel; steps (of walker 0) whose exchange phase needed the whole ladder
  // A launch of that kernel commits all of its steps or none (ptm_ladder_kernel.hpp) and is ASYNCHRONOUS: the host learns at its
  // next look (ladder_settle) whether the launches since the last look were committed -- the device keeps the number of the last one
  // that was (err[2]) -- and, if one gave up, repeats its steps and its successors' on the two-launch path.
  struct LadLaunch { int seq; uint64_t step_before; int nsteps; int log_head_before; };
  std::vector<LadLaunch> lad_log;   // launches not yet looked at
  // Steps asked for in small portions (a host loop that calls ptm_step(1): the reference sampler's, ptmcmc.cc:563-599) are only COUNTED
  // here and launched together at the engine's next look at the device -- any getter, setter or ptm_sync -- or when enough have
  // gathered: nothing can observe the difference, and a launch of the persistent kernel costs ~15 us on top of its 5 us steps.
  int lad_deferred = 0;
  int lad_seq = 0;                  // number of the last launch issued
  bool lad_disabled = false;        // a launch gave up once: this engine keeps the two-launch path from then on
  long long ladder_fallbacks = 0;   // launches that gave up (their steps were repeated on the two-launch path)
  hipEvent_t lad_event = nullptr;   // end of this engine's last launch of that kernel (two engines' grids must not share the device)
  unsigned int nhist_pending = 0;   // steps whose one-add-per-chain the compacted sweep left uncounted (flush_nhist)
  // the horizon (ptm_count_limit.hpp): an upper bound of every chain's Ntries and Nhist, raised by each admitted call (count_guard)
  CountHorizon horizon;
  bool step_booked = false;         // the PT step in progress (a step made in pieces) has been admitted: its later pieces are not asked again
  int steps_prepaid = 0;            // steps ptm_shard_step has been admitted for, whose pieces go through the public calls
  double* hastings = nullptr;
  int* htype = nullptr;
  unsigned char *hvalid = nullptr, *acc_out = nullptr;
  pinned_vector<double> h_rows, h_hast;
  pinned_vector<int> h_type;
  pinned_vector<unsigned char> h_valid, h_touch, h_acc;
  std::vector<double> p_xcur, p_xprop, p_hast;
  std::vector<int32_t> p_rung, p_walker, p_type, p_valid, p_acc;
  std::vector<size_t> p_pick;
  double *xprop = nullptr, *lprior_new = nullptr, *llike_new = nullptr;  // device buffers of the callback path
  // reads of device arrays by the ptm_get_* calls: asynchronous copies into one pinned arena, finished by ONE wait (a
  // synchronous hipMemcpy into pageable memory costs ~20 us whatever its size); between ptm_batch_begin and ptm_batch_end the
  // calls only queue, and their output buffers are filled by ptm_batch_end
  pinned_vector<unsigned char> fetch_arena;
  size_t fetch_used = 0;
  int fetch_depth = 0;
  std::vector<std::function<void()>> fetch_after;
  std::vector<std::shared_ptr<std::vector<unsigned char>>> fetch_big;
  std::vector<std::pair<unsigned char*, size_t>> host_blocks;   // arrays kept in mapped host memory (a small history ring): read in place
  bool shared_handover = false, hist_on_host = false;   // ... or, for a small population, the pinned host images themselves (mapped into the device)
  unsigned char* gate = nullptr;
  pinned_vector<double> h_xprop, h_llnew;
  std::vector<double> h_batch, h_llbatch;
  unsigned char* h_gate = nullptr;   // view into h_xprop's tail
  unsigned long long *sums = nullptr, *h_sums = nullptr;   // ptm_get_counter_sums
  // effective sample size (ptm_ess_*): the workspace (lag list, answers, one chunk's table), allocated at the first call and grown on demand
  void* ess_ws = nullptr;
  size_t ess_ws_bytes = 0;
  int ess_on_device = 0;   // the last ptm_ess_* call of this engine ran the kernels
  // ptm_adapt_proposals: the eigen kernel's workspace (factors, eigenvalues, status, the rotations of dimensions above 64), grown on demand
  void* eig_ws = nullptr;
  size_t eig_ws_bytes = 0;
  // timing
  hipEvent_t t0 = nullptr, t1 = nullptr;
  std::vector<hipEvent_t> kev;  // pairs
  size_t kev_used = 0;
  std::string kname;
};

// Persistent ladder kernels of different engines (streams) must not run at the same time: each sizes its grid for a device of its
// own, two at once may not be resident together and would wait for each other's workgroups until they give up.  A launch
// therefore waits for the event of the last such launch of any OTHER engine of the process.
#include <mutex>
static std::mutex g_lad_mutex;
static ptm_engine* g_lad_last = nullptr;

static int round_dp(int D) {
  if (D <= 4) return 4;
  if (D <= 8) return 8;
  if (D <= 16) return 16;
  if (D <= 32) return 32;
  if (D <= 64) return 64;
  if (D <= 128) return 128;
  if (D <= 256) return 256;
  if (D <= 512) return 512;
  return 1024;
}

template <class T>
static int dalloc(T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, (n ? n : 1) * sizeof(T)));
  return PTM_OK;
}
// a copy between a device buffer and its host image; nothing to do when the two are one (small populations keep the
// hand-over buffers of the host paths in mapped host memory, alloc_proposal_buffers)
static hipError_t copy_unless_shared(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  if (dst == src) return hipSuccess;
  return hipMemcpyAsync(dst, src, bytes, kind, s);
}
struct ptm_engine;
static int fetch_flush(ptm_engine* e);
static int fetch(ptm_engine* e, const void* dev, size_t bytes, const unsigned char** staged);
static int fetch_done(ptm_engine* e);
// small write-only outputs of the kernels that the host reads after every step (the history ring of a small population):
// mapped, coherent host memory -- the kernels' writes go over the bus as they happen, the host reads them with no copy
static bool small_outputs_on_host(size_t bytes) {
  const char* z = getenv("PTM_SHARED_HANDOVER");
  return bytes <= ((size_t)1 << 20) && !(z && *z == '0');
}
template <class T>
static int halloc(ptm_engine* e, T** p, size_t n);
template <class T>
static int upload(T* d, const T* h, size_t n, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyDefault, s));
  HIPCHK(hipStreamSynchronize(s));
  return PTM_OK;
}

// Row labels back to the identity and the rows back to their own rungs, in place (restore_rows_kernel; 1024 rungs x 16384 walkers
// of 32 dimensions: see DESIGN 3.2 for its cost).  Queued on the stream; a failed launch stays with the runtime for the next check.
static void flush_rows(ptm_engine* e);
// the rows [Nc][DP], every chain's at its own place: what every reader and writer outside a labelled step takes
static double* xrows(ptm_engine* e) {
  if (e->rows_labelled) flush_rows(e);
  return e->xdev;
}

// proposals the engine does not draw itself: the host's (ptm_set_proposal_callback) or the user's on the device (ptm_set_proposal_device).
// Either way the sweep kernel takes ready-made proposals (host_prop)
static inline bool user_prop(const ptm_engine* e) { return e->pcb != nullptr || e->dpfn != nullptr; }

extern "C" const char* ptm_last_error(void) { return g_err.c_str(); }
extern "C" int ptm_abi_version(void) { return PTM_ABI_VERSION; }

extern "C" int ptm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  int ok = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, i) == hipSuccess && strncmp(pr.gcnArchName, "gfx950", 6) == 0) ok++;
  }
  return ok;
}

static int need_device() {
  if (ptm_device_count() <= 0)
    return fail(PTM_ERR_NO_DEVICE, "no gfx950 (MI355X) device visible: the engine has no CPU fallback");
  return PTM_OK;
}

extern "C" int ptm_engine_destroy(ptm_engine* e);
extern "C" int ptm_shard_finalize(ptm_engine* e);
static int build_engine(ptm_engine* e, const ptm_config* cfg);
static int launch_beta_transpose(ptm_engine* e);
static int ensure_betaC(ptm_engine* e);
static int ladder_settle(ptm_engine* e);
static int fill_evolving_ladders(ptm_engine* e);

extern "C" int ptm_engine_create(const ptm_config* cfg, ptm_engine** out) {
  if (!cfg || !out) return fail(PTM_ERR_INVALID, "null argument");
  // ABI evolution: a caller built against an older header hands a shorter struct; the fields it does not know are zero
  ptm_config cfg_full;
  memset(&cfg_full, 0, sizeof cfg_full);
  if (cfg->struct_size > sizeof(ptm_config) || cfg->struct_size < offsetof(ptm_config, walker_begin)) return fail(PTM_ERR_INVALID, "ptm_config size mismatch (ABI)");
  memcpy(&cfg_full, cfg, cfg->struct_size);
  cfg_full.struct_size = sizeof(ptm_config);
  cfg = &cfg_full;
  if (cfg->walker_begin < 0) return fail(PTM_ERR_INVALID, "walker_begin must be >= 0");
  if (cfg->dim < 1) return fail(PTM_ERR_INVALID, "dim must be >= 1");
  if (cfg->dim > 1024) return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built (kernels exist for padded dimensions 4, 8, 16, ..., 1024)");
  if (cfg->n_rungs < 1 || cfg->n_rungs > 65535) return fail(PTM_ERR_INVALID, "n_rungs must be in 1..65535");
  if (cfg->rung_begin < 0 || cfg->rung_count < 1 || cfg->rung_begin + cfg->rung_count > cfg->n_rungs)
    return fail(PTM_ERR_INVALID, "rung block out of range");
  if (cfg->n_walkers < 1) return fail(PTM_ERR_INVALID, "n_walkers must be >= 1");
  if (cfg->add_every_n < 1) return fail(PTM_ERR_INVALID, "add_every_n must be >= 1");
  if ((double)cfg->rung_count * cfg->n_walkers > 2.0e9) return fail(PTM_ERR_INVALID, "too many chains for one engine");
  // a chain's random stream id is (global walker) * n_rungs + (global rung), 32 bits
  if (((double)cfg->walker_begin + cfg->n_walkers) * cfg->n_rungs > 4294967296.0) return fail(PTM_ERR_INVALID, "too many chains for 32-bit stream ids: (walker_begin + n_walkers) * n_rungs must stay below 2^32");
  int rc = need_device();
  if (rc) return rc;
  ptm_engine* e = new ptm_engine();
  rc = build_engine(e, cfg);
  if (rc) { (void)ptm_engine_destroy(e); return rc; }   // nothing of a half-built engine survives
  *out = e;
  return PTM_OK;
}

static int build_engine(ptm_engine* e, const ptm_config* cfg) {
  int rc;
  e->cfg = *cfg;
  e->D = cfg->dim; e->DP = round_dp(cfg->dim); e->Nt = cfg->n_rungs; e->r0 = cfg->rung_begin; e->nloc = cfg->rung_count;
  e->W = cfg->n_walkers; e->Nc = e->nloc * e->W;
  e->ms = (int)(1 + 2 * cfg->swap_rate * cfg->n_rungs);                      // chain.cc:1192
  {
    // Rows that cross one shard boundary in one direction per step: at most one per walker, and a walker's boundary pair
    // is a candidate with probability <= swap_rate (maxswapsperstep * thresh / (Ntemps-1), chain.cc:1413-1416).
    // Default capacity: that binomial's mean + 8 sigma + 64, or every walker if that is less.
    const double pr = cfg->swap_rate < 1 ? (cfg->swap_rate > 0 ? cfg->swap_rate : 0) : 1;
    const double want = e->W * pr + 8 * std::sqrt(e->W * pr) + 64;
    e->row_cap = cfg->exchange_row_capacity > 0 ? cfg->exchange_row_capacity : (want < e->W ? (int)want : e->W);
    if (e->row_cap > e->W) e->row_cap = e->W;
  }
  e->thresh = (e->Nt - 1) * cfg->swap_rate / e->ms;                          // chain.cc:1413
  if (cfg->history_rungs < 0 || cfg->history_rungs > cfg->rung_count) { return fail(PTM_ERR_INVALID, "history_rungs out of range"); }
  if (cfg->history_rungs > 0) {
    if (cfg->history_capacity < 2) { return fail(PTM_ERR_INVALID, "history_capacity must be >= 2"); }
    // a rung touched twice in a step saves the row it held in between, which may be the row of the rung above: on a
    // shard that is not the ladder's last, the shard's top rung therefore cannot be recorded
    if (cfg->history_rungs == cfg->rung_count && cfg->rung_begin + cfg->rung_count < cfg->n_rungs) {
      return fail(PTM_ERR_UNSUPPORTED, "the top rung of a shard below the ladder's top cannot be recorded: history_rungs < rung_count");
    }
    if ((double)cfg->history_rungs * cfg->n_walkers >= (double)(1 << 30)) { return fail(PTM_ERR_INVALID, "too many recorded chains"); }
    e->hist.rungs = cfg->history_rungs; e->hist.cap = cfg->history_capacity; e->hist.HC = cfg->history_rungs * cfg->n_walkers;
  }
  if (cfg->device >= 0) { HIPCHK(hipSetDevice(cfg->device)); e->device = cfg->device; } else HIPCHK(hipGetDevice(&e->device));
  if (cfg->stream) e->stream = (hipStream_t)cfg->stream;
  else { HIPCHK(hipStreamCreate(&e->stream)); e->own_stream = true; }
  const size_t Nc = e->Nc, D = e->DP;  // every per-dimension table is padded to DP
  if ((rc = dalloc(&e->xdev, Nc * D)) || (rc = dalloc(&e->ll, Nc)) || (rc = dalloc(&e->lp, Nc))) return rc;
  HIPCHK(hipMemsetAsync(e->xdev, 0, Nc * D * 8, e->stream));
  if ((rc = dalloc(&e->ntries, Nc)) || (rc = dalloc(&e->naccept, Nc)) || (rc = dalloc(&e->last_type, Nc)) ||
      (rc = dalloc(&e->arr_below, (size_t)cfg->n_walkers)) || (rc = dalloc(&e->mv_src, (size_t)cfg->n_walkers * MVCAP)) ||
      (rc = dalloc(&e->mv_dst, (size_t)cfg->n_walkers * MVCAP)) || (rc = dalloc(&e->mv_n, (size_t)cfg->n_walkers)) ||
      (rc = dalloc(&e->arr_above, (size_t)cfg->n_walkers)) || (rc = dalloc(&e->touch, Nc)) || (rc = dalloc(&e->nhist, Nc)) ||
      (rc = dalloc(&e->err, 4)))
    return rc;
  if (cfg->map_rungs < 0 || cfg->map_rungs > cfg->rung_count) return fail(PTM_ERR_INVALID, "map_rungs out of range");
  if (cfg->map_rungs > 0) {
    if (cfg->map_rungs == cfg->rung_count && cfg->rung_begin + cfg->rung_count < cfg->n_rungs)
      return fail(PTM_ERR_UNSUPPORTED, "the top rung of a shard below the ladder's top cannot be tracked: map_rungs < rung_count");
    if ((double)cfg->map_rungs * cfg->n_walkers >= (double)(1 << 29)) return fail(PTM_ERR_INVALID, "too many MAP-tracked chains");
    e->map.rungs = cfg->map_rungs; e->map.MC = cfg->map_rungs * cfg->n_walkers;
    const size_t n = (size_t)e->map.MC;
    if ((rc = dalloc(&e->map.lpost, n)) || (rc = dalloc(&e->map.ll, n)) || (rc = dalloc(&e->map.lp, n)) || (rc = dalloc(&e->map.x, n * D)))
      return rc;
  }
  if (e->hist.rungs) {
    const size_t n = (size_t)e->hist.cap * e->hist.HC;
    e->hist_on_host = small_outputs_on_host(n * D * 8);
    if (e->hist_on_host) {
      if ((rc = halloc(e, &e->hist.x, n * D)) || (rc = halloc(e, &e->hist.ll, n)) || (rc = halloc(e, &e->hist.lp, n)) || (rc = halloc(e, &e->hist.meta, n)))
        return rc;
    } else if ((rc = dalloc(&e->hist.x, n * D)) || (rc = dalloc(&e->hist.ll, n)) || (rc = dalloc(&e->hist.lp, n)) || (rc = dalloc(&e->hist.meta, n)))
      return rc;
    HIPCHK(hipMemsetAsync(e->hist.meta, 0xFF, n * sizeof(int4), e->stream));   // saved row number -1: empty slot
  }
  const size_t np = (size_t)e->W * (e->Nt > 1 ? e->Nt - 1 : 1);
  if ((rc = dalloc(&e->swap_cnt, 2 * np)) || (rc = dalloc(&e->swap_log, (size_t)PTM_LOG_RING * e->W * e->ms)))
    return rc;
  HIPCHK(hipMemsetAsync(e->swap_cnt, 0, 2 * np * 8, e->stream));
  HIPCHK(hipMemsetAsync(e->swap_log, 0xFE, (size_t)PTM_LOG_RING * e->W * e->ms * 4, e->stream));  // 0xFEFEFEFE < 0: "none"
  HIPCHK(hipMemsetAsync(e->err, 0, 16, e->stream));
  HIPCHK(hipMemsetAsync(e->mv_n, 0, (size_t)e->W * 4, e->stream));
  if ((rc = dalloc(&e->blo, D)) || (rc = dalloc(&e->bhi, D)) || (rc = dalloc(&e->ptype, D)) || (rc = dalloc(&e->bmin, D)) ||
      (rc = dalloc(&e->bmax, D)) || (rc = dalloc(&e->plo, D)) || (rc = dalloc(&e->phi, D)) || (rc = dalloc(&e->pcoef, D)) ||
      (rc = dalloc(&e->P2, D * (D + 1) / 2)) || (rc = dalloc(&e->mean, D)) || (rc = dalloc(&e->beta, (size_t)e->Nt)) ||
      (rc = dalloc(&e->onedfrac, (size_t)e->nloc)) || (rc = dalloc(&e->P2_tiles, 144 * 64)) || (rc = dalloc(&e->box_row, 256)))
    return rc;
  {
    const int bd = e->DP == 128 ? 128 : (e->DP == 64 ? 64 : 32);
    std::vector<double> box(256);
    for (int d = 0; d < bd; ++d) { box[d] = -INFINITY; box[bd + d] = INFINITY; }
    if ((rc = upload(e->box_row, box.data(), 256, e->stream))) return rc;
    HIPCHK(hipMemsetAsync(e->P2_tiles, 0, (144 * 64) * 8, e->stream));
  }
  // defaults (and the permanent content of the pad dimensions): open bounds, flat prior with unbounded support
  std::vector<int> zi(D, 0);
  std::vector<double> zd(D, 0.0), one(D, 1.0), ninf(D, -INFINITY), pinf(D, INFINITY);
  if ((rc = upload(e->blo, zi.data(), D, e->stream)) || (rc = upload(e->bhi, zi.data(), D, e->stream)) ||
      (rc = upload(e->ptype, zi.data(), D, e->stream)) || (rc = upload(e->bmin, zd.data(), D, e->stream)) ||
      (rc = upload(e->bmax, zd.data(), D, e->stream)) || (rc = upload(e->plo, ninf.data(), D, e->stream)) ||
      (rc = upload(e->phi, pinf.data(), D, e->stream)) || (rc = upload(e->pcoef, one.data(), D, e->stream)) ||
      (rc = upload(e->mean, zd.data(), D, e->stream)))
    return rc;
  e->h_ptype.assign(D, 0); e->h_plo.assign(D, -INFINITY); e->h_phi.assign(D, INFINITY);
  e->all_uniform = 0;  // flat prior goes through the general product (pdf == 1)
  HIPCHK(hipEventCreate(&e->t0));
  HIPCHK(hipEventCreate(&e->t1));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

template <class T>
static int halloc(ptm_engine* e, T** p, size_t n) {
  void* h = nullptr;
  const size_t bytes = (n ? n : 1) * sizeof(T);
  HIPCHK(hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent));
  e->host_blocks.push_back(std::make_pair((unsigned char*)h, bytes));
  *p = (T*)h;
  return PTM_OK;
}

// ---- batched reads (see ptm_engine::fetch_arena) ------------------------------------------------------------------------
static const size_t FETCH_ARENA = (size_t)4 << 20;
static int fetch_flush(ptm_engine* e) {
  HIPCHK(hipStreamSynchronize(e->stream));
  for (auto& f : e->fetch_after) f();
  e->fetch_after.clear(); e->fetch_big.clear(); e->fetch_used = 0;
  return PTM_OK;
}
// queues the copy of `bytes` at device address `dev` (ordered on the engine's stream, so it sees the state at the time of the
// call); *staged is where the bytes will be once fetch_flush has waited -- valid until that flush returns
static int fetch_raw(ptm_engine* e, const void* dev, size_t bytes, const unsigned char** staged) {
  for (const auto& b : e->host_blocks)
    if ((const unsigned char*)dev >= b.first && (const unsigned char*)dev < b.first + b.second) {   // already on the host: the flush's wait is all it needs
      *staged = (const unsigned char*)dev;
      return PTM_OK;
    }
  if (e->fetch_arena.empty()) e->fetch_arena.resize(FETCH_ARENA);
  const size_t need = (bytes + 63) & ~(size_t)63;
  // A big array, or one the arena has no room left for: its own buffer, copied at once (for a big array bandwidth, not call
  // latency, is the cost).  The arena is never recycled before the flush: pointers staged earlier in the same call or the same
  // ptm_batch_begin / ptm_batch_end bracket stay valid until their lambdas have run.
  if (need > FETCH_ARENA / 2 || e->fetch_used + need > FETCH_ARENA) {
    auto buf = std::make_shared<std::vector<unsigned char>>(bytes);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(buf->data(), dev, bytes, hipMemcpyDeviceToHost));
    e->fetch_big.push_back(buf);
    *staged = buf->data();
    return PTM_OK;
  }
  unsigned char* at = e->fetch_arena.data() + e->fetch_used;
  HIPCHK(hipMemcpyAsync(at, dev, bytes, hipMemcpyDeviceToHost, e->stream));
  e->fetch_used += need;
  *staged = at;
  return PTM_OK;
}
// a read that fails cancels everything queued (the outputs of this call and of an open bracket are then never written: no
// lambda is left pointing at a caller's buffer)
static int fetch(ptm_engine* e, const void* dev, size_t bytes, const unsigned char** staged) {
  const int rc = fetch_raw(e, dev, bytes, staged);
  if (rc) { e->fetch_after.clear(); e->fetch_big.clear(); e->fetch_used = 0; }
  return rc;
}
static int fetch_done(ptm_engine* e) { return e->fetch_depth > 0 ? PTM_OK : fetch_flush(e); }
// Between ptm_batch_begin and ptm_batch_end only reads are allowed: a queued read of mapped host memory (a small population's
// history ring) is served in place at the flush, so nothing may change the engine's arrays in between.
// the launches of the persistent ladder kernel since the last look: committed, or repeated on the two-launch path (ladder_settle)
#define SETTLE(e) do { if (e) { const int _rc = ladder_settle(e); if (_rc) return _rc; } } while (0)
#define NO_BATCH(e, name) do { if ((e) && (e)->fetch_depth > 0) return fail(PTM_ERR_INVALID, name " between ptm_batch_begin and ptm_batch_end (only reads go there)"); } while (0)
#define FETCH(ptr, dev, bytes) do { int _rc = fetch(e, (dev), (bytes), &(ptr)); if (_rc) return _rc; } while (0)

extern "C" int ptm_batch_begin(ptm_engine* e) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  e->fetch_depth++;
  return PTM_OK;
}
extern "C" int ptm_batch_end(ptm_engine* e) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (e->fetch_depth <= 0) return fail(PTM_ERR_INVALID, "ptm_batch_end without ptm_batch_begin");
  if (--e->fetch_depth > 0) return PTM_OK;
  return fetch_flush(e);
}

extern "C" int ptm_engine_destroy(ptm_engine* e) {
  if (!e) return PTM_OK;
  (void)ptm_shard_finalize(e);
  (void)hipStreamSynchronize(e->stream);
  {
    std::lock_guard<std::mutex> lock(g_lad_mutex);
    if (g_lad_last == e) g_lad_last = nullptr;
  }
  if (e->lad_event) (void)hipEventDestroy(e->lad_event);
  if (e->shared_handover) e->xprop = e->llike_new = nullptr, e->hastings = nullptr, e->htype = nullptr, e->hvalid = e->acc_out = nullptr;   // (these are the pinned vectors)
  if (e->hist_on_host) e->hist.x = e->hist.ll = e->hist.lp = e->hist.beta = nullptr, e->hist.meta = nullptr;
  for (auto& b : e->host_blocks) (void)hipHostFree(b.first);
  void* ptrs[] = {e->xdev, e->rowof, e->ll, e->lp, e->ntries, e->naccept, e->last_type, e->arr_below, e->arr_above, e->mv_src, e->mv_dst, e->mv_n,
                  e->err, e->nhist, e->swap_cnt, e->touch, e->swap_log, e->hist.x, e->hist.ll, e->hist.lp, e->hist.meta, e->map.lpost, e->map.ll, e->map.lp, e->map.x, e->blo,
                  e->bhi, e->ptype, e->bmin, e->bmax, e->plo, e->phi, e->pcoef, e->P2, e->mean, e->beta, e->prop, e->prop_tiles, e->P2_tiles, e->box_row, e->onedfrac, e->mix, e->beta_w, e->betaC, e->beta_add, e->hist.beta, e->xprop, e->lprior_new, e->llike_new, e->hastings, e->htype, e->hvalid, e->acc_out, e->cidx, e->ccnt, e->pidx, e->pcnt, e->pf_flag, e->pf_counts, e->pf_margin,
                  e->pub_x, e->lad_flags, e->lad_prof, e->shard_ends, e->redo_flag, e->sums, e->de_init, e->de_hast, e->de_type,
                  e->ada_leaf, e->ada_dbl, e->ada_int, e->dl_own_x ? e->dl_x : nullptr, e->dl_own_ll ? e->dl_ll : nullptr, e->dl_count, e->dl_rows, e->dl_chunks, e->dl_xprop,
                  e->dl_lprior_new, e->dl_llike_new, e->dl_best, e->ess_ws, e->eig_ws,
                  e->dp_xcur, e->dp_xnew, e->dp_hast_k, e->dp_rung, e->dp_walker, e->dp_type_k, e->dp_valid_k, e->dp_acc_k, e->dp_count, e->dp_rows, e->dp_chunks,
                  e->dp_xprop, e->dp_hastings, e->dp_htype, e->dp_hvalid, e->dp_acc_out, e->pr_x, e->pr_lp, e->pr_count, e->pr_rows, e->pr_chunks};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (e->h_sums) (void)hipHostFree(e->h_sums);
  if (e->h_pf_flag) (void)hipHostFree(e->h_pf_flag);
  if (e->h_pf_margin) (void)hipHostFree(e->h_pf_margin);
  for (hipEvent_t ev : e->kev) (void)hipEventDestroy(ev);
  if (e->t0) (void)hipEventDestroy(e->t0);
  if (e->t1) (void)hipEventDestroy(e->t1);
  if (e->own_stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return PTM_OK;
}

// ---- problem description ----------------------------------------------------------------------------------
extern "C" int ptm_set_bounds(ptm_engine* e, const int32_t* lo, const int32_t* hi, const double* xmin, const double* xmax) {
  SETTLE(e);
  if (!e || !lo || !hi || !xmin || !xmax) return fail(PTM_ERR_INVALID, "null argument");
  int rc;
  const int D = e->D;
  e->has_bounds = 0;
  e->bounds_box = 1;
  for (int d = 0; d < D; ++d) {
    if (lo[d] < 0 || lo[d] > 3 || hi[d] < 0 || hi[d] > 3) return fail(PTM_ERR_INVALID, "bad boundary type in dimension %d", d);
    if (lo[d] != PTM_BOUND_OPEN || hi[d] != PTM_BOUND_OPEN) e->has_bounds = 1;
    if ((lo[d] != PTM_BOUND_OPEN && lo[d] != PTM_BOUND_LIMIT) || (hi[d] != PTM_BOUND_OPEN && hi[d] != PTM_BOUND_LIMIT)) e->bounds_box = 0;
  }
  // Q9: state::add() builds on state(space,n) = enforced zero vector (states.cc:183-192,205-214).  Plain host
  // arithmetic on D constants; zero is only ever *rejected* by a `limit` bound, any other bound type maps it.
  e->origin_valid = 1;
  for (int d = 0; d < D; ++d) {
    const bool lw = lo[d] == PTM_BOUND_WRAP, hw = hi[d] == PTM_BOUND_WRAP;
    if (lw != hw) { e->origin_valid = 0; break; }
    if (lw) { if (xmax[d] - xmin[d] <= 0) { e->origin_valid = 0; break; } continue; }
    if (lo[d] == PTM_BOUND_REFLECT && hi[d] == PTM_BOUND_REFLECT) { if (xmax[d] - xmin[d] <= 0) { e->origin_valid = 0; break; } continue; }
    double z = 0.0;
    if (lo[d] == PTM_BOUND_REFLECT && z < xmin[d]) z = xmin[d] + (xmin[d] - z);
    else if (hi[d] == PTM_BOUND_REFLECT && z > xmax[d]) z = xmax[d] - (z - xmax[d]);
    if (lo[d] == PTM_BOUND_LIMIT && z < xmin[d]) { e->origin_valid = 0; break; }
    if (hi[d] == PTM_BOUND_LIMIT && z > xmax[d]) { e->origin_valid = 0; break; }
  }
  if ((rc = upload(e->blo, lo, D, e->stream)) || (rc = upload(e->bhi, hi, D, e->stream)) ||      // pad dimensions stay open
      (rc = upload(e->bmin, xmin, D, e->stream)) || (rc = upload(e->bmax, xmax, D, e->stream)))
    return rc;
  return PTM_OK;
}

static inline size_t host_row_pos(size_t DP, size_t d);
extern "C" int ptm_set_prior(ptm_engine* e, const int32_t* types, const double* c, const double* h) {
  SETTLE(e);
  if (!e || !types || !c || !h) return fail(PTM_ERR_INVALID, "null argument");
  const int D = e->D;
  std::vector<double> lo(D), hi(D), coef(D);
  std::vector<int> ty(D);
  e->all_uniform = 1;
  double prod = 1;
  for (int d = 0; d < D; ++d) {
    ty[d] = types[d];
    switch (types[d]) {  // mixed_dist_product ctor (probability_function.cc:232-254) and the 1-D ctors it calls
      case PTM_PRIOR_FLAT: lo[d] = -INFINITY; hi[d] = INFINITY; coef[d] = 1; e->all_uniform = 0; break;
      case PTM_PRIOR_UNIFORM: lo[d] = c[d] - h[d]; hi[d] = c[d] + h[d]; coef[d] = 1 / (hi[d] - lo[d]); prod *= coef[d]; break;
      case PTM_PRIOR_GAUSSIAN: lo[d] = c[d]; hi[d] = h[d]; coef[d] = 0; e->all_uniform = 0; break;
      case PTM_PRIOR_POLAR: {  // UniformPolarDist ctor: clamps only the normalisation (ProbabilityDist.h:181-186)
        double a = c[d] - h[d], b = c[d] + h[d];
        lo[d] = a; hi[d] = b;
        if (a < 0) a = 0;
        if (b > M_PI) b = M_PI;
        coef[d] = -std::cos(b) + std::cos(a);
        e->all_uniform = 0;
        break;
      }
      case PTM_PRIOR_COPOLAR: {  // ProbabilityDist.h:227-232
        double a = c[d] - h[d], b = c[d] + h[d];
        lo[d] = a; hi[d] = b;
        if (a < -M_PI / 2) a = -M_PI / 2;
        if (b > M_PI / 2) b = M_PI / 2;
        coef[d] = std::sin(b) - std::sin(a);
        e->all_uniform = 0;
        break;
      }
      case PTM_PRIOR_LOG:  // probability_function.cc:245-250, ProbabilityDist.h:109-117
        if (c[d] <= 0 || h[d] <= 1) return fail(PTM_ERR_INVALID, "log prior needs center>0 and halfwidth>1 (dimension %d)", d);
        lo[d] = c[d] / h[d]; hi[d] = c[d] * h[d]; coef[d] = std::log(hi[d]) - std::log(lo[d]);
        e->all_uniform = 0;
        break;
      default: return fail(PTM_ERR_INVALID, "unknown prior type %d in dimension %d", types[d], d);
    }
  }
  e->lprior_const = std::log(prod);  // the reference takes libm log of the product of these constants on every call
  e->pf_dirty = true;
  e->lp_is_const = false;            // (re-established when states are set)
  for (int d = 0; d < D; ++d) { e->h_ptype[d] = ty[d]; e->h_plo[d] = lo[d]; e->h_phi[d] = hi[d]; }
  int rc;
  if ((rc = upload(e->ptype, ty.data(), D, e->stream)) || (rc = upload(e->plo, lo.data(), D, e->stream)) ||
      (rc = upload(e->phi, hi.data(), D, e->stream)) || (rc = upload(e->pcoef, coef.data(), D, e->stream)))
    return rc;
  if (e->DP == 32 || e->DP == 64 || e->DP == 128) {   // the box in row layout, for the MFMA kernels (pad dimensions stay unbounded)
    const int bd = e->DP;
    std::vector<double> box(2 * bd);
    for (int d = 0; d < bd; ++d) {
      box[host_row_pos(bd, d)] = d < D ? lo[d] : -INFINITY;
      box[bd + host_row_pos(bd, d)] = d < D ? hi[d] : INFINITY;
    }
    if ((rc = upload(e->box_row, box.data(), 2 * bd, e->stream))) return rc;
  }
  return PTM_OK;
}

extern "C" int ptm_set_target_gaussian(ptm_engine* e, const double* mean, const double* P, double like0) {
  SETTLE(e);
  if (!e || !P) return fail(PTM_ERR_INVALID, "null argument");
  const int D = e->D, DP = e->DP;
  std::vector<double> packed((size_t)DP * (DP + 1) / 2, 0.0);
  for (int i = 0; i < D; ++i) {
    const size_t o = (size_t)i * (i + 1) / 2;
    for (int j = 0; j < i; ++j) packed[o + j] = P[i * D + j] + P[j * D + i];
    packed[o + i] = P[i * D + i];
  }
  int rc;
  if ((rc = upload(e->P2, packed.data(), packed.size(), e->stream))) return rc;
  if (DP == 32) {
    // A-operand tiles of the MFMA kernel: tile t = step*2 + rowtile, lane 16k + i holds P2[16 rowtile + i][4 step + k]
    std::vector<double> tiles(16 * 64, 0.0);
    for (int t = 0; t < 16; ++t) {
      const int rt = t & 1, m = t >> 1;
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 16; ++i) {
          const int row = 16 * rt + i, col = 4 * m + k;
          if (row < D && col <= row) tiles[(size_t)t * 64 + 16 * k + i] = packed[(size_t)row * (row + 1) / 2 + col];
        }
    }
    if ((rc = upload(e->P2_tiles, tiles.data(), tiles.size(), e->stream))) return rc;
  }
  if (DP == 64 || DP == 128) {
    // A-operand tiles of ptm_mfma64_kernel.hpp / ptm_mfma128_kernel.hpp: (row tile rt, step m) with m <= 4 rt + 3 at base(rt) + m,
    // base(rt) = 2 rt (rt + 1) = 0, 4, 12, 24, ..; lane 16k + i holds P2[16 rt + i][4 m + k] (lower triangle, off-diagonals doubled;
    // zeros above the diagonal)
    const int NT = DP / 16;
    std::vector<double> tiles((size_t)2 * NT * (NT + 1) * 64, 0.0);
    for (int rt = 0; rt < NT; ++rt)
      for (int m = 0; m <= 4 * rt + 3; ++m)
        for (int k = 0; k < 4; ++k)
          for (int i = 0; i < 16; ++i) {
            const int row = 16 * rt + i, col = 4 * m + k;
            if (row < D && col <= row) tiles[(size_t)(2 * rt * (rt + 1) + m) * 64 + 16 * k + i] = packed[(size_t)row * (row + 1) / 2 + col];
          }
    if ((rc = upload(e->P2_tiles, tiles.data(), tiles.size(), e->stream))) return rc;
  }
  e->has_mean = mean ? 1 : 0;
  if (mean && (rc = upload(e->mean, mean, D, e->stream))) return rc;
  e->like0 = like0;
  e->have_target = 1;
  e->cb = nullptr;  // a device target replaces a host callback
  e->dfn = nullptr;  // ... and a device likelihood
  return PTM_OK;
}

// the proposal hand-over buffers both host paths use (callback likelihood: propose pass -> host; host-side proposals: host ->
// kernel): proposed states in row layout, the gate bytes right behind them (one device-to-host copy fetches both)
static int alloc_proposal_buffers(ptm_engine* e) {
  const size_t Nc = e->Nc, DP = e->DP;
  int rc;
  // A small population's step on the host paths is a chain of copies and waits, each ~5-10 us of runtime calls for a few
  // kilobytes: there the kernels read and write the pinned host images directly (coherent mapped memory; a kernel's writes are
  // on the host when its stream has drained, the host's are there for the next launch) and the copies fall away.
  const char* zc = getenv("PTM_SHARED_HANDOVER");
  if (!e->xprop) e->shared_handover = Nc * DP * 8 <= ((size_t)1 << 20) && !(zc && *zc == '0');
  e->h_xprop.resize(Nc * DP + (Nc + 7) / 8); e->h_llnew.assign(Nc, 0.0);
  e->h_gate = reinterpret_cast<unsigned char*>(e->h_xprop.data() + Nc * DP);
  if (e->shared_handover) {
    HIPCHK(hipHostGetDevicePointer((void**)&e->xprop, e->h_xprop.data(), 0));
    HIPCHK(hipHostGetDevicePointer((void**)&e->llike_new, e->h_llnew.data(), 0));
    if (!e->lprior_new && (rc = dalloc(&e->lprior_new, Nc))) return rc;
  } else if (!e->xprop && ((rc = dalloc(&e->xprop, Nc * DP + (Nc + 7) / 8)) || (rc = dalloc(&e->lprior_new, Nc)) || (rc = dalloc(&e->llike_new, Nc))))
    return rc;
  e->gate = reinterpret_cast<unsigned char*>(e->xprop + Nc * DP);
  return PTM_OK;
}

extern "C" int ptm_set_target_callback(ptm_engine* e, ptm_loglike_batch_fn fn, void* user) {
  SETTLE(e);
  if (!e || !fn) return fail(PTM_ERR_INVALID, "null argument");
  int rc = alloc_proposal_buffers(e);
  if (rc) return rc;
  e->cb = fn; e->cb_user = user;
  e->dfn = nullptr;   // (the last target setter wins)
  e->have_target = 1;
  return PTM_OK;
}

extern "C" int ptm_set_prior_callback(ptm_engine* e, ptm_logprior_batch_fn fn, void* user) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (fn && e->dprior) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior beside a device prior is not built: remove that one first (ptm_set_prior_device)");
  if (fn && e->dfn) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior with a device likelihood is not built (ptm_set_target_device)");
  e->prior_cb = fn; e->prior_user = fn ? user : nullptr;
  e->lp_is_const = false;
  return PTM_OK;
}

extern "C" int ptm_set_proposal_callback(ptm_engine* e, ptm_propose_batch_fn propose, ptm_proposal_result_fn result, void* user) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!propose) {   // back to the device proposals, if any were set
    e->pcb = nullptr; e->pres = nullptr; e->pcb_user = nullptr;
    e->dpfn = nullptr; e->dpres = nullptr; e->dp_user = nullptr;   // (the last proposal setter wins)
    e->have_prop = e->prop ? 1 : 0;
    return PTM_OK;
  }
  if (e->dfn) return fail(PTM_ERR_UNSUPPORTED, "host-side proposals with a device likelihood are not built (ptm_set_target_device)");
  if (e->dprior) return fail(PTM_ERR_UNSUPPORTED, "host-side proposals with a device prior are not built (ptm_set_prior_device)");
  const size_t Nc = e->Nc, DP = e->DP;
  int rc = alloc_proposal_buffers(e);
  if (rc) return rc;
  e->h_rows.resize(Nc * DP); e->h_hast.assign(Nc, 0.0); e->h_type.assign(Nc, 0); e->h_valid.assign(Nc, 0); e->h_touch.assign(Nc, 0); e->h_acc.assign(Nc, 0);
  if (e->shared_handover) {
    HIPCHK(hipHostGetDevicePointer((void**)&e->hastings, e->h_hast.data(), 0));
    HIPCHK(hipHostGetDevicePointer((void**)&e->htype, e->h_type.data(), 0));
    HIPCHK(hipHostGetDevicePointer((void**)&e->hvalid, e->h_valid.data(), 0));
    HIPCHK(hipHostGetDevicePointer((void**)&e->acc_out, e->h_acc.data(), 0));
  } else if (!e->hastings && ((rc = dalloc(&e->hastings, Nc)) || (rc = dalloc(&e->htype, Nc)) || (rc = dalloc(&e->hvalid, Nc)) || (rc = dalloc(&e->acc_out, Nc))))
    return rc;
  if (!e->onedfrac) return fail(PTM_ERR_INVALID, "engine not built");
  e->pcb = propose; e->pres = result; e->pcb_user = user;
  e->dpfn = nullptr; e->dpres = nullptr; e->dp_user = nullptr;   // (the last proposal setter wins)
  e->have_prop = 1;
  return PTM_OK;
}

extern "C" int ptm_set_proposal_device(ptm_engine* e, ptm_propose_device_fn propose, ptm_proposal_result_device_fn result, void* user) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!propose && result) return fail(PTM_ERR_INVALID, "a result function without a propose function");
  SETTLE(e);
  NO_BATCH(e, "ptm_set_proposal_device");
  if (!propose) {   // back to the device's own proposals, if any were set
    e->dpfn = nullptr; e->dpres = nullptr; e->dp_user = nullptr;
    e->pcb = nullptr; e->pres = nullptr; e->pcb_user = nullptr;
    e->have_prop = e->prop ? 1 : 0;
    return PTM_OK;
  }
  if (!e->onedfrac) return fail(PTM_ERR_INVALID, "engine not built");
  const size_t Nc = e->Nc, D = e->D, DP = e->DP;
  int rc;
  if (!e->dp_count) {
    if ((rc = dalloc(&e->dp_xcur, Nc * D)) || (rc = dalloc(&e->dp_xnew, Nc * D)) || (rc = dalloc(&e->dp_hast_k, Nc)) || (rc = dalloc(&e->dp_rung, Nc)) ||
        (rc = dalloc(&e->dp_walker, Nc)) || (rc = dalloc(&e->dp_type_k, Nc)) || (rc = dalloc(&e->dp_valid_k, Nc)) || (rc = dalloc(&e->dp_acc_k, Nc)) ||
        (rc = dalloc(&e->dp_rows, Nc)) || (rc = dalloc(&e->dp_chunks, (Nc + DL_CHUNK - 1) / DL_CHUNK)) || (rc = dalloc(&e->dp_xprop, Nc * DP)) ||
        (rc = dalloc(&e->dp_hastings, Nc)) || (rc = dalloc(&e->dp_htype, Nc)) || (rc = dalloc(&e->dp_hvalid, Nc)) || (rc = dalloc(&e->dp_acc_out, Nc)) ||
        (rc = dalloc(&e->dp_count, 1)))
      return rc;
    // the rows of chains that make no move are read by the sweep kernel and never used: let them hold zeros, not what the allocator left
    HIPCHK(hipMemsetAsync(e->dp_xprop, 0, Nc * DP * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->dp_xnew, 0, Nc * D * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->dp_hastings, 0, Nc * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->dp_htype, 0, Nc * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->dp_hvalid, 0, Nc, e->stream));
    HIPCHK(hipMemsetAsync(e->dp_acc_out, 0, Nc, e->stream));
    HIPCHK(hipMemsetAsync(e->dp_acc_k, 0, Nc * 4, e->stream));
  }
  e->dpfn = propose; e->dpres = result; e->dp_user = user;
  e->pcb = nullptr; e->pres = nullptr; e->pcb_user = nullptr;   // (the last proposal setter wins)
  e->have_prop = 1;
  return PTM_OK;
}

// the user's batched log-likelihood on the chains picked by `pick` (row indices into the padded row image `rows`)
static int call_user(ptm_engine* e, const pinned_vector<double>& rows, const std::vector<size_t>& pick, std::vector<double>& out) {
  const size_t D = e->D, DP = e->DP, n = pick.size();
  out.assign(n, 0.0);
  if (!n) return PTM_OK;
  e->h_batch.resize(n * D);
  for (size_t k = 0; k < n; ++k)
    for (size_t d = 0; d < D; ++d) e->h_batch[k * D + d] = rows[pick[k] * DP + host_row_pos(DP, d)];
  e->cb(e->cb_user, e->h_batch.data(), (int)n, (int)D, out.data());
  return PTM_OK;
}

// the user's batched log-prior on the chains picked by `pick`
static int call_user_prior(ptm_engine* e, const pinned_vector<double>& rows, const std::vector<size_t>& pick, std::vector<double>& out) {
  const size_t D = e->D, DP = e->DP, n = pick.size();
  out.assign(n, 0.0);
  if (!n) return PTM_OK;
  e->h_batch.resize(n * D);
  for (size_t k = 0; k < n; ++k)
    for (size_t d = 0; d < D; ++d) e->h_batch[k * D + d] = rows[pick[k] * DP + host_row_pos(DP, d)];
  e->prior_cb(e->prior_user, e->h_batch.data(), (int)n, (int)D, out.data());
  return PTM_OK;
}
// host prior: the log-priors of the states now in e->xdev (their rows in e->h_xprop) replace what the device prior gave -- except
// where that is -inf by the state's invalidity (the device's flat stand-in prior has no other way to say -inf)
static int host_prior_of_states(ptm_engine* e) {
  const size_t Nc = e->Nc;
  std::vector<double> lp(Nc), out;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(lp.data(), e->lp, Nc * 8, hipMemcpyDeviceToHost));
  std::vector<size_t> pick;
  for (size_t c = 0; c < Nc; ++c)
    if (lp[c] > -__builtin_inf()) pick.push_back(c);
  int rc = call_user_prior(e, e->h_xprop, pick, out);
  if (rc) return rc;
  for (size_t k = 0; k < pick.size(); ++k) lp[pick[k]] = out[k];
  return upload(e->lp, lp.data(), Nc, e->stream);
}

extern "C" int ptm_set_ladder(ptm_engine* e, const double* beta) {
  SETTLE(e);
  NO_BATCH(e, "ptm_set_ladder");
  if (!e || !beta) return fail(PTM_ERR_INVALID, "null argument");
  e->h_beta.assign(beta, beta + e->Nt);
  int rc = upload(e->beta, beta, (size_t)e->Nt, e->stream);
  if (rc) return rc;
  e->have_ladder = 1;
  if (e->beta_w) return fill_evolving_ladders(e);   // evolving ladders restart from the new common ladder
  return PTM_OK;
}

// every ladder starts from the common ladder
static int fill_evolving_ladders(ptm_engine* e) {
  std::vector<double> bw((size_t)e->W * e->Nt);
  for (int w = 0; w < e->W; ++w) std::copy(e->h_beta.begin(), e->h_beta.end(), bw.begin() + (size_t)w * e->Nt);
  int rc = upload(e->beta_w, bw.data(), bw.size(), e->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));   // bw leaves scope
  return launch_beta_transpose(e);
}

extern "C" int ptm_set_evolve_temps(ptm_engine* e, double rate, double lpost_cut) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!(rate > 0)) {
    if (e->evolve_rate > 0) return fail(PTM_ERR_UNSUPPORTED, "an evolving ladder cannot be frozen again (the reference has no such call either)");
    return PTM_OK;   // evolve_temps is never called with rate <= 0 (ptmcmc.cc:512)
  }
  if (e->nloc != e->Nt) {
    // A rung shard: every accepted exchange renormalises ALL gaps and every later trial of the step sees it, so each shard replays
    // the whole ladder's trials -- from the whole ladder's llikes, which the caller gathers each step (ptm_exchange_decide_gathered;
    // the reference's MPI ranks do exactly that: gather_llikes, chain.cc:1433-1435,1950-1972).  Every shard keeps every ladder's
    // temperatures [W][Nt]; the gathered llikes (+ lpriors with a posterior-ordering cut) are [Nt][W] doubles per step.
    // (history / MAP tracking of the shard's own rungs: every shard replays every pick and so knows the temperature each of its
    //  rungs had at each add_state of the exchange phase -- beta_add, chain-indexed; the shard's top rung cannot be recorded unless
    //  it is the ladder's, as on a fixed ladder: ptm_engine_create)
    if ((double)e->W * e->Nt * 16.0 > 512.0 * 1024 * 1024)
      return fail(PTM_ERR_UNSUPPORTED, "evolving ladders on a rung shard gather %d x %d llikes (and lpriors) per step: more than 512 MB -- split such a population by walkers "
                                       "(ptm_config.walker_begin)", e->Nt, e->W);
  }
  if (!e->have_ladder) return fail(PTM_ERR_INVALID, "set the ladder first (ptm_set_ladder)");
  int rc;
  if (!e->beta_w) {
    if ((rc = dalloc(&e->beta_w, (size_t)e->W * e->Nt)) || (rc = dalloc(&e->betaC, (size_t)e->Nc))) return rc;
    if ((rc = fill_evolving_ladders(e))) return rc;
    // history / MAP tracking: an add_state of the exchange phase sees its rung's temperature between two pries of the step
    if ((e->hist.rungs || e->map.rungs) && (rc = dalloc(&e->beta_add, (size_t)e->Nc))) return rc;
    if (e->hist.rungs) {   // every saved row keeps the temperature it was saved at; the rows so far: the common ladder's
      const size_t n = (size_t)e->hist.cap * e->hist.HC;
      if ((rc = e->hist_on_host ? halloc(e, &e->hist.beta, n) : dalloc(&e->hist.beta, n))) return rc;
      hipLaunchKernelGGL(hist_beta_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->hist, e->beta, e->W, e->r0);
      HIPCHK(hipGetLastError());
    }
  }
  e->evolve_rate = rate;
  e->evolve_cut = lpost_cut >= 0 ? lpost_cut : -1;
  return PTM_OK;
}

extern "C" int ptm_get_invtemps(ptm_engine* e, double* beta) {
  SETTLE(e);
  if (!e || !beta) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->have_ladder) return fail(PTM_ERR_INVALID, "no ladder set");
  if (e->beta_w) {
    const size_t n = (size_t)e->W * e->Nt * 8;
    const unsigned char* s;
    FETCH(s, e->beta_w, n);
    e->fetch_after.push_back([=] { memcpy(beta, s, n); });
    return fetch_done(e);
  }
  for (int w = 0; w < e->W; ++w) std::copy(e->h_beta.begin(), e->h_beta.end(), beta + (size_t)w * e->Nt);
  return PTM_OK;
}

extern "C" int ptm_get_history_invtemps(ptm_engine* e, double* beta) {
  SETTLE(e);
  if (!e || !beta) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "this engine keeps no history (ptm_config.history_rungs)");
  if (!e->have_ladder) return fail(PTM_ERR_INVALID, "no ladder set");
  const size_t n = (size_t)e->hist.cap * e->hist.HC;
  if (e->hist.beta) {
    const unsigned char* s;
    FETCH(s, e->hist.beta, n * 8);
    e->fetch_after.push_back([=] { memcpy(beta, s, n * 8); });
    return fetch_done(e);
  }
  for (size_t i = 0; i < n; ++i) beta[i] = e->h_beta[e->r0 + (int)(i % e->hist.HC) / e->W];
  return PTM_OK;
}

extern "C" int ptm_set_invtemps(ptm_engine* e, const double* beta) {
  SETTLE(e);
  NO_BATCH(e, "ptm_set_invtemps");
  if (!e || !beta) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->beta_w) return fail(PTM_ERR_INVALID, "per-ladder temperatures exist only once the ladders evolve (ptm_set_evolve_temps)");
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(e->beta_w, beta, (size_t)e->W * e->Nt * 8, hipMemcpyHostToDevice));
  return launch_beta_transpose(e);
}

extern "C" int ptm_set_proposals(ptm_engine* e, int kind, const double* factors, const double* one_d_frac) {
  SETTLE(e);
  if (!e || !factors) return fail(PTM_ERR_INVALID, "null argument");
  const int D = e->D, DP = e->DP, nloc = e->nloc;
  int stride;
  std::vector<double> packed;
  if (kind == PTM_PROP_DIAG) {
    stride = DP;
    packed.assign((size_t)nloc * stride, 0.0);
    for (int r = 0; r < nloc; ++r)
      for (int d = 0; d < D; ++d) packed[(size_t)r * stride + d] = factors[(size_t)r * D + d];
  } else if (kind == PTM_PROP_DENSE || kind == PTM_PROP_LOWER) {
    stride = DP * DP;  // column-major, padded: element (i,j) at j*DP + i; a Cholesky factor keeps its zeros
    packed.assign((size_t)nloc * stride, 0.0);
    for (int r = 0; r < nloc; ++r)
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) packed[(size_t)r * stride + (size_t)j * DP + i] = factors[(size_t)r * D * D + (size_t)i * D + j];
    if (kind == PTM_PROP_LOWER)
      for (int r = 0; r < nloc; ++r)
        for (int i = 0; i < D; ++i)
          for (int j = i + 1; j < D; ++j)
            if (factors[(size_t)r * D * D + (size_t)i * D + j] != 0.0)
              return fail(PTM_ERR_INVALID, "PTM_PROP_LOWER factor of local rung %d has a non-zero above the diagonal", r);
  } else {
    return fail(PTM_ERR_INVALID, "unknown proposal kind %d", kind);
  }
  if (e->prop) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->prop)); e->prop = nullptr; }
  if (e->prop_tiles) { HIPCHK(hipFree(e->prop_tiles)); e->prop_tiles = nullptr; }
  int rc;
  if ((rc = dalloc(&e->prop, packed.size())) || (rc = upload(e->prop, packed.data(), packed.size(), e->stream))) return rc;
  if (DP == 32) {
    // A-operand tiles of the MFMA kernel: tile t = (half*4 + slot)*2 + rowtile, lane 16k + i holds
    // T[16 rowtile + i][16 half + 4k + slot].  A diagonal proposal (sigmas) goes through the same kernel as the diagonal
    // matrix it is: fma(sigma_i, z_i, +0) is the product sigma_i z_i, and the zero terms around it change nothing.
    std::vector<double> tiles((size_t)nloc * 16 * 64, 0.0);
    for (int r = 0; r < nloc; ++r)
      for (int t = 0; t < 16; ++t) {
        const int rt = t & 1, sl = (t >> 1) & 3, hb = t >> 3;
        for (int k = 0; k < 4; ++k)
          for (int i = 0; i < 16; ++i) {
            const int row = 16 * rt + i, col = 16 * hb + 4 * k + sl;
            if (row < D && col < D)
              tiles[((size_t)r * 16 + t) * 64 + 16 * k + i] =
                  kind == PTM_PROP_DIAG ? (row == col ? factors[(size_t)r * D + row] : 0.0) : factors[(size_t)r * D * D + (size_t)row * D + col];
          }
      }
    if ((rc = dalloc(&e->prop_tiles, tiles.size())) || (rc = upload(e->prop_tiles, tiles.data(), tiles.size(), e->stream))) return rc;
  }
  if (DP == 64 || DP == 128) {
    // A-operand tiles of ptm_mfma64_kernel.hpp / ptm_mfma128_kernel.hpp: tile t = (half*4 + slot)*NT + rowtile (NT = DP / 16 row
    // tiles), lane 16k + i holds T[16 rowtile + i][16 half + 4k + slot]
    const int NT = DP / 16, ntile = NT * NT * 4;
    std::vector<double> tiles((size_t)nloc * ntile * 64, 0.0);
    for (int r = 0; r < nloc; ++r)
      for (int t = 0; t < ntile; ++t) {
        const int rt = t % NT, sl = (t / NT) & 3, hb = t / (4 * NT);
        for (int k = 0; k < 4; ++k)
          for (int i = 0; i < 16; ++i) {
            const int row = 16 * rt + i, col = 16 * hb + 4 * k + sl;
            if (row < D && col < D)
              tiles[((size_t)r * ntile + t) * 64 + 16 * k + i] =
                  kind == PTM_PROP_DIAG ? (row == col ? factors[(size_t)r * D + row] : 0.0) : factors[(size_t)r * D * D + (size_t)row * D + col];
          }
      }
    if ((rc = dalloc(&e->prop_tiles, tiles.size())) || (rc = upload(e->prop_tiles, tiles.data(), tiles.size(), e->stream))) return rc;
  }
  std::vector<double> f(nloc, 0.0);
  e->any_oned = 0;
  if (one_d_frac)
    for (int r = 0; r < nloc; ++r) {
      if (one_d_frac[r] < 0 || one_d_frac[r] > 1) return fail(PTM_ERR_INVALID, "oneDfrac must be in [0,1]");  // hh:159-162
      f[r] = one_d_frac[r];
      if (f[r] > 0) e->any_oned = 1;
    }
  if ((rc = upload(e->onedfrac, f.data(), (size_t)nloc, e->stream))) return rc;
  e->prop_kind = kind; e->prop_stride = stride; e->have_prop = 1;
  e->pf_sigma.assign((size_t)nloc * PREFILTER_DIMS, 0.0);
  e->pf_margin_nat.assign((size_t)nloc * PREFILTER_DIMS, 0.0);
  for (int r = 0; r < nloc; ++r) {
    const double* fr = factors + (size_t)r * (kind == PTM_PROP_DIAG ? D : D * D);
    prefilter_sigmas(kind == PTM_PROP_DIAG, fr, D, &e->pf_sigma[(size_t)r * PREFILTER_DIMS]);
    prefilter_margins(kind == PTM_PROP_DIAG, fr, D, &e->pf_margin_nat[(size_t)r * PREFILTER_DIMS]);
  }
  e->pf_dirty = true;
  return PTM_OK;
}

// the adaptive proposal set's device arrays go (ptm_set_proposal_mixture replaces it)
static int ada_off(ptm_engine* e) {
  e->ada_on = false;
  if (!e->ada_leaf && !e->ada_dbl && !e->ada_int) return PTM_OK;
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->ada_leaf) HIPCHK(hipFree(e->ada_leaf));
  if (e->ada_dbl) HIPCHK(hipFree(e->ada_dbl));
  if (e->ada_int) HIPCHK(hipFree(e->ada_int));
  e->ada_leaf = e->ada_dbl = nullptr;
  e->ada_int = nullptr;
  return PTM_OK;
}

// A proposal_distribution_set of Gaussian members (proposal_distribution.cc:99-129) whose members are scalar multiples of
// the rung's factor -- the sampler's default Gaussian recipe (six diagonal Gaussians a factor gauss_step_fac apart with
// doubling shares, ptmcmc.cc:117-139).  Per local rung K members: cumulative shares (proposal_distribution_set's
// bin_max), scales, oneDfracs.  K = 0 removes the mixture.  last_type becomes member + 10 * (member's type).
extern "C" int ptm_set_proposal_mixture(ptm_engine* e, int K, const double* cum_shares, const double* scales, const double* one_d_fracs) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!e->have_prop) return fail(PTM_ERR_INVALID, "set the base proposals first (ptm_set_proposals)");
  if (K < 0 || K > 64) return fail(PTM_ERR_INVALID, "mixture size must be in 0..64");
  if (e->mix) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->mix)); e->mix = nullptr; }
  e->mix_K = 0;
  e->prior_member = -1; e->set_neg.clear();           // (the prior member is named anew for every set: ptm_set_proposal_prior_draw)
  { const int rc = ada_off(e); if (rc) return rc; }   // (a fixed mixture, or none, replaces an adaptive set)
  if (K == 0) return PTM_OK;
  if (!cum_shares || !scales || !one_d_fracs) return fail(PTM_ERR_INVALID, "null argument");
  const int nloc = e->nloc;
  std::vector<double> t((size_t)nloc * K * 3);
  int oned = 0;
  for (int r = 0; r < nloc; ++r)
    for (int k = 0; k < K; ++k) {
      const size_t i = (size_t)r * K + k;
      if (k > 0 && cum_shares[i] < cum_shares[i - 1]) return fail(PTM_ERR_INVALID, "cumulative shares must not decrease (rung %d)", r);
      if (one_d_fracs[i] < 0 || one_d_fracs[i] > 1) return fail(PTM_ERR_INVALID, "oneDfrac must be in [0,1]");
      t[3 * i] = cum_shares[i]; t[3 * i + 1] = scales[i]; t[3 * i + 2] = one_d_fracs[i];
      if (one_d_fracs[i] > 0) oned = 1;
    }
  int rc;
  if ((rc = dalloc(&e->mix, t.size())) || (rc = upload(e->mix, t.data(), t.size(), e->stream))) return rc;
  e->mix_K = K;
  e->set_neg.assign((size_t)K, 0);
  for (int r = 0; r < nloc; ++r)
    for (int k = 0; k < K; ++k)
      if (scales[(size_t)r * K + k] < 0) e->set_neg[k] = 1;
  if (oned) e->any_oned = 1;
  return PTM_OK;
}

// ---- adaptive proposal set (include/ptm_engine.h: ptm_set_proposal_adaptive) ------------------------------------------------
// A per-chain state (host layout [Nc][L] and [Nc][2]) checked against the set's shape: finite non-negative weights with a positive sum per
// set, thresholds non-decreasing in [0, 1] with each set's last exactly 1 (what reset_bins leaves), repeat bits of the set's members
// only, outcome counts >= 0.  Nothing is touched.
static int ada_check_state(const ptm_adaptive_set& a, size_t Nc, const double* w, const double* th, const int32_t* bits, const int32_t* cnt) {
  if (!w || !th || !bits || !cnt) return fail(PTM_ERR_INVALID, "null argument");
  const int L = a.K + a.K_inner;
  for (size_t c = 0; c < Nc; ++c)
    for (int b = 0; b < 2; ++b) {
      const int first = b ? a.K : 0, n = b ? a.K_inner : a.K;
      const int32_t bv = bits[c * 2 + b], cv = cnt[c * 2 + b];
      if (bv < 0 || (n < 31 && bv >= (1 << n)) || cv < 0)
        return fail(PTM_ERR_INVALID, "adaptive set: repeat bits name members of the set only and outcome counts are >= 0 (chain %zu)", c);
      if (n == 0) continue;
      double sum = 0.0, prev = 0.0;
      for (int k = 0; k < n; ++k) {
        const double wk = w[c * L + first + k], tk = th[c * L + first + k];
        if (!std::isfinite(wk) || wk < 0) return fail(PTM_ERR_INVALID, "adaptive set: weights must be finite and >= 0 (chain %zu)", c);
        if (!(tk >= prev && tk <= 1.0)) return fail(PTM_ERR_INVALID, "adaptive set: thresholds must not decrease and lie in [0, 1] (chain %zu)", c);
        sum += wk;
        prev = tk;
      }
      if (!(sum > 0)) return fail(PTM_ERR_INVALID, "adaptive set: the weights of a set must have a positive sum (chain %zu)", c);
      if (prev != 1.0) return fail(PTM_ERR_INVALID, "adaptive set: the last threshold of a set must be exactly 1 (chain %zu)", c);
    }
  return PTM_OK;
}
// host layout -> the device's structure of arrays (or back)
static void ada_to_soa(size_t Nc, int L, const double* w, const double* th, const int32_t* bits, const int32_t* cnt, std::vector<double>& dbl, std::vector<int>& in) {
  dbl.assign(2 * (size_t)L * Nc, 0.0);
  in.assign(4 * Nc, 0);
  for (size_t c = 0; c < Nc; ++c) {
    for (int k = 0; k < L; ++k) { dbl[(size_t)k * Nc + c] = w[c * L + k]; dbl[((size_t)L + k) * Nc + c] = th[c * L + k]; }
    for (int b = 0; b < 2; ++b) { in[(size_t)b * Nc + c] = bits[c * 2 + b]; in[(size_t)(2 + b) * Nc + c] = cnt[c * 2 + b]; }
  }
}

extern "C" int ptm_set_proposal_adaptive(ptm_engine* e, const ptm_adaptive_set* a, const double* scales, const double* one_d_fracs, const double* weights,
                                         const double* thresholds, const int32_t* repeat_bits, const int32_t* outcomes) {
  if (!e || !a || !scales || !one_d_fracs) return fail(PTM_ERR_INVALID, "null argument");
  SETTLE(e);
  NO_BATCH(e, "ptm_set_proposal_adaptive");
  // every check first: a refused call leaves the current proposals as they are
  if (!e->have_prop) return fail(PTM_ERR_INVALID, "set the base proposals first (ptm_set_proposals)");
  if (e->nloc != e->Nt)
    return fail(PTM_ERR_UNSUPPORTED, "an adaptive proposal set on a rung shard is not built: split the population by walkers (walker_begin)");
  if (a->K < 1 || a->K > 8) return fail(PTM_ERR_INVALID, "adaptive set: K must be in 1..8");
  if (a->nested < -1 || a->nested >= a->K) return fail(PTM_ERR_INVALID, "adaptive set: nested must be -1 or a top member");
  if (a->nested < 0 ? a->K_inner != 0 : (a->K_inner < 1 || a->K_inner > 8))
    return fail(PTM_ERR_INVALID, "adaptive set: K_inner must be 1..8 with a nested set, 0 without");
  if (!(a->rate >= 0 && a->rate < 1) || !(a->rate_inner >= 0 && a->rate_inner < 1)) return fail(PTM_ERR_INVALID, "adaptive set: rates must lie in [0, 1)");
  const int L = a->K + a->K_inner, nloc = e->nloc;
  const size_t Nc = e->Nc;
  int oned = 0;
  std::vector<double> leaf((size_t)nloc * L * 2);
  for (int r = 0; r < nloc; ++r) {
    int neg = 0;
    for (int k = 0; k < L; ++k) {
      const size_t i = (size_t)r * L + k;
      if (k == a->nested) { leaf[2 * i] = 1.0; leaf[2 * i + 1] = 0.0; continue; }   // (the nested set's own entry is not read)
      const double sc = scales[i], f = one_d_fracs[i];
      if (!std::isfinite(sc)) return fail(PTM_ERR_INVALID, "adaptive set: scales must be finite (rung %d)", r);
      if (!(f >= 0 && f <= 1)) return fail(PTM_ERR_INVALID, "oneDfrac must be in [0,1]");
      if (sc < 0) {
        if (k >= a->K) return fail(PTM_ERR_INVALID, "adaptive set: differential evolution (scale < 0) is a top member only (rung %d)", r);
        if (k == a->K - 1) return fail(PTM_ERR_INVALID, "adaptive set: differential evolution must not be the last top member (rung %d)", r);
        if (++neg > 1) return fail(PTM_ERR_INVALID, "adaptive set: at most one member with a negative scale (rung %d)", r);
      }
      leaf[2 * i] = sc; leaf[2 * i + 1] = f;
      if (f > 0) oned = 1;
    }
  }
  { const int rc = ada_check_state(*a, Nc, weights, thresholds, repeat_bits, outcomes); if (rc) return rc; }
  std::vector<double> dbl;
  std::vector<int> in;
  ada_to_soa(Nc, L, weights, thresholds, repeat_bits, outcomes, dbl, in);
  // the new arrays first, then the old configuration goes
  double *nleaf = nullptr, *ndbl = nullptr;
  int* nint = nullptr;
  int rc;
  if ((rc = dalloc(&nleaf, leaf.size())) || (rc = dalloc(&ndbl, dbl.size())) || (rc = dalloc(&nint, in.size()))) {
    if (nleaf) (void)hipFree(nleaf);
    if (ndbl) (void)hipFree(ndbl);
    return rc;
  }
  if ((rc = upload(nleaf, leaf.data(), leaf.size(), e->stream)) || (rc = upload(ndbl, dbl.data(), dbl.size(), e->stream)) ||
      (rc = upload(nint, in.data(), in.size(), e->stream))) {
    (void)hipFree(nleaf); (void)hipFree(ndbl); (void)hipFree(nint);
    return rc;
  }
  if ((rc = ada_off(e))) return rc;
  if (e->mix) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->mix)); e->mix = nullptr; }
  e->mix_K = 0;
  e->ada_leaf = nleaf; e->ada_dbl = ndbl; e->ada_int = nint;
  e->ada = *a;
  e->ada_on = true;
  e->prior_member = -1;   // (named anew for every set)
  e->set_neg.assign((size_t)a->K, 0);
  for (int r = 0; r < nloc; ++r)
    for (int k = 0; k < a->K; ++k)
      if (k != a->nested && scales[(size_t)r * L + k] < 0) e->set_neg[k] = 1;
  if (oned) e->any_oned = 1;
  return PTM_OK;
}

// can the engine's prior be drawn from, dimension by dimension, on the device?  (what a prior member needs: ptm_set_proposal_prior_draw)
static int prior_drawable(const ptm_engine* e) {
  if (e->prior_cb) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior (ptm_set_prior_callback) cannot be drawn from on the device: draw on the host (ptm_set_proposal_callback)");
  if (e->dprior) return fail(PTM_ERR_UNSUPPORTED, "a user prior on the device (ptm_set_prior_device) cannot be drawn from on the device: draw in a device proposal (ptm_set_proposal_device)");
  for (int d = 0; d < e->D; ++d)
    if (e->h_ptype[d] == PTM_PRIOR_FLAT) return fail(PTM_ERR_UNSUPPORTED, "a flat prior (dimension %d) cannot be drawn from", d);
  return PTM_OK;
}

// A member of the current set draws whole states from the prior (include/ptm_engine.h).  Every check first: a refused call changes nothing.
extern "C" int ptm_set_proposal_prior_draw(ptm_engine* e, int member) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  SETTLE(e);
  NO_BATCH(e, "ptm_set_proposal_prior_draw");
  if (member == -1) { e->prior_member = -1; return PTM_OK; }
  const int K = e->ada_on ? e->ada.K : e->mix_K;
  if (K == 0) return fail(PTM_ERR_INVALID, "no proposal set to name a member of (ptm_set_proposal_mixture, ptm_set_proposal_adaptive)");
  if (member < 0 || member >= K) return fail(PTM_ERR_INVALID, "prior draw: member %d is not one of the set's %d (top) members", member, K);
  if (e->ada_on && member == e->ada.nested) return fail(PTM_ERR_INVALID, "prior draw: member %d is the nested set", member);
  if (e->set_neg[member]) return fail(PTM_ERR_INVALID, "prior draw: member %d has a negative scale, which marks differential evolution", member);
  if (user_prop(e)) return fail(PTM_ERR_INVALID, "host-side proposals are set (ptm_set_proposal_callback): they replace every device proposal");
  { const int rc = prior_drawable(e); if (rc) return rc; }
  e->prior_member = member;
  return PTM_OK;
}

extern "C" int ptm_get_proposal_adapt_state(ptm_engine* e, double* weights, double* thresholds, int32_t* repeat_bits, int32_t* outcomes) {
  if (!e || !weights || !thresholds || !repeat_bits || !outcomes) return fail(PTM_ERR_INVALID, "null argument");
  SETTLE(e);
  if (!e->ada_on) return fail(PTM_ERR_INVALID, "no adaptive proposal set (ptm_set_proposal_adaptive)");
  const size_t Nc = e->Nc;
  const int L = e->ada.K + e->ada.K_inner;
  const unsigned char *sd, *si;
  FETCH(sd, e->ada_dbl, 2 * (size_t)L * Nc * 8);
  FETCH(si, e->ada_int, 4 * Nc * 4);
  e->fetch_after.push_back([=] {
    const double* d = (const double*)sd;
    const int* q = (const int*)si;
    for (size_t c = 0; c < Nc; ++c) {
      for (int k = 0; k < L; ++k) { weights[c * L + k] = d[(size_t)k * Nc + c]; thresholds[c * L + k] = d[((size_t)L + k) * Nc + c]; }
      for (int b = 0; b < 2; ++b) { repeat_bits[c * 2 + b] = q[(size_t)b * Nc + c]; outcomes[c * 2 + b] = q[(size_t)(2 + b) * Nc + c]; }
    }
  });
  return fetch_done(e);
}

extern "C" int ptm_set_proposal_adapt_state(ptm_engine* e, const double* weights, const double* thresholds, const int32_t* repeat_bits, const int32_t* outcomes) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  SETTLE(e);
  NO_BATCH(e, "ptm_set_proposal_adapt_state");
  if (!e->ada_on) return fail(PTM_ERR_INVALID, "no adaptive proposal set (ptm_set_proposal_adaptive)");
  const size_t Nc = e->Nc;
  const int L = e->ada.K + e->ada.K_inner;
  { const int rc = ada_check_state(e->ada, Nc, weights, thresholds, repeat_bits, outcomes); if (rc) return rc; }
  std::vector<double> dbl;
  std::vector<int> in;
  ada_to_soa(Nc, L, weights, thresholds, repeat_bits, outcomes, dbl, in);
  int rc;
  if ((rc = upload(e->ada_dbl, dbl.data(), dbl.size(), e->stream)) || (rc = upload(e->ada_int, in.data(), in.size(), e->stream))) return rc;
  return PTM_OK;
}

// Differential evolution drawn on the device (include/ptm_engine.h)
extern "C" int ptm_set_proposal_de(ptm_engine* e, const ptm_de_params* q, int n_init_extra, const double* init_rows) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  NO_BATCH(e, "ptm_set_proposal_de");
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->de_init) { HIPCHK(hipFree(e->de_init)); e->de_init = nullptr; }
  e->de_on = false; e->de_init_extra = 0;
  if (!q) return PTM_OK;
  if (e->DP > 128) return fail(PTM_ERR_UNSUPPORTED, "differential evolution on the device is built for up to 128 dimensions; above, draw it on the host (ptm_set_proposal_callback)");
  if (e->nloc != e->Nt)
    return fail(PTM_ERR_UNSUPPORTED, "differential evolution draws from EVERY rung's saved history, and a rung shard cannot record its top rung's: the row that "
                                     "rung holds between two exchanges of one step sits in the shard above (error bit 16).  Split the population by walkers "
                                     "(whole ladders per GPU: walker_begin) or draw on the host (ptm_set_proposal_callback)");
  if (e->hist.rungs != e->nloc || e->hist.cap < 2)
    return fail(PTM_ERR_INVALID, "differential evolution draws from every rung's saved history: create the engine with history_rungs = rung_count and a "
                                 "history_capacity that holds every row of the run");
  if (user_prop(e)) return fail(PTM_ERR_INVALID, "host-side proposals are set (ptm_set_proposal_callback): they replace every device proposal");
  if (!(q->snooker >= 0 && q->snooker <= 1) || !(q->gamma_one_frac >= 0 && q->gamma_one_frac <= 1) || !(q->reduce_gamma > 0) ||
      !(q->ignore_frac >= 0 && q->ignore_frac < 1) || n_init_extra < 0 || (n_init_extra > 0 && !init_rows))
    return fail(PTM_ERR_INVALID, "differential evolution: snooker and gamma_one_frac in [0, 1], reduce_gamma > 0, ignore_frac in [0, 1), init rows given");
  int rc;
  if (n_init_extra > 0) {
    const size_t Nc = e->Nc, D = e->D, DP = e->DP;
    std::vector<double> img((size_t)n_init_extra * Nc * DP, 0.0);
    for (size_t k = 0; k < (size_t)n_init_extra; ++k)
      for (size_t c = 0; c < Nc; ++c)
        for (size_t d = 0; d < D; ++d) img[(k * Nc + c) * DP + host_row_pos(DP, d)] = init_rows[(k * Nc + c) * D + d];
    if ((rc = dalloc(&e->de_init, img.size()))) return rc;
    HIPCHK(hipMemcpy(e->de_init, img.data(), img.size() * 8, hipMemcpyHostToDevice));
  }
  if (!e->de_hast && ((rc = dalloc(&e->de_hast, (size_t)e->Nc)) || (rc = dalloc(&e->de_type, (size_t)e->Nc)))) return rc;
  e->de = *q;
  e->de_init_extra = n_init_extra;
  e->de_on = true;
  return PTM_OK;
}

// The packing of one rung's factor, shared by ptm_set_proposal_rung and ptm_adapt_proposals: the padded column-major copy, the
// matrix-core tiles of the 32 / 64 / 128 padded dimensions, the box pre-pass's sigmas and margins, pf_dirty.
// pending: null: every copy is waited for (one rung); else the copies are only enqueued and their host images are kept in *pending
// until the caller has waited for the stream once (many rungs: no wait per rung).
static int install_rung_factor(ptm_engine* e, int local_rung, const double* factor, std::vector<std::vector<double> >* pending = nullptr) {
  auto put = [e, pending](double* dst, std::vector<double>& img) -> int {
    if (!pending) return upload(dst, img.data(), img.size(), e->stream);
    pending->emplace_back(std::move(img));   // (a vector's buffer stays where it is when the vector is moved)
    HIPCHK(hipMemcpyAsync(dst, pending->back().data(), pending->back().size() * sizeof(double), hipMemcpyDefault, e->stream));
    return PTM_OK;
  };
  const int D = e->D, DP = e->DP, kind = e->prop_kind == KIND_DIAG ? PTM_PROP_DIAG : (e->prop_kind == KIND_LOWER ? PTM_PROP_LOWER : PTM_PROP_DENSE);
  std::vector<double> packed((size_t)e->prop_stride, 0.0);
  if (kind == PTM_PROP_DIAG) {
    for (int d = 0; d < D; ++d) packed[d] = factor[d];
  } else {
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        if (kind == PTM_PROP_LOWER && j > i && factor[(size_t)i * D + j] != 0.0)
          return fail(PTM_ERR_INVALID, "PTM_PROP_LOWER factor has a non-zero above the diagonal");
        packed[(size_t)j * DP + i] = factor[(size_t)i * D + j];
      }
  }
  int rc;
  if ((rc = put(e->prop + (size_t)local_rung * e->prop_stride, packed))) return rc;
  if (DP == 32) {
    std::vector<double> tiles(16 * 64, 0.0);
    for (int t = 0; t < 16; ++t) {
      const int rt = t & 1, sl = (t >> 1) & 3, hb = t >> 3;
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 16; ++i) {
          const int row = 16 * rt + i, col = 16 * hb + 4 * k + sl;
          if (row < D && col < D)
            tiles[(size_t)t * 64 + 16 * k + i] = kind == PTM_PROP_DIAG ? (row == col ? factor[row] : 0.0) : factor[(size_t)row * D + col];
        }
    }
    if ((rc = put(e->prop_tiles + (size_t)local_rung * 16 * 64, tiles))) return rc;
  }
  if (DP == 64 || DP == 128) {
    const int NT = DP / 16, ntile = NT * NT * 4;
    std::vector<double> tiles((size_t)ntile * 64, 0.0);
    for (int t = 0; t < ntile; ++t) {
      const int rt = t % NT, sl = (t / NT) & 3, hb = t / (4 * NT);
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 16; ++i) {
          const int row = 16 * rt + i, col = 16 * hb + 4 * k + sl;
          if (row < D && col < D)
            tiles[(size_t)t * 64 + 16 * k + i] = kind == PTM_PROP_DIAG ? (row == col ? factor[row] : 0.0) : factor[(size_t)row * D + col];
        }
    }
    if ((rc = put(e->prop_tiles + (size_t)local_rung * ntile * 64, tiles))) return rc;
  }
  prefilter_sigmas(kind == PTM_PROP_DIAG, factor, D, &e->pf_sigma[(size_t)local_rung * PREFILTER_DIMS]);
  prefilter_margins(kind == PTM_PROP_DIAG, factor, D, &e->pf_margin_nat[(size_t)local_rung * PREFILTER_DIMS]);
  e->pf_dirty = true;
  return PTM_OK;
}
// One rung's factor replaced between steps -- what user_gaussian_prop::check_update achieves in the reference when its
// callback returns a new covariance for a chain (proposal_distribution.cc:406-441, reset_dist :340-403).  Same kind and
// storage as the factors set by ptm_set_proposals; one_d_frac < 0 keeps the rung's current value.
extern "C" int ptm_set_proposal_rung(ptm_engine* e, int local_rung, const double* factor, double one_d_frac) {
  SETTLE(e);
  if (!e || !factor) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->have_prop) return fail(PTM_ERR_INVALID, "set all proposals first (ptm_set_proposals)");
  if (local_rung < 0 || local_rung >= e->nloc) return fail(PTM_ERR_INVALID, "rung out of the shard");
  int rc = install_rung_factor(e, local_rung, factor);
  if (rc) return rc;
  if (one_d_frac >= 0) {
    if (one_d_frac > 1) return fail(PTM_ERR_INVALID, "oneDfrac must be in [0,1]");
    if ((rc = upload(e->onedfrac + local_rung, &one_d_frac, 1, e->stream))) return rc;
    if (one_d_frac > 0) e->any_oned = 1;
  }
  return PTM_OK;
}

// ---- kernel argument block ----------------------------------------------------------------------------------
static Dev make_dev(ptm_engine* e, bool labelled = false) {   // labelled: the compacted sweep of a labelled step, which finds the rows by their labels
  Dev p;
  memset(&p, 0, sizeof p);
  p.D = e->D; p.DP = e->DP; p.Nt = e->Nt; p.r0 = e->r0; p.nloc = e->nloc; p.W = e->W; p.Nc = e->Nc; p.w_off = e->cfg.walker_begin;
  p.seed = e->cfg.seed; p.step = e->step; p.add_every_n = e->cfg.add_every_n; p.min_prior = e->cfg.min_prior;
  p.has_bounds = e->has_bounds; p.origin_valid = e->origin_valid; p.bounds_box = e->bounds_box;
  p.blo = e->blo; p.bhi = e->bhi; p.bmin = e->bmin; p.bmax = e->bmax;
  p.all_uniform = e->all_uniform; p.lprior_const = e->lprior_const;
  p.ptype = e->ptype; p.plo = e->plo; p.phi = e->phi; p.pcoef = e->pcoef;
  p.P2 = e->P2; p.mean = e->mean; p.has_mean = e->has_mean; p.like0 = e->like0;
  p.beta = e->beta; p.prop = e->prop; p.prop_tiles = e->prop_tiles; p.P2_tiles = e->P2_tiles; p.box_row = e->box_row; p.onedfrac = e->onedfrac; p.prop_stride = e->prop_stride; p.any_oned = e->any_oned;
  p.mix_K = e->mix_K; p.mix = e->mix;
  p.de_on = e->de_on ? 1 : 0; p.de_init_extra = e->de_init_extra; p.de_init = e->de_init; p.de_hast = e->de_hast; p.de_type = e->de_type;
  p.de_snooker = e->de.snooker; p.de_gamma_one = e->de.gamma_one_frac; p.de_gamma_div = e->de.reduce_gamma; p.de_ignore = e->de.ignore_frac;
  p.de_gamma_std = e->de_on ? 1.68 / std::sqrt((double)e->D) / e->de.reduce_gamma : 0.0;   // (the reference's own expression, proposal_distribution.cc:492)
  p.prior_k = e->prior_member + 1;
  p.betaC = e->betaC; p.beta_add = e->beta_add; p.beta_w = e->beta_w;
  p.x = labelled ? e->xdev : xrows(e); p.ll = e->ll; p.lp = e->lp;
  p.ntries = e->ntries; p.naccept = e->naccept; p.last_type = e->last_type; p.nhist = e->nhist;
  p.touch = e->touch; p.err = e->err;
  p.hist = e->hist;
  p.map = e->map;
  p.c_begin = 0; p.c_end = e->Nc;
  p.host_prop = user_prop(e) ? 1 : 0; p.hastings = e->hastings; p.htype = e->htype; p.hvalid = e->hvalid; p.acc_out = e->acc_out;
  return p;
}

// the adaptive set's kernel argument (zero without one)
static AdaArgs make_ada(const ptm_engine* e) {
  AdaArgs a;
  memset(&a, 0, sizeof a);
  if (!e->ada_on) return a;
  const size_t L = (size_t)e->ada.K + e->ada.K_inner, Nc = e->Nc;
  a.K = e->ada.K; a.nested = e->ada.nested; a.Ki = e->ada.K_inner; a.rate = e->ada.rate; a.rate_in = e->ada.rate_inner;
  a.leaf = e->ada_leaf; a.w = e->ada_dbl; a.th = e->ada_dbl + L * Nc; a.bits = e->ada_int; a.cnt = e->ada_int + 2 * Nc;
  return a;
}

// the launches of a padded dimension's translation unit (ptm_launch.hpp)
const DpLaunch* ptm::dp_launch(int DP) {
  switch (DP) {
    case 4: return &dp_launch_4;
    case 8: return &dp_launch_8;
    case 16: return &dp_launch_16;
    case 32: return &dp_launch_32;
    case 64: return &dp_launch_64;
    case 128: return &dp_launch_128;
    case 256: return &dp_launch_256;
    case 512: return &dp_launch_512;
    case 1024: return &dp_launch_1024;
  }
  return nullptr;
}

// a user likelihood, on the host (ptm_set_target_callback) or on the device (ptm_set_target_device): the propose / accept passes
static inline bool user_like(const ptm_engine* e) { return e->cb != nullptr || e->dfn != nullptr; }

// the build a sweep over `chains` chains runs on (ptm_sweep_plan.hpp); step_sweep_plan: the sweep of a PT step -- every local rung, after an
// exchange phase -- which is what the engine prepares for (row labels, temperatures) and what it reports by name
static SweepFacts sweep_facts(const ptm_engine* e, long long chains, bool touched) {
  SweepFacts f;
  memset(&f, 0, sizeof f);
  f.DP = e->DP; f.W = e->W; f.chains = chains; f.nloc = e->nloc;
  f.kind = e->prop_kind == PTM_PROP_DIAG ? PLAN_DIAG : (e->prop_kind == PTM_PROP_LOWER ? PLAN_LOWER : PLAN_DENSE);
  f.has_bounds = e->has_bounds; f.bounds_box = e->bounds_box; f.all_uniform = e->all_uniform; f.has_mean = e->has_mean; f.any_oned = e->any_oned;
  f.mix_K = e->mix_K;
  f.evolving = e->betaC != nullptr; f.tracked = e->hist.rungs || e->map.rungs;
  f.user_like = user_like(e); f.host_prop = user_prop(e); f.ada = e->ada_on;
  f.de = e->de_on || e->prior_member >= 0;   // (a prior member routes as differential evolution does: only the lanes and general kernels draw it)
  f.mode = f.user_like ? 1 : 0;   // (the propose and accept passes run on one build)
  f.touched = touched;
  f.prior_draw = e->prior_member >= 0; f.history = e->hist.rungs > 0 && e->hist.rungs == e->nloc;
  return f;
}
static SweepPlan sweep_plan(const ptm_engine* e, long long chains, bool touched) { return plan_sweep(sweep_facts(e, chains, touched), sweep_env()); }
static SweepPlan step_sweep_plan(const ptm_engine* e) { return sweep_plan(e, e->Nc, true); }
// Differential evolution on the matrix cores: does de_mfma32_kernel (ptm_de_mfma_kernel.hpp) run the sweep over `chains` chains in place of
// the plan's kernel?  Asked here for PT steps, ptm_sweep and ptm_sweep_rungs alike (launch_sweep) and for the reported name.  The
// preparations stay the plan's -- a general sweep: chain-indexed temperatures kept current, no row labels, no partition.
static bool de_mfma_sweep(const ptm_engine* e, long long chains) { return e->de_on && de_mfma_applies(sweep_facts(e, chains, true), sweep_env()); }

static bool lean_ev_sweeps(const ptm_engine* e) { return reads_ladder_major_beta(step_sweep_plan(e)); }

// the compacted sweep counts a step's add_state calls for all chains at once: bring nhist up to date before anything reads it
static int flush_nhist(ptm_engine* e) {
  if (!e->nhist_pending) return PTM_OK;
  hipLaunchKernelGGL(nhist_flush_kernel, dim3((unsigned)(((size_t)e->Nc + 255) / 256)), dim3(256), 0, e->stream, e->nhist, (size_t)e->Nc, e->nhist_pending);
  HIPCHK(hipGetLastError());
  e->nhist_pending = 0;
  return PTM_OK;
}

// Row labels: does a whole step of this engine (exchange phase, then ONE sweep of all rungs) exchange labels instead of rows?  Where its
// sweep is the compacted one, the engine holds the whole ladder, and a walker fits the 16 bits a list entry leaves it.
// PTM_ROW_LABELS=0 switches it off.
static bool row_labels_apply(const ptm_engine* e) {
  static const bool labels_ok = [] { const char* v = getenv("PTM_ROW_LABELS"); return !(v && *v == '0'); }();
  return labels_ok && e->nloc == e->Nt && !e->shard && e->W <= 65536 && e->Nt > 1 && step_sweep_plan(e).compacted;
}
static void flush_rows(ptm_engine* e) {
  e->rows_labelled = false;
  hipLaunchKernelGGL(restore_rows_kernel, dim3(e->W), dim3(256), (size_t)4 * e->nloc, e->stream, e->xdev, e->rowof, e->W, e->nloc, e->DP);
}

// one fused MH sweep over local rungs [rung0, rung0 + nr); `last` closes the step (the step count is the RNG position)
// host-callback likelihood, between the propose pass and the accept pass: the gated proposals to the host, the user's function on
// them (the prior's first if it is a callback too), the new llikes back
static int ensure_betaC(ptm_engine* e);
static int callback_host_part(ptm_engine* e) {
  const size_t Nc = e->Nc, DP = e->DP;
  HIPCHK(copy_unless_shared(e->h_xprop.data(), e->xprop, Nc * DP * 8 + Nc, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->prior_cb) {
    // host-evaluated prior: the valid proposals' log-priors, then the reference's prior gate on them -- want_like (chain.cc:980)
    // with oldlprior = current_lpost - invtemp * current_llike (:973), rounded as the kernels round it
    std::vector<double> hll(Nc), hlp(Nc), hbeta(Nc), out;
    HIPCHK(hipMemcpy(hll.data(), e->ll, Nc * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hlp.data(), e->lp, Nc * 8, hipMemcpyDeviceToHost));
    { int rc2 = ensure_betaC(e); if (rc2) return rc2; }
    if (e->betaC) HIPCHK(hipMemcpy(hbeta.data(), e->betaC, Nc * 8, hipMemcpyDeviceToHost));
    std::vector<size_t> vp;
    for (size_t c = 0; c < Nc; ++c)
      if (e->h_gate[c] & 1) vp.push_back(c);
    int rcp = call_user_prior(e, e->h_xprop, vp, out);
    if (rcp) return rcp;
    std::vector<double> lpn(Nc, -__builtin_inf());
    for (size_t k = 0; k < vp.size(); ++k) {
      const size_t c = vp[k];
      const double beta = e->betaC ? hbeta[c] : e->h_beta[e->r0 + c / e->W];
      lpn[c] = out[k];
      e->h_gate[c] = prior_gate(out[k], hlp[c], hll[c], beta, e->cfg.min_prior);   // (ptm_devprior_kernels.hpp: the device prior's kernel applies the same function)
    }
    HIPCHK(hipMemcpyAsync(e->lprior_new, lpn.data(), Nc * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(copy_unless_shared(e->gate, e->h_gate, Nc, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // (lpn is a local)
  }
  std::vector<size_t> pick;
  for (size_t c = 0; c < Nc; ++c)
    if (e->h_gate[c] & 2) pick.push_back(c);
  int rc = call_user(e, e->h_xprop, pick, e->h_llbatch);
  if (rc) return rc;
  for (size_t k = 0; k < pick.size(); ++k) e->h_llnew[pick[k]] = e->h_llbatch[k];
  HIPCHK(copy_unless_shared(e->llike_new, e->h_llnew.data(), Nc * 8, hipMemcpyHostToDevice, e->stream));
  return PTM_OK;
}

// ---- device likelihood (ptm_set_target_device) ----------------------------------------------------------------------------
// pack the selected chains' rows ((gate & gmask) == gval; gate == nullptr: all) into the batch, call the user's function on the
// stream, scatter its llikes into dst by chain (gate_out: the redraw loop's verdicts) and -- best -- fold lprior + llike of the
// evaluated rows into the kept best.  Everything is queued; nothing waits.
static int devlike_eval(ptm_engine* e, const unsigned char* gate, int gmask, int gval, const double* xsel, const double* xrest, double* dst,
                        unsigned char* gate_out, const double* lprior, bool best) {
  const int n = e->Nc, D = e->D;
  const int nchunk = (n + DL_CHUNK - 1) / DL_CHUNK;
  hipLaunchKernelGGL(devlike_count_kernel, dim3(nchunk), dim3(DL_CHUNK), 0, e->stream, n, gate, gmask, gval, e->dl_chunks);
  HIPCHK(hipGetLastError());
#define PTM_DL_PACK(N) case N: hipLaunchKernelGGL((devlike_pack_kernel<N>), dim3(nchunk), dim3(DL_CHUNK), 0, e->stream, n, D, nchunk, gate, gmask, gval, \
                                                  (const int*)e->dl_chunks, xsel, xrest, e->dl_x, e->dl_rows, e->dl_count); break;
  switch (e->DP) {
    PTM_DL_PACK(4) PTM_DL_PACK(8) PTM_DL_PACK(16) PTM_DL_PACK(32) PTM_DL_PACK(64) PTM_DL_PACK(128) PTM_DL_PACK(256) PTM_DL_PACK(512) PTM_DL_PACK(1024)
    default: return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  }
#undef PTM_DL_PACK
  HIPCHK(hipGetLastError());
  if (!xrest) {
    const size_t tot = (size_t)n * D;
    hipLaunchKernelGGL(devlike_fill_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, e->stream, n, D, (const int32_t*)e->dl_count, e->dl_x);
    HIPCHK(hipGetLastError());
  }
  e->dfn(e->dfn_user, (void*)e->stream, n, D, e->dl_x, e->dl_count, e->dl_ll);
  hipLaunchKernelGGL(devlike_scatter_kernel, dim3(1), dim3(DL_SCATTER_THREADS), 0, e->stream, D, (const int32_t*)e->dl_count, (const int*)e->dl_rows,
                     (const double*)e->dl_ll, dst, gate_out, lprior, (const double*)e->dl_x, best ? e->dl_best : nullptr);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

// the best posterior seen: none yet (-inf, the zero state: bayes_likelihood::reset)
static int devlike_reset_best(ptm_engine* e) {
  if (!e->dl_best) return PTM_OK;
  std::vector<double> b((size_t)e->D + 1, 0.0);
  b[0] = -__builtin_inf();
  return upload(e->dl_best, b.data(), b.size(), e->stream);
}

extern "C" int ptm_set_target_device(ptm_engine* e, ptm_loglike_device_fn fn, void* user, double* x_batch_dev, double* llike_batch_dev) {
  if (!e || !fn) return fail(PTM_ERR_INVALID, "null argument");
  SETTLE(e);
  NO_BATCH(e, "ptm_set_target_device");
  if (e->prior_cb) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior with a device likelihood is not built (ptm_set_prior_callback)");
  if (e->pcb) return fail(PTM_ERR_UNSUPPORTED, "host-side proposals with a device likelihood are not built (ptm_set_proposal_callback)");
  if (e->nloc != e->Nt) return fail(PTM_ERR_UNSUPPORTED, "a device likelihood on a rung shard is not built: split such a population by walkers");
  const size_t Nc = e->Nc, D = e->D, DP = e->DP;
  int rc;
  if (!e->dl_count &&
      ((rc = dalloc(&e->dl_count, 1)) || (rc = dalloc(&e->dl_rows, Nc)) || (rc = dalloc(&e->dl_chunks, (Nc + DL_CHUNK - 1) / DL_CHUNK)) ||
       (rc = dalloc(&e->dl_xprop, Nc * DP)) || (rc = dalloc(&e->dl_gate, Nc)) || (rc = dalloc(&e->dl_lprior_new, Nc)) ||
       (rc = dalloc(&e->dl_llike_new, Nc)) || (rc = dalloc(&e->dl_best, D + 1))))
    return rc;
  // the batch buffers: the caller's, or the engine's own (kept across calls)
  if (x_batch_dev) {
    if (e->dl_own_x && e->dl_x) { HIPCHK(hipStreamSynchronize(e->stream)); (void)hipFree(e->dl_x); }
    e->dl_x = x_batch_dev; e->dl_own_x = false;
  } else if (!e->dl_own_x) {
    e->dl_x = nullptr;
    if ((rc = dalloc(&e->dl_x, Nc * D))) return rc;
    e->dl_own_x = true;
  }
  if (llike_batch_dev) {
    if (e->dl_own_ll && e->dl_ll) { HIPCHK(hipStreamSynchronize(e->stream)); (void)hipFree(e->dl_ll); }
    e->dl_ll = llike_batch_dev; e->dl_own_ll = false;
  } else if (!e->dl_own_ll) {
    e->dl_ll = nullptr;
    if ((rc = dalloc(&e->dl_ll, Nc))) return rc;
    e->dl_own_ll = true;
  }
  HIPCHK(hipMemsetAsync(e->dl_gate, 0, Nc, e->stream));
  HIPCHK(hipMemsetAsync(e->dl_xprop, 0, Nc * DP * 8, e->stream));   // (device proposals: the sweep reads, and never uses, the rows of chains that make no move)
  if ((rc = devlike_reset_best(e))) return rc;
  e->dfn = fn; e->dfn_user = user;
  e->cb = nullptr;   // (the last target setter wins)
  e->have_target = 1;
  return PTM_OK;
}

extern "C" int ptm_target_device_rows(ptm_engine* e) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  return e->Nc;
}

// ---- device prior (ptm_set_prior_device) ----------------------------------------------------------------------------------
extern "C" int ptm_set_prior_device(ptm_engine* e, ptm_logprior_device_fn fn, void* user) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  SETTLE(e);
  NO_BATCH(e, "ptm_set_prior_device");
  if (!fn) {   // back to the device-side prior of ptm_set_prior (the chains' lpriors are made anew by the next ptm_set_states / ptm_restore)
    e->dprior = nullptr; e->dprior_user = nullptr;
    return PTM_OK;
  }
  if (e->prior_cb) return fail(PTM_ERR_UNSUPPORTED, "a device prior beside a host-evaluated prior is not built: remove that one first (ptm_set_prior_callback)");
  if (e->pcb) return fail(PTM_ERR_UNSUPPORTED, "host-side proposals with a device prior are not built (ptm_set_proposal_callback)");
  if (e->nloc != e->Nt) return fail(PTM_ERR_UNSUPPORTED, "a device prior on a rung shard is not built: split such a population by walkers");
  const size_t Nc = e->Nc, D = e->D;
  int rc;
  if (!e->pr_count &&
      ((rc = dalloc(&e->pr_x, Nc * D)) || (rc = dalloc(&e->pr_lp, Nc)) || (rc = dalloc(&e->pr_rows, Nc)) ||
       (rc = dalloc(&e->pr_chunks, (Nc + DL_CHUNK - 1) / DL_CHUNK)) || (rc = dalloc(&e->pr_count, 1))))
    return rc;
  e->dprior = fn; e->dprior_user = user;
  e->lp_is_const = false;
  return PTM_OK;
}

// a device prior runs between the propose pass and the device likelihood's pack: without that likelihood there is no place for it
static int devprior_ready(const ptm_engine* e) {
  if (e->dprior && !e->dfn) return fail(PTM_ERR_UNSUPPORTED, "a device prior needs the device likelihood (ptm_set_target_device)");
  return PTM_OK;
}

// count + pack of the chains with (gate & 1) == 1 into the prior's batch, then the user's function on the stream.  xrest == nullptr: the
// rows past the count become copies of row 0 (set-up: the other chains hold no state to trust)
static int devprior_call(ptm_engine* e, const unsigned char* gate, const double* xsel, const double* xrest) {
  const int n = e->Nc, D = e->D;
  const int nchunk = (n + DL_CHUNK - 1) / DL_CHUNK;
  hipLaunchKernelGGL(devlike_count_kernel, dim3(nchunk), dim3(DL_CHUNK), 0, e->stream, n, gate, 1, 1, e->pr_chunks);
  HIPCHK(hipGetLastError());
#define PTM_PR_PACK(N) case N: hipLaunchKernelGGL((devlike_pack_kernel<N>), dim3(nchunk), dim3(DL_CHUNK), 0, e->stream, n, D, nchunk, gate, 1, 1, \
                                                  (const int*)e->pr_chunks, xsel, xrest, e->pr_x, e->pr_rows, e->pr_count); break;
  switch (e->DP) {
    PTM_PR_PACK(4) PTM_PR_PACK(8) PTM_PR_PACK(16) PTM_PR_PACK(32) PTM_PR_PACK(64) PTM_PR_PACK(128) PTM_PR_PACK(256) PTM_PR_PACK(512) PTM_PR_PACK(1024)
    default: return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  }
#undef PTM_PR_PACK
  HIPCHK(hipGetLastError());
  if (!xrest) {
    const size_t tot = (size_t)n * D;
    hipLaunchKernelGGL(devlike_fill_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, e->stream, n, D, (const int32_t*)e->pr_count, e->pr_x);
    HIPCHK(hipGetLastError());
  }
  e->dprior(e->dprior_user, (void*)e->stream, n, D, e->pr_x, e->pr_count, e->pr_lp);
  return PTM_OK;
}

// a step's prior phase, behind the propose pass: the valid proposals' log-priors from the user's function, then the prior gate on them
// (devprior_gate_kernel): lprior_new and the gate bytes the likelihood's pack and the accept pass read.  Queued; nothing waits.
static int devprior_stage(ptm_engine* e) {
  const int n = e->Nc;
  const double* xcur = xrows(e);
  int rc = ensure_betaC(e);
  if (rc) return rc;
  if ((rc = devprior_call(e, e->dl_gate, e->dl_xprop, xcur))) return rc;
  hipLaunchKernelGGL(devprior_gate_kernel, dim3((unsigned)((n + DEVPRIOR_THREADS - 1) / DEVPRIOR_THREADS)), dim3(DEVPRIOR_THREADS), 0, e->stream, n, e->W, e->r0,
                     (const int32_t*)e->pr_count, (const int*)e->pr_rows, (const double*)e->pr_lp, (const double*)e->lp, (const double*)e->ll,
                     (const double*)e->beta, (const double*)e->betaC, e->cfg.min_prior, e->dl_lprior_new, e->dl_gate);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

// set-up (ptm_set_states, ptm_restore): the user's log-priors replace what the device-side prior gave the valid states (lprior above
// -inf), as host_prior_of_states does for a host prior; dl_gate is free between steps (the propose pass writes every chain's byte)
static int devprior_of_states(ptm_engine* e) {
  const int n = e->Nc;
  const unsigned grid = (unsigned)((n + DEVPRIOR_THREADS - 1) / DEVPRIOR_THREADS);
  const double* x = xrows(e);
  hipLaunchKernelGGL(devprior_valid_kernel, dim3(grid), dim3(DEVPRIOR_THREADS), 0, e->stream, n, (const double*)e->lp, e->dl_gate);
  HIPCHK(hipGetLastError());
  int rc = devprior_call(e, e->dl_gate, x, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(devprior_states_kernel, dim3(grid), dim3(DEVPRIOR_THREADS), 0, e->stream, n, (const int32_t*)e->pr_count, (const int*)e->pr_rows,
                     (const double*)e->pr_lp, e->lp);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

// the device prior of ptm_debug_evaluate's rows (natural order, enforced): those that are valid and inside the device-side prior, in
// batches of the engine's n_rows (rows past the count: the batch's first row)
static int devprior_debug(ptm_engine* e, const double* X, int n, const int32_t* valid, double* lprior) {
  const size_t Nc = e->Nc, D = e->D;
  std::vector<size_t> pick;
  for (size_t k = 0; k < (size_t)n; ++k)
    if (valid[k] && lprior[k] > -__builtin_inf()) pick.push_back(k);
  std::vector<double> rows(Nc * D), out(Nc);
  for (size_t k0 = 0; k0 < pick.size(); k0 += Nc) {
    const size_t m = std::min(Nc, pick.size() - k0);
    for (size_t k = 0; k < Nc; ++k) memcpy(&rows[k * D], X + pick[k0 + (k < m ? k : 0)] * D, D * 8);
    const int32_t cnt = (int32_t)m;
    HIPCHK(hipMemcpyAsync(e->pr_x, rows.data(), Nc * D * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->pr_count, &cnt, 4, hipMemcpyHostToDevice, e->stream));
    e->dprior(e->dprior_user, (void*)e->stream, (int)Nc, (int)D, e->pr_x, e->pr_count, e->pr_lp);
    HIPCHK(hipMemcpyAsync(out.data(), e->pr_lp, m * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // (rows, cnt and out are reused)
    for (size_t k = 0; k < m; ++k) lprior[pick[k0 + k]] = out[k];
  }
  return PTM_OK;
}

extern "C" int ptm_get_best_evaluated(ptm_engine* e, double* lpost, double* x) {
  if (!e || !lpost) return fail(PTM_ERR_INVALID, "null argument");
  SETTLE(e);
  NO_BATCH(e, "ptm_get_best_evaluated");
  if (!e->dl_best) return fail(PTM_ERR_INVALID, "no device likelihood set (ptm_set_target_device)");
  std::vector<double> b((size_t)e->D + 1);
  HIPCHK(hipMemcpyAsync(b.data(), e->dl_best, b.size() * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *lpost = b[0];
  if (x) memcpy(x, b.data() + 1, (size_t)e->D * 8);
  return PTM_OK;
}

// the device likelihood of ptm_debug_evaluate's rows (natural order, enforced), in batches of the engine's n_rows
static int devlike_debug(ptm_engine* e, const double* X, int n, double* llike) {
  const size_t Nc = e->Nc, D = e->D;
  std::vector<double> rows(Nc * D);
  for (size_t k0 = 0; k0 < (size_t)n; k0 += Nc) {
    const size_t m = std::min(Nc, (size_t)n - k0);
    for (size_t k = 0; k < Nc; ++k) memcpy(&rows[k * D], X + (k0 + (k < m ? k : 0)) * D, D * 8);   // (rows past the count: row 0)
    const int32_t cnt = (int32_t)m;
    HIPCHK(hipMemcpyAsync(e->dl_x, rows.data(), Nc * D * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->dl_count, &cnt, 4, hipMemcpyHostToDevice, e->stream));
    e->dfn(e->dfn_user, (void*)e->stream, (int)Nc, (int)D, e->dl_x, e->dl_count, e->dl_ll);
    HIPCHK(hipMemcpyAsync(llike + k0, e->dl_ll, m * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // (rows and cnt are reused)
  }
  return PTM_OK;
}

// a shard's exchange phases and partial sweeps: not with a device likelihood
#define NO_DEVLIKE(e, name) do { if ((e) && (e)->dfn) return fail(PTM_ERR_UNSUPPORTED, name " with a device likelihood is not built (rung-sharded steps)"); \
                                 if ((e) && (e)->dprior) return fail(PTM_ERR_UNSUPPORTED, name " with a device prior is not built (rung-sharded steps)"); } while (0)

// box pre-pass: which local rungs it takes (ptm_sweep_plan.hpp: prefilter_flag), from the proposals' spread and the prior box.
// pf_sigma follows every writer of prop_tiles (ptm_set_proposals, ptm_set_proposal_rung: there is no other -- mixtures, adaptive sets and
// differential evolution keep a sweep off this kernel family or off its lean build); a setter that marks pf_dirty has waited for the
// stream, so the pinned staging buffer is free when it is rewritten here and the upload is queued without a host wait.
static int prefilter_flags(ptm_engine* e) {
  const int nd = e->D < PREFILTER_DIMS ? e->D : PREFILTER_DIMS;
  double width[PREFILTER_DIMS];
  for (int d = 0; d < nd; ++d) width[d] = e->h_phi[d] - e->h_plo[d];
  if (!e->h_pf_flag) HIPCHK(hipHostMalloc((void**)&e->h_pf_flag, (size_t)e->nloc, hipHostMallocDefault));
  unsigned char* fl = e->h_pf_flag;
  e->pf_flagged = 0;
  for (int r = 0; r < e->nloc; ++r) {
    fl[r] = (e->pf_sigma.size() == (size_t)e->nloc * PREFILTER_DIMS && prefilter_flag(&e->pf_sigma[(size_t)r * PREFILTER_DIMS], width, nd, sweep_env().prefilter)) ? 1 : 0;
    e->pf_flagged += fl[r];
  }
  HIPCHK(hipMemcpyAsync(e->pf_flag, fl, (size_t)e->nloc, hipMemcpyHostToDevice, e->stream));
  // the single-precision kernel's margins: the factor's (infinite while there is none: nothing settles) plus the faces' slack, as
  // floats; lane group q of a wave owns dimensions q + 4 i and reads its four side by side
  const size_t nm = (size_t)e->nloc * PREFILTER_DIMS;
  if (!e->h_pf_margin) HIPCHK(hipHostMalloc((void**)&e->h_pf_margin, nm * sizeof(float), hipHostMallocDefault));
  for (int r = 0; r < e->nloc; ++r)
    for (int d = 0; d < PREFILTER_DIMS; ++d)
      e->h_pf_margin[(size_t)r * PREFILTER_DIMS + 4 * (d & 3) + (d >> 2)] = d >= nd ? 0.0f :
          prefilter_margin_f32((e->pf_margin_nat.size() == nm ? e->pf_margin_nat[(size_t)r * PREFILTER_DIMS + d] : INFINITY) + prefilter_face_slack(e->h_plo[d], e->h_phi[d]));
  HIPCHK(hipMemcpyAsync(e->pf_margin, e->h_pf_margin, nm * sizeof(float), hipMemcpyHostToDevice, e->stream));
  e->pf_dirty = false;
  return PTM_OK;
}

// the box pre-pass over local rungs [rung0, rung0 + nr) of rows x, behind partition_kernel and in front of the compacted sweep
static int launch_box_prefilter(ptm_engine* e, const double* x, int rung0, int nr, bool labelled) {
  BoxPreF32 bf;
  memset(&bf, 0, sizeof bf);
  BoxPre& b = bf.b;
  b.W = e->W; b.Nt = e->Nt; b.r0 = e->r0; b.w_off = e->cfg.walker_begin; b.rung0 = rung0; b.nrung = nr; b.labelled = labelled ? 1 : 0;
  b.seed = e->cfg.seed; b.step = e->step;
  b.x = x; b.ll = e->ll; b.lp = e->lp; b.beta = e->beta; b.prop_tiles = e->prop_tiles; b.box_row = e->box_row; b.ntries = e->ntries;
  b.pidx = e->pidx; b.pcnt = e->pcnt; b.cidx = e->cidx; b.ccnt = e->ccnt; b.counts = e->pf_counts;
  bf.margin = e->pf_margin;
  // single precision behind a margin unless PTM_BOX_PREFILTER_EXACT asks for the sweep's own arithmetic: the same chains either way
  struct { const void* fn; bool tables; } k = {(const void*)box_prefilter_f32_kernel, false};
  if (sweep_env().prefilter_exact != 0) { k.fn = (const void*)box_prefilter_kernel; k.tables = true; }
  if (!e->pf_grid) {   // a persistent grid: the blocks the device holds at once, of the kernel that is launched
    int per_cu = 0, dev = 0;
    hipDeviceProp_t pr;
    const hipError_t oc = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, 256, BoxPreLds(nullptr, k.tables, e->nloc).bytes);
    if (oc != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); per_cu = 2; }
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipGetDeviceProperties(&pr, dev));
    e->pf_grid = per_cu * (pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256);
    const int cap = sweep_env().prefilter_grid;   // PTM_PREFILTER_GRID: many tiles per block on a small population (tests)
    if (cap > 0 && cap < e->pf_grid) e->pf_grid = cap;
  }
  const long long tiles = (long long)nr * ((e->W + 255) / 256);
  void* args[] = {&bf};   // (BoxPre is BoxPreF32's first member: the exact kernel takes that much of it)
  (void)hipLaunchKernel(k.fn, dim3((unsigned)(tiles < e->pf_grid ? tiles : e->pf_grid)), dim3(256), args, BoxPreLds(nullptr, k.tables, nr).bytes, e->stream);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

// ---- device proposals (ptm_set_proposal_device) ---------------------------------------------------------------------------
// pack the chains that make a Metropolis move this step (touch flag 0) into the batch, name their rungs and walkers, call the user's
// function on the stream and put its proposals, ratios, types and validity where the sweep kernel reads them by chain (xprop: the
// buffer of the branch the sweep takes).  Everything is queued; nothing waits.
static int devprop_stage(ptm_engine* e, double* xprop) {
  const int n = e->Nc, D = e->D;
  const int nchunk = (n + DL_CHUNK - 1) / DL_CHUNK;
  const double* xcur = xrows(e);
  hipLaunchKernelGGL(devlike_count_kernel, dim3(nchunk), dim3(DL_CHUNK), 0, e->stream, n, (const unsigned char*)e->touch, 0xFF, 0, e->dp_chunks);
  HIPCHK(hipGetLastError());
  const unsigned ugrid = (unsigned)(((size_t)n * e->DP + DEVPROP_THREADS - 1) / DEVPROP_THREADS), rgrid = (unsigned)((n + DEVPROP_THREADS - 1) / DEVPROP_THREADS);
#define PTM_DP_PACK(N) case N: hipLaunchKernelGGL((devlike_pack_kernel<N>), dim3(nchunk), dim3(DL_CHUNK), 0, e->stream, n, D, nchunk, (const unsigned char*)e->touch, 0xFF, 0, \
                                                  (const int*)e->dp_chunks, xcur, xcur, e->dp_xcur, e->dp_rows, e->dp_count); break;
  switch (e->DP) {
    PTM_DP_PACK(4) PTM_DP_PACK(8) PTM_DP_PACK(16) PTM_DP_PACK(32) PTM_DP_PACK(64) PTM_DP_PACK(128) PTM_DP_PACK(256) PTM_DP_PACK(512) PTM_DP_PACK(1024)
    default: return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  }
#undef PTM_DP_PACK
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(devprop_ids_kernel, dim3(rgrid), dim3(DEVPROP_THREADS), 0, e->stream, n, e->W, e->r0, (int)e->cfg.walker_begin, (const int*)e->dp_rows,
                     e->dp_rung, e->dp_walker, e->dp_hast_k, e->dp_type_k, e->dp_valid_k);
  HIPCHK(hipGetLastError());
  e->dpfn(e->dp_user, (void*)e->stream, n, D, e->dp_xcur, e->dp_rung, e->dp_walker, e->dp_count, e->step, e->dp_xnew, e->dp_hast_k, e->dp_type_k, e->dp_valid_k);
#define PTM_DP_UNPACK(N) case N: hipLaunchKernelGGL((devprop_unpack_kernel<N>), dim3(ugrid), dim3(DEVPROP_THREADS), 0, e->stream, n, D, (const int32_t*)e->dp_count, \
                                                    (const int*)e->dp_rows, (const double*)e->dp_xnew, (const double*)e->dp_hast_k, (const int32_t*)e->dp_type_k, \
                                                    (const int32_t*)e->dp_valid_k, xprop, e->dp_hastings, e->dp_htype, e->dp_hvalid); break;
  switch (e->DP) {
    PTM_DP_UNPACK(4) PTM_DP_UNPACK(8) PTM_DP_UNPACK(16) PTM_DP_UNPACK(32) PTM_DP_UNPACK(64) PTM_DP_UNPACK(128) PTM_DP_UNPACK(256) PTM_DP_UNPACK(512) PTM_DP_UNPACK(1024)
    default: return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  }
#undef PTM_DP_UNPACK
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

static int launch_sweep(ptm_engine* e, int rung0 = 0, int nr = -1, bool last = true) {
  const bool labelled = e->label_step;   // (set by this step's exchange phase under the very conditions of the compacted sweep below)
  e->label_step = false;
  Dev p = make_dev(e, labelled);
  if (nr < 0) nr = e->nloc - rung0;
  if (rung0 < 0 || nr < 0 || rung0 + nr > e->nloc) return fail(PTM_ERR_INVALID, "rung range out of the shard");
  p.c_begin = rung0 * e->W; p.c_end = (rung0 + nr) * e->W;
  if ((user_like(e) || user_prop(e)) && (rung0 != 0 || nr != e->nloc)) return fail(PTM_ERR_UNSUPPORTED, "partial sweeps with a user likelihood (host or device) or host-side proposals are not built");
  { const int rc = devprior_ready(e); if (rc) return rc; }
  auto close_step = [&]() {
    e->step += 1; e->touched = false; e->step_booked = false;
    if (e->compact_step) { e->nhist_pending += 1; e->compact_step = false; }
  };
  if (nr == 0) { if (last) close_step(); return PTM_OK; }
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (e->cfg.time_kernels) {
    if (e->kev_used + 2 > e->kev.size()) {
      for (int k = 0; k < 2; ++k) { hipEvent_t ev; HIPCHK(hipEventCreate(&ev)); e->kev.push_back(ev); }
    }
    ev0 = e->kev[e->kev_used]; ev1 = e->kev[e->kev_used + 1];
    e->kev_used += 2;
  }
  const SweepPlan plan = sweep_plan(e, p.c_end - p.c_begin, e->touched);
  if (e->betaC_stale && !reads_ladder_major_beta(plan)) { int rc = ensure_betaC(e); if (rc) return rc; }   // (a build that reads the chain-indexed temperatures)
  // Compacted sweep: after an exchange phase ~1/6 of a long ladder's chains make no move; the lean MFMA build on a big
  // population then visits the moving chains only (partition_kernel packs them per rung).
  const bool compact = plan.compacted;
  if (labelled && !(compact && rung0 == 0 && nr == e->nloc)) return fail(PTM_ERR_HIP, "internal: a labelled exchange phase without its compacted sweep");
  if (!compact) { int rc = flush_nhist(e); if (rc) return rc; }
  if (compact) {
    if (!e->cidx) { int rc; if ((rc = dalloc(&e->cidx, (size_t)e->Nc)) || (rc = dalloc(&e->ccnt, (size_t)e->nloc))) return rc; }
    HIPCHK(hipMemsetAsync(e->ccnt + rung0, 0, (size_t)nr * sizeof(int), e->stream));
    // box pre-pass (ptm_box_prefilter.hpp): the flagged rungs' lists go to it first, and it hands their survivors on to the sweep
    bool pre = plan.prefilter;
    if (pre) {
      if (!e->pidx) {
        int rc;
        if ((rc = dalloc(&e->pidx, (size_t)e->Nc)) || (rc = dalloc(&e->pcnt, (size_t)e->nloc)) || (rc = dalloc(&e->pf_flag, (size_t)e->nloc)) || (rc = dalloc(&e->pf_counts, 2)) ||
            (rc = dalloc(&e->pf_margin, (size_t)e->nloc * PREFILTER_DIMS))) return rc;
        HIPCHK(hipMemsetAsync(e->pf_counts, 0, 16, e->stream));
        e->pf_dirty = true;
      }
      if (e->pf_dirty) { int rc = prefilter_flags(e); if (rc) return rc; }
      pre = e->pf_flagged > 0;
      if (pre) HIPCHK(hipMemsetAsync(e->pcnt + rung0, 0, (size_t)nr * sizeof(int), e->stream));
    }
    const int nchunk = (e->W + PART_CHUNK - 1) / PART_CHUNK;
    hipLaunchKernelGGL(partition_kernel, dim3((unsigned)((size_t)nr * nchunk)), dim3(1024), (size_t)PART_CHUNK * sizeof(int), e->stream, e->W, rung0, nchunk, e->touch, e->nhist,
                       e->cidx, e->ccnt, labelled ? (const unsigned short*)e->rowof : nullptr, pre ? (const unsigned char*)e->pf_flag : nullptr, e->pidx, e->pcnt);
    e->compact_step = true;   // (every partial sweep of this step goes the same way: the step is counted once, at its end)
    HIPCHK(hipGetLastError());
    if (pre) { int rc = launch_box_prefilter(e, p.x, rung0, nr, labelled); if (rc) return rc; }
    p.cidx = e->cidx; p.ccnt = e->ccnt; p.cidx_slot = labelled ? 1 : 0;
  }
  // the timed bracket holds the sweep kernel alone (its name: ptm_sweep_kernel_name): the list fill and partition_kernel of a
  // compacted sweep stay outside, so that the events' mean is what rocprofv3 reports for that kernel
  if (ev0) HIPCHK(hipEventRecord(ev0, e->stream));
  const AdaArgs ada = make_ada(e);
  const DpLaunch* dl = dp_launch(e->DP);
  if (!dl) return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  const bool de_mfma = de_mfma_sweep(e, p.c_end - p.c_begin);
  if (de_mfma && (compact || plan.family == FAM_MFMA32)) return fail(PTM_ERR_HIP, "internal: differential evolution on the matrix cores beside a matrix-core plan");
  auto launch = [&](const Dev& q) {
    if (de_mfma) return launch_de_mfma32(q, e->prop_kind == PTM_PROP_DENSE ? KIND_DENSE : KIND_LOWER, e->betaC != nullptr, e->stream);
    return dl->sweep(q, plan, e->stream, ada);
  };

  size_t npick = 0;
  if (e->pcb) {
    // host-side proposals: fetch the rows and the exchange phase's touch flags, let the host propose for every chain that
    // moves this step, hand the proposals (whole states), their log-Hastings ratios, types and validity to the kernel
    const size_t Nc = e->Nc, D = e->D, DP = e->DP;
    HIPCHK(hipMemcpyAsync(e->h_rows.data(), xrows(e), Nc * DP * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(e->h_touch.data(), e->touch, Nc, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->p_pick.clear();
    for (size_t c = 0; c < Nc; ++c)
      if (!e->h_touch[c]) e->p_pick.push_back(c);
    npick = e->p_pick.size();
    e->p_xcur.resize(npick * D); e->p_xprop.assign(npick * D, 0.0); e->p_hast.assign(npick, 0.0);
    e->p_rung.resize(npick); e->p_walker.resize(npick); e->p_type.assign(npick, 0); e->p_valid.assign(npick, 1);
    for (size_t k = 0; k < npick; ++k) {
      const size_t c = e->p_pick[k];
      for (size_t d = 0; d < D; ++d) e->p_xcur[k * D + d] = e->h_rows[c * DP + host_row_pos(DP, d)];
      e->p_rung[k] = e->r0 + (int)(c / e->W); e->p_walker[k] = e->cfg.walker_begin + (int)(c % e->W);   // GLOBAL rung and walker (ptm_engine.h)
    }
    if (npick)
      e->pcb(e->pcb_user, (int)npick, (int)D, e->p_xcur.data(), e->p_rung.data(), e->p_walker.data(), e->step, e->p_xprop.data(),
             e->p_hast.data(), e->p_type.data(), e->p_valid.data());
    // (rows of chains that make no move keep whatever the buffer held: the kernel never uses them)
    for (size_t k = 0; k < npick; ++k) {
      const size_t c = e->p_pick[k];
      for (size_t d = 0; d < DP; ++d) e->h_xprop[c * DP + d] = 0.0;
      for (size_t d = 0; d < D; ++d) e->h_xprop[c * DP + host_row_pos(DP, d)] = e->p_xprop[k * D + d];
      e->h_hast[c] = e->p_hast[k]; e->h_type[c] = e->p_type[k]; e->h_valid[c] = e->p_valid[k] ? 1 : 0;
    }
    HIPCHK(copy_unless_shared(e->xprop, e->h_xprop.data(), Nc * DP * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(copy_unless_shared(e->hastings, e->h_hast.data(), Nc * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(copy_unless_shared(e->htype, e->h_type.data(), Nc * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(copy_unless_shared(e->hvalid, e->h_valid.data(), Nc, hipMemcpyHostToDevice, e->stream));
    p.xprop = e->xprop; p.lprior_new = e->lprior_new; p.gate = e->gate; p.llike_new = e->llike_new;
  }
  if (e->dpfn) {
    // device proposals: the user's function fills the rows of the buffer the sweep (or its propose pass) reads its proposals from
    p.xprop = e->dfn ? e->dl_xprop : e->cb ? e->xprop : e->dp_xprop;
    p.hastings = e->dp_hastings; p.htype = e->dp_htype; p.hvalid = e->dp_hvalid; p.acc_out = e->dp_acc_out;
    const int rc = devprop_stage(e, p.xprop);
    if (rc) return rc;
  }
  if (e->dfn) {
    // device likelihood: propose pass -> pack -> the user's work -> scatter (+ best) -> accept pass, all queued on the stream
    p.xprop = e->dl_xprop; p.lprior_new = e->dl_lprior_new; p.gate = e->dl_gate; p.llike_new = e->dl_llike_new;
    p.mode = 1;
    HIPCHK(launch(p));
    // device prior: pack of the valid proposals -> the user's prior work -> prior gate, in front of the likelihood's pack
    if (e->dprior) { const int rc = devprior_stage(e); if (rc) return rc; }
    { const int rc = devlike_eval(e, e->dl_gate, 2, 2, e->dl_xprop, xrows(e), e->dl_llike_new, nullptr, e->dl_lprior_new, true); if (rc) return rc; }
    p.mode = 2;
    HIPCHK(launch(p));
  } else if (!e->cb) {
    HIPCHK(launch(p));
  } else {
    // host-callback likelihood: propose kernel -> user function on the gated proposals -> accept kernel
    const size_t Nc = e->Nc, DP = e->DP;
    p.xprop = e->xprop; p.lprior_new = e->lprior_new; p.gate = e->gate; p.llike_new = e->llike_new;
    p.mode = 1;
    HIPCHK(launch(p));   // (the propose pass writes every chain's gate byte: 0 for the rungs that make no move)
    { const int rc = callback_host_part(e); if (rc) return rc; }
    p.mode = 2;
    HIPCHK(launch(p));
  }
  if (e->pcb && e->pres && npick) {   // proposal_distribution::accept() / reject() (chain.cc:1009,1015)
    HIPCHK(copy_unless_shared(e->h_acc.data(), e->acc_out, (size_t)e->Nc, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->p_acc.resize(npick);
    for (size_t k = 0; k < npick; ++k) e->p_acc[k] = e->h_acc[e->p_pick[k]] == 1 ? 1 : 0;
    e->pres(e->pcb_user, (int)npick, e->p_rung.data(), e->p_walker.data(), e->p_acc.data());
  }
  if (e->dpfn && e->dpres) {   // the same for device proposals: the outcomes by row, then the user's function, queued behind the accept pass
    const int n = e->Nc;
    hipLaunchKernelGGL(devprop_result_kernel, dim3((unsigned)((n + DEVPROP_THREADS - 1) / DEVPROP_THREADS)), dim3(DEVPROP_THREADS), 0, e->stream, n,
                       (const int32_t*)e->dp_count, (const int*)e->dp_rows, (const unsigned char*)e->dp_acc_out, e->dp_acc_k);
    HIPCHK(hipGetLastError());
    e->dpres(e->dp_user, (void*)e->stream, n, e->dp_rung, e->dp_walker, e->dp_count, e->dp_acc_k);
  }
  if (ev1) HIPCHK(hipEventRecord(ev1, e->stream));
  if (last) close_step();
  return PTM_OK;
}

// adds the logged, not yet counted steps to the swap counters
static int fold_swap_log(ptm_engine* e) {
  if (!e->log_pending) return PTM_OK;
  const int first = ((e->log_head - e->log_pending) % PTM_LOG_RING + PTM_LOG_RING) % PTM_LOG_RING;
  if (e->Nt > 1) {
    hipLaunchKernelGGL(fold_swap_log_kernel, dim3(e->W), dim3(256), (size_t)2 * (e->Nt - 1) * sizeof(int), e->stream, e->swap_log, e->swap_cnt,
                       e->W, e->ms, e->Nt, e->r0, e->r0 + e->nloc, first, e->log_pending);
    HIPCHK(hipGetLastError());
  }
  e->log_pending = 0;
  return PTM_OK;
}

// chain-indexed image of the evolving ladders' temperatures, for the sweep kernels
static int launch_beta_transpose(ptm_engine* e) {
  e->betaC_stale = false;
  if (e->nloc != e->Nt) {   // a rung shard: its own rungs' temperatures out of the whole ladders'
    hipLaunchKernelGGL(beta_local_kernel, dim3((unsigned)(((size_t)e->Nc + 255) / 256)), dim3(256), 0, e->stream, e->beta_w, e->betaC, e->W, e->Nt, e->r0, e->nloc);
    HIPCHK(hipGetLastError());
    return PTM_OK;
  }
  hipLaunchKernelGGL(beta_transpose_kernel, dim3((e->Nt + 31) / 32, (e->W + 31) / 32), dim3(256), 0, e->stream, e->beta_w, e->betaC, e->W, e->Nt);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}
// the chain-indexed image, for everybody but the lean MFMA build of evolving ladders (which reads the ladder-major one)
static int ensure_betaC(ptm_engine* e) {
  if (!e->betaC_stale) return PTM_OK;
  e->betaC_stale = false;
  return launch_beta_transpose(e);
}

static Decide make_decide(ptm_engine* e, const double* ll_below, const double* ll_above, int H, double* send_up, double* send_down,
                          const double* ll_all = nullptr, const double* lp_all = nullptr, bool labels = false) {
  Decide p;
  memset(&p, 0, sizeof p);
  p.rowof = labels ? e->rowof : nullptr;
  p.ll_all = ll_all; p.lp_all = lp_all;
  p.shard_ends = e->shard_ends; p.nshards = e->nshards; p.halo_nominal = e->halo_nominal;
  p.redo_flag = e->redo_flag; p.redo_count = e->redo_flag ? e->redo_flag + e->W : nullptr;
  p.DP = e->DP; p.Nt = e->Nt; p.r0 = e->r0; p.nloc = e->nloc; p.W = e->W; p.Nc = e->Nc; p.ms = e->ms; p.w_off = e->cfg.walker_begin;
  p.seed = e->cfg.seed; p.step = e->step; p.thresh = e->thresh;
  p.beta = e->beta; p.ll_below = ll_below; p.ll_above = ll_above; p.H = ll_above ? H : 0; p.x = labels ? e->xdev : xrows(e); p.ll = e->ll; p.lp = e->lp;
  p.touch = e->touch; p.arr_below = e->arr_below; p.arr_above = e->arr_above;
  p.swap_log = e->swap_log + (size_t)e->log_head * e->W * e->ms; p.send_up = send_up; p.send_down = send_down; p.row_cap = e->row_cap; p.err = e->err;
  p.mv_src = e->mv_src; p.mv_dst = e->mv_dst; p.mv_n = e->mv_n;
  p.hist = e->hist; p.add_every_n = e->cfg.add_every_n; p.nhist = e->nhist;
  p.naccept = e->naccept; p.ntries = e->ntries; p.last_type = e->last_type;
  p.map = e->map;
  p.evolve_rate = e->evolve_rate; p.evolve_cut = e->evolve_cut; p.beta_w = e->beta_w; p.beta_add = e->beta_add;
  p.lp_is_const = e->lp_is_const ? 1 : 0; p.lp_const = e->lprior_const;
  // few ladders: the exchange kernel scatters the new temperatures into their chain-indexed image itself.  For populations the
  // scattered 8-byte stores cost the kernel what the transposition launch costs (measured at 1024 rungs x 16384 ladders: 0.621 ms
  // against 0.564 + 0.049; PTM_BETA_DIRECT=1 selects it anyway)
  static const bool direct_all = [] { const char* v = getenv("PTM_BETA_DIRECT"); return v && *v == '1'; }();
  const bool beta_direct = e->evolve_rate > 0 && (e->W <= 64 || direct_all);
  p.betaC_direct = beta_direct ? e->betaC : nullptr;
  return p;
}

static int launch_decide(ptm_engine* e, const double* ll_below, const double* ll_above, int H, double* send_up, double* send_down,
                         const double* ll_all = nullptr, const double* lp_all = nullptr, bool redo = false, bool labels = false) {
  // labels: a whole step of a whole-ladder engine whose sweep will be the compacted one (two_launch_steps) -- the kernel exchanges
  // row labels, and never looks at the rows
  if (labels && !e->rowof) {
    int rc = dalloc(&e->rowof, (size_t)e->Nc);
    if (rc) return rc;
    hipLaunchKernelGGL(identity_rows_kernel, dim3((unsigned)(((size_t)e->Nc + 255) / 256)), dim3(256), 0, e->stream, e->rowof, e->W, (size_t)e->Nc);
    HIPCHK(hipGetLastError());
  }
  Decide p = make_decide(e, ll_below, ll_above, H, send_up, send_down, ll_all, lp_all, labels);
  if (labels) { e->rows_labelled = true; e->label_step = true; }
  p.redo_only = redo ? 1 : 0;
  if (!redo && e->log_pending >= PTM_LOG_RING) { int rc = fold_swap_log(e); if (rc) return rc; }
  if (redo) {   // the second pass of the SAME step: the log slot, the messages and the move lists are the first pass's
    const int slot = (e->log_head + PTM_LOG_RING - 1) % PTM_LOG_RING;
    p.swap_log = e->swap_log + (size_t)slot * e->W * e->ms;
  }
  const bool beta_direct = p.betaC_direct != nullptr;
  e->touched = true;
  const int WN = ll_all ? e->Nt : e->nloc + (ll_below ? 1 : 0) + p.H;
  const bool evb = e->evolve_rate > 0 && e->beta_add;
  const bool cut = e->evolve_rate > 0 && e->evolve_cut >= 0;
  const size_t lds = DecideLds(nullptr, e->Nt, e->ms, WN, e->evolve_rate > 0, evb, cut).bytes;
  if (lds > 160 * 1024) return fail(PTM_ERR_UNSUPPORTED, "ladder too long for the LDS-resident exchange kernel (%zu B)", lds);
  if (e->ms >= 65535) return fail(PTM_ERR_UNSUPPORTED, "more than 65534 exchange candidates per step (the exchange kernel numbers them in 16 bits)");
  // expected candidates inside the window; evolving ladders with history / MAP tracking: the wide form alone carries the
  // saved rows' temperatures through its own row moves
  // ... and a few ladders only (latency regime) whose moves may overflow the 64-thread block: one launch instead of two
  const int per_pick = (e->nloc == e->Nt ? 2 : 4) + (e->hist.rungs ? 1 : 0) + (e->map.rungs ? 1 : 0);
  const bool wide = (double)e->ms * WN / e->Nt > 96.0 || evb || cut || (e->W <= 256 && per_pick * e->ms > 64);
  if (lds > 64 * 1024) {
    HIPCHK(hipFuncSetAttribute((const void*)decide_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipFuncSetAttribute((const void*)decide_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  // the boundary messages start empty (the row count lives in their first word)
  if (send_up && !redo) HIPCHK(hipMemsetAsync(send_up, 0, 16, e->stream));
  if (send_down && !redo) HIPCHK(hipMemsetAsync(send_down, 0, 16, e->stream));
  if (cut) {   // (always the wide form)
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)decide_kernel<256, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((decide_kernel<256, true>), dim3(e->W), dim3(256), lds, e->stream, p);
  } else if (wide) hipLaunchKernelGGL(decide_kernel<256>, dim3(e->W), dim3(256), lds, e->stream, p);
  else hipLaunchKernelGGL(decide_kernel<64>, dim3(e->W), dim3(64), lds, e->stream, p);
  HIPCHK(hipGetLastError());
  if (!redo) {   // (the ring is folded when the NEXT step finds it full: a second pass of this step still finds its slot pending)
    e->log_head = (e->log_head + 1) % PTM_LOG_RING;
    ++e->log_pending;
  }
  if (e->evolve_rate > 0 && !beta_direct) {
    if (lean_ev_sweeps(e)) e->betaC_stale = true;   // (nobody reads the chain-indexed image in such a step)
    else { e->betaC_stale = false; int rc = launch_beta_transpose(e); if (rc) return rc; }
  }
  if (wide) return PTM_OK;   // the 256-thread decide kernel has applied the moves itself
  // a pick lists at most four row moves (two rungs, each a local move and / or a departure) and one in-between row each for
  // the history and the MAP: short ladders
  // can never overflow the 64-thread block's own moves
  if (per_pick * e->ms <= 64 || labels) return PTM_OK;   // (labels: the block exchanged them itself whatever the list's length)
  Move m;
  m.DP = e->DP; m.W = e->W; m.row_cap = e->row_cap; m.x = xrows(e); m.ll = e->ll; m.lp = e->lp; m.send_up = send_up; m.send_down = send_down;
  m.mv_src = e->mv_src; m.mv_dst = e->mv_dst; m.mv_n = e->mv_n; m.err = e->err;
  m.hist = e->hist; m.add_every_n = e->cfg.add_every_n; m.nhist = e->nhist;
  m.naccept = e->naccept; m.ntries = e->ntries; m.last_type = e->last_type;
  m.map = e->map; m.beta = e->beta; m.r0 = e->r0;
  // (64-thread form only) ladders whose list did not fit the decide block's registers: rare, the kernel exits at once
  // for everybody else
  const dim3 mgrid((unsigned)((e->W + 63) / 64));   // (a wave scans the list lengths of 64 ladders)
  if (e->hist.rungs || e->map.rungs) hipLaunchKernelGGL((move_kernel<MVCAP, 1, true>), mgrid, dim3(64), 0, e->stream, m);
  else hipLaunchKernelGGL((move_kernel<MVCAP, 1, false>), mgrid, dim3(64), 0, e->stream, m);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

static int launch_install(ptm_engine* e, const double* recv_below, const double* recv_above) {
  if (!recv_below && !recv_above) return PTM_OK;
  Install q;
  q.DP = e->DP; q.W = e->W; q.row_cap = e->row_cap; q.x = xrows(e); q.ll = e->ll; q.lp = e->lp;
  q.recv_below = recv_below; q.recv_above = recv_above; q.arr_below = e->arr_below; q.arr_above = e->arr_above; q.err = e->err;
  e->touched = true;
  hipLaunchKernelGGL(install_kernel, dim3((e->row_cap + 15) / 16, 2), dim3(256), 0, e->stream, q);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}

static int ready(ptm_engine* e) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!e->have_target) return fail(PTM_ERR_INVALID, "no target set (ptm_set_target_gaussian)");
  if (!e->have_ladder) return fail(PTM_ERR_INVALID, "no ladder set (ptm_set_ladder)");
  if (!e->have_prop) return fail(PTM_ERR_INVALID, "no proposals set (ptm_set_proposals)");
  if (!e->have_state) return fail(PTM_ERR_INVALID, "no states set (ptm_set_states / ptm_init_from_prior)");
  { const int rc = devprior_ready(e); if (rc) return rc; }
  if (e->prior_member >= 0) return prior_drawable(e);   // (the prior may have changed since the member was named)
  return PTM_OK;
}

// ---- state ------------------------------------------------------------------------------------------------------
// all-uniform prior with every state inside the box: one lprior for all chains, and the sweeps keep it so (a move out of
// the box is never accepted) -- the exchange kernel then moves no lprior
static int check_lp_const(ptm_engine* e) {
  e->lp_is_const = false;
  if (!e->all_uniform || e->prior_cb || e->dprior) return PTM_OK;
  std::vector<double> lp((size_t)e->Nc);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(lp.data(), e->lp, lp.size() * 8, hipMemcpyDeviceToHost));
  for (double v : lp)
    if (!(v == e->lprior_const)) return PTM_OK;
  e->lp_is_const = true;
  return PTM_OK;
}
static int reset_counters(ptm_engine* e) {
  const size_t Nc = e->Nc;
  std::vector<int> one(Nc, 1), m1(Nc, -1);
  std::vector<unsigned int> z(Nc, 0u);
  int rc;
  if ((rc = upload(e->ntries, one.data(), Nc, e->stream)) || (rc = upload(e->naccept, one.data(), Nc, e->stream)) ||  // chain.cc:649
      (rc = upload(e->last_type, m1.data(), Nc, e->stream)) ||
      (rc = upload(e->nhist, z.data(), Nc, e->stream)))                                                        // chain.cc:871-875
    return rc;
  e->nhist_pending = 0; e->compact_step = false; e->touched = false;
  e->horizon.rebase(1); e->step_booked = false;
  HIPCHK(hipMemsetAsync(e->touch, 0, Nc, e->stream));
  HIPCHK(hipMemsetAsync(e->arr_below, 0xFF, (size_t)e->W * 4, e->stream));
  HIPCHK(hipMemsetAsync(e->arr_above, 0xFF, (size_t)e->W * 4, e->stream));
  e->step = 0;
  if (e->map.rungs) {    // MAP = the initial state (MH_chain::initialize -> add_state)
    if (!e->have_ladder) return fail(PTM_ERR_INVALID, "set the ladder before the states when tracking the MAP (ptm_set_ladder)");
    hipLaunchKernelGGL(map_init_kernel, dim3((e->map.MC + 255) / 256), dim3(256), 0, e->stream, e->map, e->DP, e->W, e->r0, e->beta, xrows(e), e->ll,
                       e->lp);
    HIPCHK(hipGetLastError());
  }
  if (e->hist.rungs) {   // history row 0 = the initial state (chain.cc:871-875)
    HIPCHK(hipMemsetAsync(e->hist.meta, 0xFF, (size_t)e->hist.cap * e->hist.HC * sizeof(int4), e->stream));
    if (e->hist.beta && !e->have_ladder) return fail(PTM_ERR_INVALID, "set the ladder before the states (ptm_set_ladder)");
    hipLaunchKernelGGL(hist_init_kernel, dim3((e->hist.HC + 255) / 256), dim3(256), 0, e->stream, e->hist, e->DP, xrows(e), e->ll, e->lp,
                       e->naccept, e->ntries, e->last_type, e->beta, e->betaC, e->W, e->r0);
    HIPCHK(hipGetLastError());
  }
  return PTM_OK;
}

// enforce == false: the states are taken as they are (ptm_restore: a saved state went through its one enforce when it was proposed, and
// the reference's two-sided reflection is not idempotent -- states.cc:31-45 folds to a NEGATIVE offset, so a second pass moves it)
static int run_eval(ptm_engine* e, int n, double* x, int* valid, double* lp, double* ll, int eval_like, bool enforce = true) {
  Dev p = make_dev(e);
  if (!enforce) p.has_bounds = 0;
  const DpLaunch* dl = dp_launch(e->DP);
  if (!dl) return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  HIPCHK(dl->eval(p, n, x, valid, lp, ll, eval_like, e->stream));
  return PTM_OK;
}

// host rows [n][D] -> device row image [n][DP]: padded, and for DP == 32 / 64 / 128 with dimension d at position row_pos(d)
// (ptm_kernels.hpp: the MFMA accumulator layout)
static inline size_t host_row_pos(size_t DP, size_t d) { return (DP == 32 || DP == 64 || DP == 128) ? 8 * ((d >> 2) >> 1) + 2 * (d & 3) + ((d >> 2) & 1) : d; }
static std::vector<double> pad_rows(const double* X, size_t n, size_t D, size_t DP) {
  std::vector<double> r(n * DP, 0.0);
  for (size_t c = 0; c < n; ++c)
    for (size_t d = 0; d < D; ++d) r[c * DP + host_row_pos(DP, d)] = X[c * D + d];
  return r;
}
static void unpad_rows(const double* r, size_t n, size_t D, size_t DP, double* X) {
  for (size_t c = 0; c < n; ++c)
    for (size_t d = 0; d < D; ++d) X[c * D + d] = r[c * DP + host_row_pos(DP, d)];
}
static void unpad_rows(const std::vector<double>& r, size_t n, size_t D, size_t DP, double* X) { unpad_rows(r.data(), n, D, DP, X); }

static int set_states(ptm_engine* e, const double* X, const double* llike, bool enforce);
extern "C" int ptm_set_states(ptm_engine* e, const double* X, const double* llike) {
  SETTLE(e);
  NO_BATCH(e, "ptm_set_states");
  return set_states(e, X, llike, true);
}
static int set_states(ptm_engine* e, const double* X, const double* llike, bool enforce) {
  if (!e || !X) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->have_target && !llike) return fail(PTM_ERR_INVALID, "set the target first (or pass llike)");
  { const int rc0 = devprior_ready(e); if (rc0) return rc0; }
  const size_t Nc = e->Nc, D = e->D, DP = e->DP;
  const std::vector<double> rows = pad_rows(X, Nc, D, DP);
  int rc;
  if ((rc = upload(xrows(e), rows.data(), Nc * DP, e->stream))) return rc;
  if (llike && (rc = upload(e->ll, llike, Nc, e->stream))) return rc;
  if ((rc = run_eval(e, (int)Nc, xrows(e), nullptr, e->lp, e->ll, (llike || user_like(e)) ? 0 : 1, enforce))) return rc;
  if (e->dfn) {
    // the device likelihood evaluates the (enforced) start states; the best posterior starts over with them
    if ((rc = devlike_reset_best(e))) return rc;
    if (e->dprior && (rc = devprior_of_states(e))) return rc;   // (first: the kept best starts from lprior + llike with the user's lprior)
    if (!llike && (rc = devlike_eval(e, nullptr, 0, 0, xrows(e), xrows(e), e->ll, nullptr, e->lp, true))) return rc;
  }
  if (e->cb && !llike) {
    // MH_chain::add_state(s) with the 999 sentinel: the likelihood plug-in evaluates the (enforced) start states (chain.cc:925)
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(e->h_xprop.data(), xrows(e), Nc * DP * 8, hipMemcpyDeviceToHost));
    std::vector<size_t> all(Nc);
    for (size_t c = 0; c < Nc; ++c) all[c] = c;
    if ((rc = call_user(e, e->h_xprop, all, e->h_llbatch))) return rc;
    if ((rc = upload(e->ll, e->h_llbatch.data(), Nc, e->stream))) return rc;
  }
  if (e->prior_cb) {
    if (!e->cb) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior needs the host-callback likelihood (ptm_set_target_callback)");
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(e->h_xprop.data(), xrows(e), Nc * DP * 8, hipMemcpyDeviceToHost));
    if ((rc = host_prior_of_states(e))) return rc;
  }
  if ((rc = reset_counters(e))) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  if ((rc = check_lp_const(e))) return rc;
  e->have_state = 1;
  return PTM_OK;
}

static int launch_init(ptm_engine* e, const Dev& p, long long attempt, unsigned char* pending, double* x = nullptr, double* ll = nullptr, double* lp = nullptr) {
  const DpLaunch* dl = dp_launch(e->DP);
  if (!dl) return fail(PTM_ERR_UNSUPPORTED, "dim > 1024 is not built");
  if (x) HIPCHK(dl->init(p, x, ll, lp, e->err + 1, attempt, pending, e->stream));   // (into a caller's staging arrays: ptm_draw_prior_rows)
  else HIPCHK(dl->init(p, xrows(e), e->ll, e->lp, e->err + 1, attempt, pending, e->stream));
  return PTM_OK;
}

extern "C" int ptm_init_from_prior(ptm_engine* e) { return ptm_init_from_prior_k(e, 0); }

extern "C" int ptm_init_from_prior_k(ptm_engine* e, int kdraw) {
  SETTLE(e);
  NO_BATCH(e, "ptm_init_from_prior");
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (kdraw < 0 || kdraw > 8191) return fail(PTM_ERR_INVALID, "initial draw index out of range (0..8191)");
  if (!e->have_target) return fail(PTM_ERR_INVALID, "set the target first");
  if (e->prior_cb) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior cannot be drawn from here: draw the start states with its drawSample and pass them to ptm_set_states");
  if (e->dprior) return fail(PTM_ERR_UNSUPPORTED, "a user prior on the device cannot be drawn from here: draw the start states with its drawSample and pass them to ptm_set_states");
  for (int d = 0; d < e->D; ++d)
    if (e->h_ptype[d] == PTM_PRIOR_FLAT)
      return fail(PTM_ERR_UNSUPPORTED, "a flat (improper) prior cannot be drawn from (dimension %d): pass start states", d);
  Dev p = make_dev(e);
  p.init_base = (uint64_t)kdraw << 17;   // attempts of draw k count from k * 2^17 (a draw gives up after 100000 < 2^17 attempts)
  HIPCHK(hipMemsetAsync(e->err + 1, 0, 4, e->stream));
  int rc;
  if (e->dfn && (rc = devlike_reset_best(e))) return rc;
  if (!user_like(e)) {
    if ((rc = launch_init(e, p, -1, nullptr))) return rc;
  } else if (e->dfn) {
    // the redraw loop with the device likelihood: one attempt per launch for the chains still pending (dl_gate), the device's
    // verdicts (dl_gate 0: draw again, 2: done), the pending count looked at once per attempt
    const size_t Nc = e->Nc;
    HIPCHK(hipMemsetAsync(e->dl_gate, 0, Nc, e->stream));
    std::vector<unsigned char> hg(Nc);
    size_t left = Nc;
    for (long long a = 0; left && a < 100000; ++a) {
      if ((rc = launch_init(e, p, a, e->dl_gate))) return rc;
      if ((rc = devlike_eval(e, e->dl_gate, 3, 1, xrows(e), nullptr, e->dl_llike_new, e->dl_gate, e->lp, true))) return rc;
      HIPCHK(hipMemcpyAsync(hg.data(), e->dl_gate, Nc, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      left = (size_t)std::count_if(hg.begin(), hg.end(), [](unsigned char g) { return g != 2; });
    }
    if (left) return fail(PTM_ERR_INVALID, "could not draw a valid start state from the prior for some chain");
    HIPCHK(hipMemcpyAsync(e->ll, e->dl_llike_new, Nc * 8, hipMemcpyDeviceToDevice, e->stream));
  } else {
    // MH_chain::initialize's redraw loop (chain.cc:856-869) with the plug-in likelihood on the host: one attempt per
    // launch for the chains still pending; `gate` doubles as the pending flag array
    const size_t Nc = e->Nc, DP = e->DP;
    HIPCHK(hipMemsetAsync(e->gate, 0, Nc, e->stream));
    std::vector<double> llh(Nc, 0.0);
    size_t left = Nc;
    for (long long a = 0; left && a < 100000; ++a) {
      if ((rc = launch_init(e, p, a, e->gate))) return rc;
      HIPCHK(copy_unless_shared(e->h_gate, e->gate, Nc, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->h_xprop.data(), xrows(e), Nc * DP * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      std::vector<size_t> pick;
      for (size_t c = 0; c < Nc; ++c)
        if (e->h_gate[c] == 1) pick.push_back(c);
      if ((rc = call_user(e, e->h_xprop, pick, e->h_llbatch))) return rc;
      for (size_t k = 0; k < pick.size(); ++k) {
        const double v = e->h_llbatch[k];
        if (v < -1e100) { e->h_gate[pick[k]] = 0; continue; }   // chain.cc:858: (slike=evaluate_log(s)) < -1e100 => redraw
        llh[pick[k]] = v;
        e->h_gate[pick[k]] = 2;
        left--;
      }
      HIPCHK(copy_unless_shared(e->gate, e->h_gate, Nc, hipMemcpyHostToDevice, e->stream));
    }
    if (left) return fail(PTM_ERR_INVALID, "could not draw a valid start state from the prior for some chain");
    if ((rc = upload(e->ll, llh.data(), Nc, e->stream))) return rc;
  }
  rc = reset_counters(e);
  if (rc) return rc;
  int flag = 0;
  HIPCHK(hipMemcpy(&flag, e->err + 1, 4, hipMemcpyDeviceToHost));
  if (flag) return fail(PTM_ERR_INVALID, "could not draw a valid start state from the prior for some chain");
  if ((rc = check_lp_const(e))) return rc;
  e->have_state = 1;
  return PTM_OK;
}

// Draws k_begin .. k_begin + n - 1 of every chain's initial draws (the rows ptm_init_from_prior_k(e, k) would leave in the engine) into
// host arrays, the engine's own state untouched: what MH_chain::initialize(n) saves in FRONT of the start state (chain.cc:846-876) in
// one call -- the sampler's default asks for 50 x dim of them, and one engine initialisation per row was most of a short run's time.
extern "C" int ptm_draw_prior_rows(ptm_engine* e, int k_begin, int n, double* x_out, double* ll_out, double* lp_out) {
  SETTLE(e);
  NO_BATCH(e, "ptm_draw_prior_rows");
  if (!e || (n > 0 && (!x_out || !ll_out || !lp_out))) return fail(PTM_ERR_INVALID, "null argument");
  if (n <= 0) return PTM_OK;
  if (k_begin < 0 || k_begin + n - 1 > 8191) return fail(PTM_ERR_INVALID, "initial draw index out of range (0..8191)");
  if (!e->have_target) return fail(PTM_ERR_INVALID, "set the target first");
  if (e->prior_cb) return fail(PTM_ERR_UNSUPPORTED, "a host-evaluated prior cannot be drawn from here: draw with its drawSample");
  if (e->dprior) return fail(PTM_ERR_UNSUPPORTED, "a user prior on the device cannot be drawn from here: draw with its drawSample");
  for (int d = 0; d < e->D; ++d)
    if (e->h_ptype[d] == PTM_PRIOR_FLAT)
      return fail(PTM_ERR_UNSUPPORTED, "a flat (improper) prior cannot be drawn from (dimension %d)", d);
  const size_t Nc = e->Nc, D = e->D, DP = e->DP;
  // staging on the device: G draws at a time (at most ~256 MB of rows)
  const size_t per = Nc * DP * 8;
  size_t G = per ? (size_t)(256u << 20) / per : 1;
  if (G < 1) G = 1;
  if (G > (size_t)n) G = (size_t)n;
  if (user_like(e)) G = 1;
  double *xs = nullptr, *ls = nullptr, *ps = nullptr;
  int rc = PTM_OK;
  if ((rc = dalloc(&xs, G * Nc * DP)) || (rc = dalloc(&ls, G * Nc)) || (rc = dalloc(&ps, G * Nc))) { hipFree(xs); hipFree(ls); hipFree(ps); return rc; }
  std::vector<double> hx(G * Nc * DP), hl(G * Nc), hp(G * Nc);
  auto done = [&](int r) { hipFree(xs); hipFree(ls); hipFree(ps); return r; };
#define PTM_DRAW_CHK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return done(fail(PTM_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_))); } while (0)
  PTM_DRAW_CHK(hipMemsetAsync(e->err + 1, 0, 4, e->stream));
  for (int k0 = 0; k0 < n; k0 += (int)G) {
    const int g = std::min((int)G, n - k0);
    for (int j = 0; j < g; ++j) {
      Dev p = make_dev(e);
      p.init_base = (uint64_t)(k_begin + k0 + j) << 17;
      double *xj = xs + (size_t)j * Nc * DP, *lj = ls + (size_t)j * Nc, *pj = ps + (size_t)j * Nc;
      if (!user_like(e)) {
        if ((rc = launch_init(e, p, -1, nullptr, xj, lj, pj))) return done(rc);
      } else if (e->dfn) {
        // the redraw loop of ptm_init_from_prior_k with the device likelihood, on the staging row
        PTM_DRAW_CHK(hipMemsetAsync(e->dl_gate, 0, Nc, e->stream));
        std::vector<unsigned char> hg(Nc);
        size_t left = Nc;
        for (long long a = 0; left && a < 100000; ++a) {
          if ((rc = launch_init(e, p, a, e->dl_gate, xj, lj, pj))) return done(rc);
          if ((rc = devlike_eval(e, e->dl_gate, 3, 1, xj, nullptr, e->dl_llike_new, e->dl_gate, pj, true))) return done(rc);
          PTM_DRAW_CHK(hipMemcpyAsync(hg.data(), e->dl_gate, Nc, hipMemcpyDeviceToHost, e->stream));
          PTM_DRAW_CHK(hipStreamSynchronize(e->stream));
          left = (size_t)std::count_if(hg.begin(), hg.end(), [](unsigned char g) { return g != 2; });
        }
        if (left) return done(fail(PTM_ERR_INVALID, "could not draw a valid state from the prior for some chain"));
        PTM_DRAW_CHK(hipMemcpyAsync(lj, e->dl_llike_new, Nc * 8, hipMemcpyDeviceToDevice, e->stream));
      } else {
        // the redraw loop of ptm_init_from_prior_k (chain.cc:856-869) on the staging row
        PTM_DRAW_CHK(hipMemsetAsync(e->gate, 0, Nc, e->stream));
        std::vector<double> llh(Nc, 0.0);
        size_t left = Nc;
        for (long long a = 0; left && a < 100000; ++a) {
          if ((rc = launch_init(e, p, a, e->gate, xj, lj, pj))) return done(rc);
          PTM_DRAW_CHK(copy_unless_shared(e->h_gate, e->gate, Nc, hipMemcpyDeviceToHost, e->stream));
          PTM_DRAW_CHK(hipMemcpyAsync(e->h_xprop.data(), xj, Nc * DP * 8, hipMemcpyDeviceToHost, e->stream));
          PTM_DRAW_CHK(hipStreamSynchronize(e->stream));
          std::vector<size_t> pick;
          for (size_t c = 0; c < Nc; ++c)
            if (e->h_gate[c] == 1) pick.push_back(c);
          if ((rc = call_user(e, e->h_xprop, pick, e->h_llbatch))) return done(rc);
          for (size_t q = 0; q < pick.size(); ++q) {
            const double v = e->h_llbatch[q];
            if (v < -1e100) { e->h_gate[pick[q]] = 0; continue; }
            llh[pick[q]] = v;
            e->h_gate[pick[q]] = 2;
            left--;
          }
          PTM_DRAW_CHK(copy_unless_shared(e->gate, e->h_gate, Nc, hipMemcpyHostToDevice, e->stream));
        }
        if (left) return done(fail(PTM_ERR_INVALID, "could not draw a valid state from the prior for some chain"));
        PTM_DRAW_CHK(hipMemcpyAsync(lj, llh.data(), Nc * 8, hipMemcpyHostToDevice, e->stream));
        PTM_DRAW_CHK(hipStreamSynchronize(e->stream));   // (llh is a local)
      }
    }
    PTM_DRAW_CHK(hipMemcpyAsync(hx.data(), xs, (size_t)g * Nc * DP * 8, hipMemcpyDeviceToHost, e->stream));
    PTM_DRAW_CHK(hipMemcpyAsync(hl.data(), ls, (size_t)g * Nc * 8, hipMemcpyDeviceToHost, e->stream));
    PTM_DRAW_CHK(hipMemcpyAsync(hp.data(), ps, (size_t)g * Nc * 8, hipMemcpyDeviceToHost, e->stream));
    PTM_DRAW_CHK(hipStreamSynchronize(e->stream));
    for (int j = 0; j < g; ++j) {
      const size_t o = (size_t)(k0 + j);
      for (size_t c = 0; c < Nc; ++c) {
        for (size_t d = 0; d < D; ++d) x_out[(o * Nc + c) * D + d] = hx[((size_t)j * Nc + c) * DP + host_row_pos(DP, d)];
        ll_out[o * Nc + c] = hl[(size_t)j * Nc + c];
        lp_out[o * Nc + c] = hp[(size_t)j * Nc + c];
      }
    }
  }
  int flag = 0;
  PTM_DRAW_CHK(hipMemcpy(&flag, e->err + 1, 4, hipMemcpyDeviceToHost));
#undef PTM_DRAW_CHK
  if (flag) return done(fail(PTM_ERR_INVALID, "could not draw a valid state from the prior for some chain"));
  return done(PTM_OK);
}

// ---- hot path ----------------------------------------------------------------------------------------------------
// The horizon (PTM_COUNT_MAX, ptm_count_limit.hpp): may this engine take n more PT steps?  One add and one compare while the host's
// bound allows it; when the bound trips, the two arrays are read once (queued and deferred work first, so they are the true counters),
// the bound is re-based to the true maximum and the question is asked again.  A refusal queues nothing and changes nothing.
static int count_guard(ptm_engine* e, long long n, const char* who) {
  if (e->horizon.admit(n)) return PTM_OK;
  int rc;
  if ((rc = ladder_settle(e)) || (rc = flush_nhist(e))) return rc;
  const size_t Nc = e->Nc;
  std::vector<int32_t> nt(Nc);
  std::vector<uint32_t> nh(Nc);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(nt.data(), e->ntries, Nc * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nh.data(), e->nhist, Nc * 4, hipMemcpyDeviceToHost));
  e->horizon.rebase(count_true_max(nt.data(), nh.data(), Nc));
  if (e->horizon.admit(n)) return PTM_OK;
  return fail(PTM_ERR_UNSUPPORTED, "%s: %lld more steps could take a chain's Ntries / Nhist (now %lld at the most) past PTM_COUNT_MAX = %lld, the largest count the engine "
              "represents; checkpoint, shift the counters down and restore (INTEGRATION.md, \"The horizon\")", who, n, (long long)e->horizon.bound, (long long)PTM_COUNT_MAX);
}
// the same for ONE step made in pieces: its first piece is the one that asks (close_step ends the step)
static int count_guard_piece(ptm_engine* e, const char* who) {
  if (e->step_booked) return PTM_OK;
  if (e->steps_prepaid > 0) e->steps_prepaid -= 1;
  else { const int rc = count_guard(e, 1, who); if (rc) return rc; }
  e->step_booked = true;
  return PTM_OK;
}

extern "C" int ptm_sweep(ptm_engine* e, int n) {
  SETTLE(e);
  NO_BATCH(e, "ptm_sweep");
  int rc = ready(e);
  if (rc) return rc;
  // (after an exchange phase of its own -- ptm_exchange_decide -- the first sweep belongs to the step that call was admitted for)
  if ((rc = count_guard(e, (long long)n - (e->step_booked && n > 0 ? 1 : 0), "ptm_sweep"))) return rc;
  for (int k = 0; k < n; ++k)
    if ((rc = launch_sweep(e))) return rc;
  return PTM_OK;
}

// Small ladders (rungs x padded dimensions <= the 1024 lanes of one workgroup, device target and proposals): whole PT steps in
// ONE launch per batch, a block per walker-ladder looping over the steps (ptm_fused_kernel.hpp).  PTM_FUSED=0 keeps the
// two-launch path.  Returns the steps taken (0: not this engine's case), or a negative status.
static size_t fused_decide_lds(const ptm_engine* e) { return DecideLds(nullptr, e->Nt, e->ms, e->Nt, e->evolve_rate > 0, e->evolve_rate > 0 && e->beta_add, false).bytes; }
static bool fused_applies(const ptm_engine* e) {
  static const bool fused_ok = [] { const char* v = getenv("PTM_FUSED"); return !(v && *v == '0'); }();
  StepFacts f;
  f.DP = e->DP; f.Nt = e->Nt; f.W = e->W;
  f.user_like = user_like(e); f.host_prop = user_prop(e); f.ada = e->ada_on || e->prior_member >= 0; f.time_kernels = e->cfg.time_kernels != 0;
  f.evolving = e->evolve_rate > 0; f.evolve_cut = e->evolve_cut >= 0;
  f.decide_lds = fused_decide_lds(e);
  return fused_applies(f, fused_ok);
}
static int fused_steps(ptm_engine* e, int n) {
  if (!fused_applies(e)) return 0;
  const size_t dlds = fused_decide_lds(e);
  int rc = flush_nhist(e);
  if (rc) return rc;
  if (e->log_pending >= PTM_LOG_RING && (rc = fold_swap_log(e))) return rc;
  int done = 0;
  while (done < n) {
    const int k = std::min(n - done, PTM_LOG_RING - e->log_pending);   // the candidate logs of at most a ring's worth of steps
    Dev p = make_dev(e);
    const Decide d = make_decide(e, nullptr, nullptr, 0, nullptr, nullptr);
    const bool diag = e->prop_kind == PTM_PROP_DIAG;
    HIPCHK(dp_launch(e->DP)->fused(p, d, diag, k, e->swap_log, e->log_head, dlds, e->stream));
    e->step += (uint64_t)k;
    e->log_head = (e->log_head + k) % PTM_LOG_RING;
    e->log_pending += k;
    if (e->log_pending >= PTM_LOG_RING && (rc = fold_swap_log(e))) return rc;
    done += k;
  }
  e->touched = false;
  return done;
}

// Long ladders of few walkers (the reference's own shape: one ladder of 1024 rungs): the steps of a ptm_step(n) call in ONE launch
// of resident workgroups that keep the chains in registers and talk to their neighbours through flags (ptm_ladder_kernel.hpp).
// Plain workload only; PTM_LADDER=0 keeps the two-launch path.  Returns the steps taken (0: not this engine's case), or a negative
// status.
// does a ptm_step call of this engine go through the persistent ladder kernel?  (grid: its workgroups; lds: their LDS)
#ifndef PTM_LADDER_MIN_STEPS
#define PTM_LADDER_MIN_STEPS 1
#endif
// the build of the persistent ladder kernel an engine takes: bit 0 one-dimensional moves / scale mixtures, bit 1 history / MAP tracking,
// bit 2 evolving ladders (built plain, 4, and with everything, 7)
static int ladder_flavour(const ptm_engine* e) {
  const int fl = ((e->any_oned || e->mix_K > 0) ? 1 : 0) | ((e->hist.rungs || e->map.rungs) ? 2 : 0);
  // any boundary (wrap, reflect) or a prior that is not all uniform: the builds with the general state space, which carry the recipe's and
  // the history's code whether or not this engine uses them (19, 23, 27, 31)
  if ((e->has_bounds && !e->bounds_box) || !e->all_uniform) return 16 | 3 | (e->evolve_rate > 0 ? 4 : 0) | (e->de_on ? 8 : 0);
  if (e->de_on) return e->evolve_rate > 0 ? 15 : 11;   // differential evolution: a member of a set, drawn from the history ring
  return e->evolve_rate > 0 ? (fl ? 7 : 4) : fl;
}
static bool ladder_applies(ptm_engine* e, long long* grid_out = nullptr, size_t* lds_out = nullptr) {
  static const bool ladder_ok = [] { const char* v = getenv("PTM_LADDER"); return !(v && *v == '0'); }();
  if (!ladder_ok || e->lad_disabled || e->DP > 32 || e->Nt < 2 || e->nloc != e->Nt || e->cfg.time_kernels || (e->evolve_rate > 0 && e->evolve_cut >= 0) || e->shard)
    return false;
  // open / `limit` boundaries, all-uniform prior, zero mean, fixed ladder, device target and proposals (one-dimensional moves, scale
  // mixtures, history and MAP tracking have their builds: ladder_flavour); ANY population whose grid is resident at once (below): where
  // it fits, a step costs this kernel its ~6 us of latency whatever the walkers' number (64 walkers x 64 rungs of 12 dimensions with the
  // sampler's defaults: 14 us against 40 on two launches)
  if (user_like(e) || e->prior_cb || user_prop(e)) return false;
  if (e->ada_on) return false;   // (an adaptive proposal set: exchange kernel + the lanes or general kernel's ADA build)
  if (e->prior_member >= 0) return false;   // (a member that draws from the prior: only the lanes and general kernels carry it)
  const int R = 256 / e->DP, NB = (e->Nt + R - 1) / R;
  const long long grid = (long long)e->W * NB;
  const bool diag = e->prop_kind == PTM_PROP_DIAG;
  const int fl = ladder_flavour(e);
  const bool ev_ = e->evolve_rate > 0;
  const DpLaunch* dl = dp_launch(e->DP);
  const size_t lds = dl->ladder_lds(e->Nt, e->ms, ev_);
  if (lds > 160 * 1024) return false;
  int& cap = e->lad_capacity[diag ? 1 : 0][fl];   // (asked per build: the builds differ in registers, and the LDS attribute is per kernel)
  if (cap < 0) cap = dl->ladder_blocks(diag, fl, lds);
  // every workgroup must be resident at once (they wait for each other)
  if (grid > cap || grid > 1024) return false;
  if (grid_out) *grid_out = grid;
  if (lds_out) *lds_out = lds;
  return true;
}
static int two_launch_steps(ptm_engine* e, int n);
// Have the launches of the persistent ladder kernel since the last look been committed?  If one gave up, the engine's arrays are as
// they were before it (the kernel commits all of a launch or nothing, and the launches behind it found its number missing and did
// nothing): its steps and theirs are repeated on the two-launch path, and this engine keeps that path from now on.
static int ladder_steps(ptm_engine* e, int n);
static int ladder_flush(ptm_engine* e) {
  if (!e->lad_deferred) return PTM_OK;
  int n = e->lad_deferred;
  e->lad_deferred = 0;
  const int f = ladder_steps(e, n);
  if (f < 0) return f;
  n -= f;
  if (n > 0) {   // (the kernel was switched off meanwhile: a launch gave up)
    HIPCHK(hipStreamSynchronize(e->stream));
    return two_launch_steps(e, n);
  }
  return PTM_OK;
}
static int ladder_settle(ptm_engine* e) {
  if (e->lad_deferred) { const int rc = ladder_flush(e); if (rc) return rc; }
  if (e->lad_log.empty()) return PTM_OK;
  HIPCHK(hipStreamSynchronize(e->stream));
  int w[3] = {0, 0, 0};
  HIPCHK(hipMemcpy(w, e->err, sizeof w, hipMemcpyDeviceToHost));
  if (w[2] == e->lad_seq) { e->lad_log.clear(); return PTM_OK; }
  size_t k = 0;
  while (k < e->lad_log.size() && e->lad_log[k].seq != w[2] + 1) ++k;
  if (k == e->lad_log.size()) return fail(PTM_ERR_HIP, "persistent ladder kernel: the device reports launch %d as the last one committed, the host has no record of its successor", w[2]);
  long long todo = 0;
  for (size_t j = k; j < e->lad_log.size(); ++j) todo += e->lad_log[j].nsteps;
  e->step = e->lad_log[k].step_before;
  e->log_head = e->lad_log[k].log_head_before;
  e->lad_log.clear();
  e->lad_disabled = true;
  e->ladder_fallbacks += 1;
  const int clr = w[0] & ~32;
  HIPCHK(hipMemcpy(e->err, &clr, 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->err + 2, &e->lad_seq, 4, hipMemcpyHostToDevice));
  static const bool quiet = [] { const char* v = getenv("PTM_QUIET"); return v && *v && *v != '0'; }();
  if (!quiet)
    fprintf(stderr, "[ptm] the persistent ladder kernel gave up waiting for a neighbouring workgroup (is the device shared?): nothing of that launch was "
                    "kept, its %lld steps are repeated on the two-launch path, which this engine keeps from now on\n", todo);
  while (todo > 0) {
    const int n = todo > (1 << 30) ? (1 << 30) : (int)todo;
    const int rc = two_launch_steps(e, n);
    if (rc) return rc;
    todo -= n;
  }
  return PTM_OK;
}
static int ladder_steps(ptm_engine* e, int n) {
  long long grid = 0;
  size_t lds = 0;
  // A launch of the persistent kernel stages its tables and loads its chains: a few microseconds on top of its steps
  // (tools/step1_probe.py).  A host loop that steps one at a time keeps the two-launch path.
  if (n < PTM_LADDER_MIN_STEPS) return 0;
  if (!ladder_applies(e, &grid, &lds)) return 0;
  const int R = 256 / e->DP, NB = (e->Nt + R - 1) / R;
  const bool diag = e->prop_kind == PTM_PROP_DIAG;
  const int fl = ladder_flavour(e);
  static const int max_run = [] { const char* v = getenv("PTM_LADDER_MAXRUN"); const int m = v && *v ? atoi(v) : LADDER_H; return m < 1 ? 1 : (m > LADDER_H ? LADDER_H : m); }();
  // how long a workgroup waits for a neighbour before it gives up: 3 s of the 100 MHz wall clock (a neighbour that is not there by
  // then never will be); PTM_LADDER_SPIN_US shortens it (tests: 0 makes every flag that is not up at the first look a reason to give up)
  static const long long spin_limit = [] { const char* v = getenv("PTM_LADDER_SPIN_US"); return v && *v ? atoll(v) * 100ll : 300000000ll; }();
  int rc = flush_nhist(e);
  if (rc) return rc;
  if (e->lad_log.size() >= 256 && (rc = ladder_settle(e))) return rc;   // (a host that never looks: look for it now and then)
  if (e->lad_disabled) return 0;
  const size_t Nc = e->Nc;
  if (!e->pub_x) {
    // what the workgroups publish for each other: fine-grained device memory where the runtime has it (a little faster across
    // XCDs: tools/probes/flag_pingpong_probe.hip), else ordinary -- the accesses are agent-scope atomics either way
    const size_t doubles = 2 * Nc * e->DP + 4 * Nc + 4 * Nc + 2;   // rows | llikes | lpriors | stamped llikes (16-byte aligned)
    void* buf = nullptr;
    if (hipExtMallocWithFlags(&buf, doubles * sizeof(double), hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      HIPCHK(hipMalloc(&buf, doubles * sizeof(double)));
    }
    e->pub_x = (double*)buf; e->pub_ll = e->pub_x + 2 * Nc * e->DP; e->pub_lp = e->pub_ll + 2 * Nc;
    HIPCHK(hipMemsetAsync(e->pub_lp + 2 * Nc, 0, (4 * Nc + 2) * sizeof(double), e->stream));   // (no stale word may look like a stamp)
    void* fl_ = nullptr;
    const size_t flbytes = ((size_t)grid + 16 + (size_t)e->W) * sizeof(int);
    if (hipExtMallocWithFlags(&fl_, flbytes, hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      HIPCHK(hipMalloc(&fl_, flbytes));
    }
    e->lad_flags = (int*)fl_; e->lad_ctl = e->lad_flags + grid;   // [grid] flags | [16] control words | [W] whole-ladder barrier counters
    HIPCHK(hipEventCreateWithFlags(&e->lad_event, hipEventDisableTiming));
  }
  static const bool prof_on = [] { const char* v = getenv("PTM_LADDER_PROF"); return v && *v && *v != '0'; }();
  if (prof_on && !e->lad_prof && (rc = dalloc(&e->lad_prof, (size_t)grid * 8))) return rc;
  int done = 0;
  while (done < n) {
    // (one launch walks at most 2^24 steps: its step-counted flags and LDS counters are ints, and a launch should end some day)
    const int k = n - done < (1 << 24) ? n - done : (1 << 24);
    Dev p = make_dev(e);
    LadderArgs a;
    a.nsteps = k; a.NB = NB; a.ms = e->ms; a.thresh = e->thresh;
    a.pub_x = e->pub_x; a.pub_ll = e->pub_ll; a.pub_lp = e->pub_lp; a.pub_s = e->pub_lp + 2 * (size_t)e->Nc + ((2 * (size_t)e->Nc * e->DP) & 1); a.flags = e->lad_flags; a.ctl = e->lad_ctl; a.slow_done = e->lad_ctl + 16;
    a.swap_cnt = e->swap_cnt; a.swap_log = e->swap_log + (size_t)e->log_head * e->W * e->ms;
    a.max_run = max_run;
    a.prof = e->lad_prof;
    { static const int pt = [] { const char* v = getenv("PTM_LADDER_PROF"); return (v && *v == '2') ? 256 : ((v && *v == '3') ? 384 : 0); }(); a.prof_tid = pt; }
    if ((rc = fold_swap_log(e))) return rc;   // (the kernel adds to the swap counters itself: nothing logged may be pending behind it)
    a.spin_limit = spin_limit;
    a.evolve_rate = e->evolve_rate;
    a.done_seq = e->err + 2;
    a.seq = e->lad_seq + 1;
    HIPCHK(hipMemsetAsync(e->lad_flags, 0, ((size_t)grid + 16 + (size_t)e->W) * sizeof(int), e->stream));
    {
      std::lock_guard<std::mutex> lock(g_lad_mutex);
      if (g_lad_last && g_lad_last != e && g_lad_last->lad_event) HIPCHK(hipStreamWaitEvent(e->stream, g_lad_last->lad_event, 0));
      HIPCHK(dp_launch(e->DP)->launch_ladder(p, a, diag, fl, (int)grid, lds, e->stream));
      // (the event costs a host call per launch: only a process with several engines on this path records it)
      static int engines_seen = 0;
      static ptm_engine* first_seen = nullptr;
      if (!first_seen) first_seen = e;
      if (first_seen != e) engines_seen = 2;
      if (engines_seen >= 2 || (g_lad_last && g_lad_last != e)) HIPCHK(hipEventRecord(e->lad_event, e->stream));
      g_lad_last = e;
    }
    e->ladder_launches++;
    e->lad_seq += 1;
    e->lad_log.push_back({e->lad_seq, e->step, k, e->log_head});
    if (e->lad_prof) {
      // diagnostics (PTM_LADDER_PROF): wait for the launch, read its outcome and its phase clocks -- mean microseconds per step and
      // phase over the workgroups, and the slowest workgroup's
      int ctl[4] = {0, 0, 0, 0};
      HIPCHK(hipMemcpyAsync(ctl, e->lad_ctl, sizeof ctl, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      if (ctl[1] > 0) {
        std::vector<long long> pr((size_t)grid * 8);
        HIPCHK(hipMemcpy(pr.data(), e->lad_prof, pr.size() * 8, hipMemcpyDeviceToHost));
        static const char* const phase[7] = {"", "publish", "draws | random blocks", "filter | offsets", "window | Metropolis", "commit + trials (evolving: decisions + pries)", "rows (evolving: temperatures, Metropolis, rows)"};
        fprintf(stderr, "[ladder kernel] %d steps, %lld workgroups; us per step (mean / max over workgroups):", ctl[1], grid);
        for (int q = 1; q < 7; ++q) {
          double sum = 0, mx = 0;
          for (long long g2 = 0; g2 < grid; ++g2) { const double v = pr[(size_t)g2 * 8 + q] * 0.01 / ctl[1]; sum += v; if (v > mx) mx = v; }
          fprintf(stderr, " %s %.2f/%.2f", phase[q], sum / grid, mx);
        }
        fprintf(stderr, "\n");
        e->ladder_whole_steps += ctl[2];
      }
    }
    e->step += (uint64_t)k;
    done += k;
    if (e->evolve_rate > 0) e->betaC_stale = true;    // (the kernel keeps the ladder-major temperatures; the chain-indexed image on demand: ensure_betaC)
    e->log_head = (e->log_head + 1) % PTM_LOG_RING;   // (the last step's candidate log sits in the slot handed over)
  }
  e->touched = false;
  return done;
}

static int two_launch_steps(ptm_engine* e, int n) {
  int rc;
  for (int k = 0; k < n; ++k) {
    if (e->Nt > 1 && (rc = launch_decide(e, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, false, row_labels_apply(e)))) return rc;
    if ((rc = launch_sweep(e))) return rc;
  }
  return PTM_OK;
}

extern "C" int ptm_step(ptm_engine* e, int n) {
  int rc = ready(e);
  if (rc) return rc;
  if (e->nloc != e->Nt) return fail(PTM_ERR_INVALID, "ptm_step needs the whole ladder on this engine; sharded engines use ptm_exchange_*");
  NO_BATCH(e, "ptm_step");
  if ((rc = count_guard(e, n, "ptm_step"))) return rc;
  if (n > 0) {
    int f = 0;
    // (the persistent ladder kernel first: where both apply it steps a small ladder in half the fused kernel's time -- 20 rungs of 6
    //  dimensions with the sampler's defaults: 11 against 22 us)
    if (ladder_applies(e)) {
      // small portions are counted and launched together later (lad_deferred); PTM_LADDER_DEFER=0: every call launches
      static const bool defer_ok = [] { const char* v = getenv("PTM_LADDER_DEFER"); return !(v && *v == '0'); }();
      if (defer_ok && n < 64) {
        e->lad_deferred += n;
        return e->lad_deferred >= 1024 ? ladder_flush(e) : PTM_OK;
      }
      if ((rc = ladder_flush(e))) return rc;
      f = ladder_steps(e, n);   // (launches of that kernel follow each other without a look at the outcome of the one before: ladder_settle)
      if (f < 0) return f;
      n -= f;
    }
    if (n > 0) {
      if ((rc = ladder_settle(e))) return rc;
      f = fused_steps(e, n);
      if (f < 0) return f;
      n -= f;
    }
  }
  if (n > 0 && (rc = ladder_settle(e))) return rc;
  return two_launch_steps(e, n);
}

extern "C" int ptm_sync(ptm_engine* e) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  { const int rc = ladder_settle(e); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->shard && e->shard->cstream) HIPCHK(hipStreamSynchronize(e->shard->cstream));   // (halos left in flight for the next step)
  int flag = 0;
  HIPCHK(hipMemcpy(&flag, e->err, 4, hipMemcpyDeviceToHost));
  if (flag & 1) return fail(PTM_ERR_FAR_MOVE, "a state crossed more than one shard boundary in one step (neighbour exchange mode)");
  if (flag & 2) return fail(PTM_ERR_FAR_MOVE, "an exchange chain reached past the llike halo: rerun with a deeper halo");
  if (flag & 4) return fail(PTM_ERR_FAR_MOVE, "a boundary message overflowed: more rows crossed a shard boundary in one step than "
                            "ptm_config.exchange_row_capacity slots (%d)", e->row_cap);
  if (flag & 8) return fail(PTM_ERR_FAR_MOVE, "a boundary message carried a row this shard did not expect (neighbour shards out of step?)");
  if (flag & 16) return fail(PTM_ERR_UNSUPPORTED, "a recorded rung's in-between history row belongs to the neighbour shard");
  if (flag & 64) return fail(PTM_ERR_INVALID, "differential evolution asked for a saved row the history ring no longer holds: history_capacity (%d rows) must hold the whole run", e->hist.cap);
  if (flag & 128) return fail(PTM_ERR_INVALID, "differential evolution: a thousand history states in a row equalled the current state (the reference exits here)");
  // (bit 32 -- a launch of the persistent ladder kernel gave up -- is not an error any more: ladder_settle has repeated its steps)
  return PTM_OK;
}

extern "C" int ptm_llike_device_ptr(ptm_engine* e, void** p) {
  SETTLE(e);
  if (!e || !p) return fail(PTM_ERR_INVALID, "null argument");
  *p = e->ll;
  return PTM_OK;
}

extern "C" int ptm_exchange_decide(ptm_engine* e, const void* ll_below, const void* ll_above, int halo_rungs, void* send_up,
                                   void* send_down) {
  SETTLE(e);
  NO_BATCH(e, "ptm_exchange_decide");
  NO_DEVLIKE(e, "ptm_exchange_decide");
  int rc = ready(e);
  if (rc) return rc;
  if (e->evolve_rate > 0 && e->nloc != e->Nt)
    return fail(PTM_ERR_INVALID, "an evolving ladder's shard decides from the whole ladder's llikes: ptm_exchange_decide_gathered");
  const bool first = e->r0 == 0, last = e->r0 + e->nloc == e->Nt;
  if ((!first && !ll_below) || (!last && (!ll_above || halo_rungs < 1)))
    return fail(PTM_ERR_INVALID, "missing llike halo: a shard needs the top rung below it and >= 1 rung above it");
  if (!last && halo_rungs > e->Nt - (e->r0 + e->nloc)) return fail(PTM_ERR_INVALID, "halo deeper than the ladder above this shard");
  if ((rc = count_guard_piece(e, "ptm_exchange_decide"))) return rc;
  if (e->Nt > 1)
    return launch_decide(e, first ? nullptr : (const double*)ll_below, last ? nullptr : (const double*)ll_above, halo_rungs,
                         last ? nullptr : (double*)send_up, first ? nullptr : (double*)send_down);
  return PTM_OK;
}

extern "C" int ptm_exchange_decide_gathered(ptm_engine* e, const void* ll_all, const void* lp_all, void* send_up, void* send_down) {
  SETTLE(e);
  NO_BATCH(e, "ptm_exchange_decide_gathered");
  NO_DEVLIKE(e, "ptm_exchange_decide_gathered");
  int rc = ready(e);
  if (rc) return rc;
  if (!ll_all) return fail(PTM_ERR_INVALID, "null argument");
  if (e->evolve_rate > 0 && e->evolve_cut >= 0 && !lp_all) return fail(PTM_ERR_INVALID, "a posterior-ordering cut needs the whole ladder's lpriors too");
  const bool first = e->r0 == 0, last = e->r0 + e->nloc == e->Nt;
  if ((!last && !send_up) || (!first && !send_down)) return fail(PTM_ERR_INVALID, "missing boundary message buffer");
  if ((rc = count_guard_piece(e, "ptm_exchange_decide_gathered"))) return rc;
  if (e->Nt > 1)
    return launch_decide(e, nullptr, nullptr, 0, last ? nullptr : (double*)send_up, first ? nullptr : (double*)send_down, (const double*)ll_all,
                         (const double*)lp_all);
  return PTM_OK;
}

extern "C" int ptm_set_shard_map(ptm_engine* e, int n_shards, const int32_t* rung_counts, int halo_rungs) {
  SETTLE(e);
  NO_BATCH(e, "ptm_set_shard_map");
  if (!e || !rung_counts || n_shards < 1 || halo_rungs < 1) return fail(PTM_ERR_INVALID, "bad argument");
  std::vector<int> ends(n_shards);
  int at = 0, mine = -1;
  for (int k = 0; k < n_shards; ++k) {
    if (rung_counts[k] < 1) return fail(PTM_ERR_INVALID, "every shard needs at least one rung");
    if (at == e->r0 && rung_counts[k] == e->nloc) mine = k;
    at += rung_counts[k];
    ends[k] = at;
  }
  if (at != e->Nt || mine < 0) return fail(PTM_ERR_INVALID, "the shard map does not describe this engine's block of the ladder");
  int rc;
  if (e->shard_ends) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->shard_ends)); e->shard_ends = nullptr; }
  if ((rc = dalloc(&e->shard_ends, (size_t)n_shards)) || (rc = upload(e->shard_ends, ends.data(), (size_t)n_shards, e->stream))) return rc;
  if (!e->redo_flag) {
    if ((rc = dalloc(&e->redo_flag, (size_t)e->W + 4))) return rc;
    HIPCHK(hipMemsetAsync(e->redo_flag, 0, ((size_t)e->W + 4) * sizeof(int), e->stream));
  }
  e->nshards = n_shards; e->halo_nominal = halo_rungs;
  return PTM_OK;
}

extern "C" int ptm_exchange_redo_count(ptm_engine* e, int* n) {
  SETTLE(e);
  if (!e || !n) return fail(PTM_ERR_INVALID, "null argument");
  *n = 0;
  if (!e->redo_flag) return PTM_OK;
  HIPCHK(hipMemcpyAsync(n, e->redo_flag + e->W, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

extern "C" int ptm_exchange_redo(ptm_engine* e, const void* ll_all, const void* lp_all, void* send_up, void* send_down) {
  SETTLE(e);
  NO_BATCH(e, "ptm_exchange_redo");
  NO_DEVLIKE(e, "ptm_exchange_redo");
  int rc = ready(e);
  if (rc) return rc;
  if (!e->redo_flag) return fail(PTM_ERR_INVALID, "ptm_set_shard_map first");
  if (!ll_all) return fail(PTM_ERR_INVALID, "null argument");
  int n = 0;
  if ((rc = ptm_exchange_redo_count(e, &n))) return rc;
  if (n == 0) return PTM_OK;
  e->redo_total += n;
  const bool first = e->r0 == 0, last = e->r0 + e->nloc == e->Nt;
  if ((!last && !send_up) || (!first && !send_down)) return fail(PTM_ERR_INVALID, "missing boundary message buffer");
  rc = launch_decide(e, nullptr, nullptr, 0, last ? nullptr : (double*)send_up, first ? nullptr : (double*)send_down, (const double*)ll_all, (const double*)lp_all, true);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(e->redo_flag + e->W, 0, sizeof(int), e->stream));
  return PTM_OK;
}

extern "C" int ptm_copy_lprior(ptm_engine* e, int first_local_rung, int n_rungs, void* dst_dev) {
  SETTLE(e);
  if (!e || !dst_dev) return fail(PTM_ERR_INVALID, "null argument");
  if (first_local_rung < 0 || n_rungs < 1 || first_local_rung + n_rungs > e->nloc) return fail(PTM_ERR_INVALID, "rung range out of the shard");
  HIPCHK(hipMemcpyAsync(dst_dev, e->lp + (size_t)first_local_rung * e->W, (size_t)n_rungs * e->W * 8, hipMemcpyDeviceToDevice, e->stream));
  return PTM_OK;
}

extern "C" int ptm_copy_llike(ptm_engine* e, int first_local_rung, int n_rungs, void* dst_dev) {
  SETTLE(e);
  if (!e || !dst_dev) return fail(PTM_ERR_INVALID, "null argument");
  if (first_local_rung < 0 || n_rungs < 1 || first_local_rung + n_rungs > e->nloc) return fail(PTM_ERR_INVALID, "rung range out of the shard");
  HIPCHK(hipMemcpyAsync(dst_dev, e->ll + (size_t)first_local_rung * e->W, (size_t)n_rungs * e->W * 8, hipMemcpyDeviceToDevice, e->stream));
  return PTM_OK;
}

// small device-memory helpers for callers without a GPU array library (tests, tools)
extern "C" int ptm_dev_alloc(size_t bytes, void** out) {
  int rc = need_device();
  if (rc) return rc;
  HIPCHK(hipMalloc(out, bytes ? bytes : 1));
  return PTM_OK;
}
extern "C" int ptm_dev_free(void* p) {
  if (p) HIPCHK(hipFree(p));
  return PTM_OK;
}
extern "C" int ptm_dev_copy(void* dst, const void* src, size_t bytes) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
  return PTM_OK;
}

extern "C" int ptm_exchange_install(ptm_engine* e, const void* recv_below, const void* recv_above) {
  SETTLE(e);
  NO_BATCH(e, "ptm_exchange_install");
  NO_DEVLIKE(e, "ptm_exchange_install");
  int rc = ready(e);
  if (rc) return rc;
  const bool first = e->r0 == 0, last = e->r0 + e->nloc == e->Nt;
  if ((!first && !recv_below) || (!last && !recv_above)) return fail(PTM_ERR_INVALID, "missing boundary message from a neighbour shard");
  if ((rc = count_guard_piece(e, "ptm_exchange_install"))) return rc;
  return launch_install(e, first ? nullptr : (const double*)recv_below, last ? nullptr : (const double*)recv_above);
}
extern "C" int ptm_sweep_rungs(ptm_engine* e, int first_local_rung, int n_rungs, int closes_step) {
  SETTLE(e);
  NO_BATCH(e, "ptm_sweep_rungs");
  NO_DEVLIKE(e, "ptm_sweep_rungs");
  int rc = ready(e);
  if (rc) return rc;
  if ((rc = count_guard_piece(e, "ptm_sweep_rungs"))) return rc;
  return launch_sweep(e, first_local_rung, n_rungs, closes_step != 0);
}

extern "C" int ptm_exchange_buffer_doubles(ptm_engine* e) { return e ? MSG_HDR + e->row_cap * (e->DP + ROW_EXTRA) : 0; }
extern "C" int ptm_exchange_row_capacity(ptm_engine* e) { return e ? e->row_cap : 0; }

extern "C" int ptm_exchange_finish_and_sweep(ptm_engine* e, const void* recv_below, const void* recv_above) {
  SETTLE(e);
  NO_BATCH(e, "ptm_exchange_finish_and_sweep");
  NO_DEVLIKE(e, "ptm_exchange_finish_and_sweep");
  if (e && e->dpfn && e->nloc != e->Nt) return fail(PTM_ERR_UNSUPPORTED, "ptm_exchange_finish_and_sweep on a rung shard with device proposals is not built (ptm_set_proposal_device)");
  int rc = ready(e);
  if (rc) return rc;
  const bool first = e->r0 == 0, last = e->r0 + e->nloc == e->Nt;
  if ((!first && !recv_below) || (!last && !recv_above)) return fail(PTM_ERR_INVALID, "missing boundary message from a neighbour shard");
  if ((rc = count_guard_piece(e, "ptm_exchange_finish_and_sweep"))) return rc;
  if ((rc = launch_install(e, first ? nullptr : (const double*)recv_below, last ? nullptr : (const double*)recv_above))) return rc;
  return launch_sweep(e);
}


// ---- native RCCL sharding -----------------------------------------------------------------------------------------------------
#define NCCLCHK(x)                                                                                                     \
  do {                                                                                                                 \
    ncclResult_t _r = (x);                                                                                             \
    if (_r != ncclSuccess) return fail(PTM_ERR_HIP, "%s failed: %s (%s:%d)", #x, rccl().GetErrorString(_r), __FILE__, __LINE__); \
  } while (0)

extern "C" int ptm_shard_unique_id(void* id_out) {
  if (!id_out) return fail(PTM_ERR_INVALID, "null argument");
  const char* why = rccl().load();
  if (why) return fail(PTM_ERR_UNSUPPORTED, "RCCL is not available: %s", why);
  static_assert(sizeof(ncclUniqueId) == PTM_SHARD_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  NCCLCHK(rccl().GetUniqueId(&id));
  memcpy(id_out, &id, sizeof id);
  return PTM_OK;
}

extern "C" int ptm_shard_finalize(ptm_engine* e) {
  if (!e || !e->shard) return PTM_OK;
  ShardComm* s = e->shard;
  (void)hipStreamSynchronize(e->stream);
  if (s->cstream) (void)hipStreamSynchronize(s->cstream);
  if (s->comm) (void)rccl().CommDestroy(s->comm);
  double* bufs[] = {s->ll_top, s->ll_bottom, s->ll_below, s->ll_above, s->send_up, s->recv_above, s->send_down, s->recv_below, s->gsend, s->grecv, s->ll_all, s->lp_all};
  if (s->ev_gather) (void)hipEventDestroy(s->ev_gather);
  for (double* b : bufs) if (b) (void)hipFree(b);
  if (s->ev_ready) (void)hipEventDestroy(s->ev_ready);
  if (s->ev_rows) (void)hipEventDestroy(s->ev_rows);
  if (s->ev_halo) (void)hipEventDestroy(s->ev_halo);
  if (s->cstream) (void)hipStreamDestroy(s->cstream);
  delete s;
  e->shard = nullptr;
  return PTM_OK;
}

extern "C" int ptm_shard_init(ptm_engine* e, const void* id, int rank, int world, const int32_t* rung_counts, int halo_rungs) {
  SETTLE(e);
  if (!e || !id || !rung_counts) return fail(PTM_ERR_INVALID, "null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(PTM_ERR_INVALID, "bad rank / world size");
  if (e->shard) return fail(PTM_ERR_INVALID, "this engine is sharded already (ptm_shard_finalize first)");
  int begin = 0, total = 0;
  for (int r = 0; r < world; ++r) { if (rung_counts[r] < 1) return fail(PTM_ERR_INVALID, "every rank needs at least one rung"); if (r < rank) begin += rung_counts[r]; total += rung_counts[r]; }
  if (total != e->Nt || begin != e->r0 || rung_counts[rank] != e->nloc)
    return fail(PTM_ERR_INVALID, "rung_counts do not describe this engine's block (rank %d: expected rungs %d..%d of %d, the engine holds %d..%d of %d)", rank, begin,
                begin + rung_counts[rank], total, e->r0, e->r0 + e->nloc, e->Nt);
  const char* why = rccl().load();
  if (why) return fail(PTM_ERR_UNSUPPORTED, "RCCL is not available: %s", why);
  ShardComm* s = new ShardComm();
  e->shard = s;
  s->rank = rank; s->world = world; s->halo = halo_rungs > 0 ? halo_rungs : 12;   // (ptmcmc_amd/parallel.py DEFAULT_HALO has the arithmetic)
  s->up = rank + 1 < world ? rank + 1 : -1;
  s->down = rank > 0 ? rank - 1 : -1;
  s->h_recv = s->up >= 0 ? (s->halo < rung_counts[rank + 1] ? s->halo : rung_counts[rank + 1]) : 0;   // what I receive from above is limited by the
  s->h_send = s->down >= 0 ? (s->halo < rung_counts[rank] ? s->halo : rung_counts[rank]) : 0;         // neighbour's size, what I send down by mine
  s->row_doubles = (size_t)ptm_exchange_buffer_doubles(e);
  HIPCHK(hipSetDevice(e->device));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  NCCLCHK(rccl().CommInitRank(&s->comm, world, uid, rank));
  HIPCHK(hipStreamCreateWithFlags(&s->cstream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&s->ev_ready, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&s->ev_rows, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&s->ev_halo, hipEventDisableTiming));
  const size_t W = (size_t)e->W;
  int rc;
  if (s->up >= 0 && ((rc = dalloc(&s->ll_top, W)) || (rc = dalloc(&s->ll_above, (size_t)s->h_recv * W)) || (rc = dalloc(&s->send_up, s->row_doubles)) ||
                     (rc = dalloc(&s->recv_above, s->row_doubles))))
    return rc;
  if (s->down >= 0 && ((rc = dalloc(&s->ll_bottom, (size_t)s->h_send * W)) || (rc = dalloc(&s->ll_below, W)) || (rc = dalloc(&s->send_down, s->row_doubles)) ||
                       (rc = dalloc(&s->recv_below, s->row_doubles))))
    return rc;
  s->counts.assign(rung_counts, rung_counts + world);
  for (int r = 0; r < world; ++r) s->maxn = rung_counts[r] > s->maxn ? rung_counts[r] : s->maxn;
  HIPCHK(hipEventCreateWithFlags(&s->ev_gather, hipEventDisableTiming));
  // a halo shallower than the default depth turns the recovery of longer runs on (PTM_SHARD_RECOVER=0/1 overrides; evolving
  // ladders gather every step anyway)
  const char* rv = getenv("PTM_SHARD_RECOVER");
  s->recover = world > 1 && e->evolve_rate <= 0 && (rv ? atoi(rv) != 0 : s->halo < 12);
  if (s->recover && (rc = ptm_set_shard_map(e, world, rung_counts, s->halo))) return rc;
  double* zero[] = {s->send_up, s->recv_above, s->send_down, s->recv_below};
  for (double* b : zero) if (b) HIPCHK(hipMemsetAsync(b, 0, s->row_doubles * 8, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

// One message round on the side stream: it starts when the engine's stream has reached `after`, and `done` marks its end.
// up_* / down_*: what goes to / comes from the upper / lower neighbour (counts in doubles).
static int shard_exchange(ptm_engine* e, const double* up_send, size_t up_ns, double* up_recv, size_t up_nr, const double* down_send, size_t down_ns,
                          double* down_recv, size_t down_nr, hipEvent_t done) {
  ShardComm* s = e->shard;
  HIPCHK(hipEventRecord(s->ev_ready, e->stream));
  HIPCHK(hipStreamWaitEvent(s->cstream, s->ev_ready, 0));
  NCCLCHK(rccl().GroupStart());
  if (s->up >= 0) {
    NCCLCHK(rccl().Send(up_send, up_ns, ncclDouble, s->up, s->comm, s->cstream));
    NCCLCHK(rccl().Recv(up_recv, up_nr, ncclDouble, s->up, s->comm, s->cstream));
  }
  if (s->down >= 0) {
    NCCLCHK(rccl().Send(down_send, down_ns, ncclDouble, s->down, s->comm, s->cstream));
    NCCLCHK(rccl().Recv(down_recv, down_nr, ncclDouble, s->down, s->comm, s->cstream));
  }
  NCCLCHK(rccl().GroupEnd());
  HIPCHK(hipEventRecord(done, s->cstream));
  return PTM_OK;
}
static int shard_stage_and_start_halos(ptm_engine* e) {
  ShardComm* s = e->shard;
  int rc;
  if (s->up >= 0 && (rc = ptm_copy_llike(e, e->nloc - 1, 1, s->ll_top))) return rc;
  if (s->down >= 0 && (rc = ptm_copy_llike(e, 0, s->h_send, s->ll_bottom))) return rc;
  const size_t W = (size_t)e->W;
  if ((rc = shard_exchange(e, s->ll_top, W, s->ll_above, (size_t)s->h_recv * W, s->ll_bottom, (size_t)s->h_send * W, s->ll_below, W, s->ev_halo))) return rc;
  s->halos_in_flight = true;
  return PTM_OK;
}

// the whole ladder's llikes and lpriors on every shard: one ncclAllGather of the shards' (padded) slabs, unpacked in rung order
// into ll_all / lp_all [Nt][W] on the engine's stream
static int shard_gather_ladder(ptm_engine* e) {
  ShardComm* s = e->shard;
  int rc;
  const size_t W = (size_t)e->W, slab = (size_t)s->maxn * W;
  if (!s->gsend && ((rc = dalloc(&s->gsend, 2 * slab)) || (rc = dalloc(&s->grecv, (size_t)s->world * 2 * slab)) || (rc = dalloc(&s->ll_all, (size_t)e->Nt * W)) ||
                    (rc = dalloc(&s->lp_all, (size_t)e->Nt * W))))
    return rc;
  if ((rc = ptm_copy_llike(e, 0, e->nloc, s->gsend)) || (rc = ptm_copy_lprior(e, 0, e->nloc, s->gsend + slab))) return rc;
  HIPCHK(hipEventRecord(s->ev_ready, e->stream));
  HIPCHK(hipStreamWaitEvent(s->cstream, s->ev_ready, 0));
  NCCLCHK(rccl().AllGather(s->gsend, s->grecv, 2 * slab, ncclDouble, s->comm, s->cstream));
  HIPCHK(hipEventRecord(s->ev_gather, s->cstream));
  HIPCHK(hipStreamWaitEvent(e->stream, s->ev_gather, 0));
  size_t at = 0;
  for (int r = 0; r < s->world; ++r) {   // the shards' slabs, unpadded, in rung order
    const size_t cnt = (size_t)s->counts[r] * W;
    HIPCHK(hipMemcpyAsync(s->ll_all + at, s->grecv + (size_t)r * 2 * slab, cnt * 8, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(s->lp_all + at, s->grecv + (size_t)r * 2 * slab + slab, cnt * 8, hipMemcpyDeviceToDevice, e->stream));
    at += cnt;
  }
  return PTM_OK;
}

// Runs of surviving picks longer than the halo (ptm_set_shard_map): every shard left the same ladders alone; if there are any
// (one wait on the stream per step to know), the ladder is gathered and they are decided from the full view.
static int shard_recover(ptm_engine* e) {
  ShardComm* s = e->shard;
  if (!s->recover) return PTM_OK;
  int rc, pending = 0;
  if ((rc = ptm_exchange_redo_count(e, &pending)) || !pending) return rc;
  if ((rc = shard_gather_ladder(e))) return rc;
  return ptm_exchange_redo(e, s->ll_all, s->lp_all, s->send_up, s->send_down);
}

static int shard_steps(ptm_engine* e, int n);
extern "C" int ptm_shard_step(ptm_engine* e, int n) {
  SETTLE(e);
  NO_BATCH(e, "ptm_shard_step");
  int rc = ready(e);
  if (rc) return rc;
  if (!e->shard) return fail(PTM_ERR_INVALID, "ptm_shard_init first");
  if (user_like(e) || user_prop(e)) return fail(PTM_ERR_UNSUPPORTED, "sharded steps with a user likelihood (host or device) or host-side proposals are not built");
  // all n steps are admitted here, before anything is queued; their pieces go through the public calls, which then do not ask again
  if ((rc = count_guard(e, n, "ptm_shard_step"))) return rc;
  e->steps_prepaid = n > 0 ? n : 0;
  rc = shard_steps(e, n);
  e->steps_prepaid = 0;
  return rc;
}
static int shard_steps(ptm_engine* e, int n) {
  int rc;
  ShardComm* s = e->shard;
  if (e->evolve_rate > 0) {
    // Evolving ladders: every shard replays the whole ladder's trials from the whole ladder's llikes (and lpriors, with a
    // posterior-ordering cut) -- one ncclAllGather per step, the reference's gather_llikes / gather_lposts (chain.cc:1433-1435,
    // 1950-1972) -- then the boundary rows travel between neighbours as ever.  No overlap: the trials need the gathered view.
    for (int k = 0; k < n; ++k) {
      if ((rc = shard_gather_ladder(e))) return rc;
      if ((rc = ptm_exchange_decide_gathered(e, s->ll_all, s->lp_all, s->send_up, s->send_down))) return rc;
      if ((rc = shard_exchange(e, s->send_up, s->row_doubles, s->recv_above, s->row_doubles, s->send_down, s->row_doubles, s->recv_below, s->row_doubles, s->ev_rows))) return rc;
      HIPCHK(hipStreamWaitEvent(e->stream, s->ev_rows, 0));
      if ((rc = ptm_exchange_finish_and_sweep(e, s->recv_below, s->recv_above))) return rc;
    }
    return PTM_OK;
  }
  const bool overlap = !e->hist.rungs && !e->map.rungs;   // (a recorded exchanged rung reads its final row: needs the arrivals first)
  // sweep plan: the boundary rungs are the ones whose llikes the neighbours need as halos (bottom h_send rungs, the top rung)
  const int nl = e->nloc, nb = s->h_send < nl ? s->h_send : nl, nt = (s->up >= 0 && nl > nb) ? 1 : 0;
  const int lo = nb, hi = nl - nt, mid = lo + (hi - lo) / 2;
  for (int k = 0; k < n; ++k) {
    if (!s->halos_in_flight && (rc = shard_stage_and_start_halos(e))) return rc;
    HIPCHK(hipStreamWaitEvent(e->stream, s->ev_halo, 0));
    s->halos_in_flight = false;
    if ((rc = ptm_exchange_decide(e, s->ll_below, s->ll_above, s->h_recv, s->send_up, s->send_down))) return rc;
    if ((rc = shard_recover(e))) return rc;
    if ((rc = shard_exchange(e, s->send_up, s->row_doubles, s->recv_above, s->row_doubles, s->send_down, s->row_doubles, s->recv_below, s->row_doubles, s->ev_rows))) return rc;
    if (!overlap) {
      HIPCHK(hipStreamWaitEvent(e->stream, s->ev_rows, 0));
      if ((rc = ptm_exchange_finish_and_sweep(e, s->recv_below, s->recv_above))) return rc;
      continue;
    }
    if ((rc = ptm_sweep_rungs(e, lo, mid - lo, 0))) return rc;            // ... while the boundary rows travel
    HIPCHK(hipStreamWaitEvent(e->stream, s->ev_rows, 0));
    if ((rc = ptm_exchange_install(e, s->recv_below, s->recv_above))) return rc;
    if ((rc = ptm_sweep_rungs(e, 0, nb, 0))) return rc;
    if ((rc = ptm_sweep_rungs(e, nl - nt, nt, 0))) return rc;
    if ((rc = shard_stage_and_start_halos(e))) return rc;                 // the NEXT step's halos ...
    if ((rc = ptm_sweep_rungs(e, mid, hi - mid, 1))) return rc;           // ... travel behind the second half of the interior
  }
  return PTM_OK;
}

// ---- read-back ------------------------------------------------------------------------------------------------------
extern "C" int ptm_get_states(ptm_engine* e, double* X) {
  SETTLE(e);
  if (!e || !X) return fail(PTM_ERR_INVALID, "null argument");
  const size_t Nc = e->Nc, D = e->D, DP = e->DP;
  const unsigned char* s;
  FETCH(s, xrows(e), Nc * DP * 8);
  e->fetch_after.push_back([=] { unpad_rows((const double*)s, Nc, D, DP, X); });
  return fetch_done(e);
}

extern "C" int ptm_get_array(ptm_engine* e, int which, void* out) {
  SETTLE(e);
  if (!e || !out) return fail(PTM_ERR_INVALID, "null argument");
  const size_t Nc = e->Nc;
  const unsigned char* s;
  switch (which) {
    case PTM_ARR_LLIKE: FETCH(s, e->ll, Nc * 8); e->fetch_after.push_back([=] { memcpy(out, s, Nc * 8); }); break;
    case PTM_ARR_LPRIOR: FETCH(s, e->lp, Nc * 8); e->fetch_after.push_back([=] { memcpy(out, s, Nc * 8); }); break;
    case PTM_ARR_LPOST: {
      if (!e->have_ladder) return fail(PTM_ERR_INVALID, "no ladder set");
      const unsigned char *sl, *sp, *sb = nullptr;
      FETCH(sl, e->ll, Nc * 8);
      FETCH(sp, e->lp, Nc * 8);
      { int rc2 = ensure_betaC(e); if (rc2) return rc2; }
      if (e->betaC) FETCH(sb, e->betaC, Nc * 8);
      e->fetch_after.push_back([=] {
        const double *ll = (const double*)sl, *lp = (const double*)sp, *bc = (const double*)sb;
        double* o = (double*)out;
        for (size_t c = 0; c < Nc; ++c) {
          volatile double t = (bc ? bc[c] : e->h_beta[e->r0 + c / e->W]) * ll[c];  // product rounded before the sum (chain.cc:928)
          o[c] = lp[c] + t;
        }
      });
      break;
    }
    case PTM_ARR_NTRIES: FETCH(s, e->ntries, Nc * 4); e->fetch_after.push_back([=] { memcpy(out, s, Nc * 4); }); break;
    case PTM_ARR_NACCEPT: FETCH(s, e->naccept, Nc * 4); e->fetch_after.push_back([=] { memcpy(out, s, Nc * 4); }); break;
    case PTM_ARR_LAST_TYPE: FETCH(s, e->last_type, Nc * 4); e->fetch_after.push_back([=] { memcpy(out, s, Nc * 4); }); break;
    case PTM_ARR_NHIST:
    case PTM_ARR_NSIZE: {
      { int rc = flush_nhist(e); if (rc) return rc; }
      FETCH(s, e->nhist, Nc * 4);
      const int64_t N = e->cfg.add_every_n;
      // add k (k = 0,1,..) appends a row iff k % N == 0 (chain.cc:935-946); one row exists after initialize(1)
      e->fetch_after.push_back([=] {
        const unsigned int* h = (const unsigned int*)s;
        int64_t* o = (int64_t*)out;
        for (size_t c = 0; c < Nc; ++c) o[c] = which == PTM_ARR_NHIST ? (int64_t)h[c] : 1 + ((int64_t)h[c] + N - 1) / N;
      });
      break;
    }
    case PTM_ARR_ROW_LABELS: {   // as they stand: this call puts no row back
      if (!e->rowof) {
        const int W = e->W;
        e->fetch_after.push_back([=] { for (size_t c = 0; c < Nc; ++c) ((int32_t*)out)[c] = (int32_t)(c / (size_t)W); });
        break;
      }
      FETCH(s, e->rowof, Nc * 2);
      e->fetch_after.push_back([=] { for (size_t c = 0; c < Nc; ++c) ((int32_t*)out)[c] = ((const unsigned short*)s)[c]; });
      break;
    }
    default: return fail(PTM_ERR_INVALID, "unknown array id %d", which);
  }
  return fetch_done(e);
}

extern "C" int ptm_get_swap_counts(ptm_engine* e, int64_t* tries, int64_t* accepts) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  const size_t np = (size_t)e->W * (e->Nt > 1 ? e->Nt - 1 : 1);
  { int rc = fold_swap_log(e); if (rc) return rc; }
  const unsigned char* s;
  FETCH(s, e->swap_cnt, 2 * np * 8);
  e->fetch_after.push_back([=] {
    const long long* both = (const long long*)s;
    for (size_t i = 0; i < np; ++i) {
      if (tries) tries[i] = both[2 * i];
      if (accepts) accepts[i] = both[2 * i + 1];
    }
  });
  return fetch_done(e);
}

extern "C" int ptm_get_last_swaps(ptm_engine* e, int32_t* pairs, int32_t* accepted) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  const size_t n = (size_t)e->W * e->ms;
  const int newest = (e->log_head + PTM_LOG_RING - 1) % PTM_LOG_RING;
  const unsigned char* s;
  FETCH(s, e->swap_log + (size_t)newest * n, n * 4);
  e->fetch_after.push_back([=] {
    const int32_t* log = (const int32_t*)s;
    for (size_t i = 0; i < n; ++i) {
      const int32_t v = log[i];
      if (pairs) pairs[i] = v < 0 ? (v == -3 ? -3 : -2) : (v & 0x3fffffff);
      if (accepted) accepted[i] = (v >= 0 && (v & 0x40000000)) ? 1 : 0;
    }
  });
  return fetch_done(e);
}

extern "C" int ptm_get_map(ptm_engine* e, double* X, double* lpost, double* llike, double* lprior) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!e->map.rungs) return fail(PTM_ERR_INVALID, "MAP tracking is off (ptm_config.map_rungs)");
  const size_t n = (size_t)e->map.MC, D = e->D, DP = e->DP;
  const unsigned char* s;
  if (X) { FETCH(s, e->map.x, n * DP * 8); e->fetch_after.push_back([=] { unpad_rows((const double*)s, n, D, DP, X); }); }
  if (lpost) { FETCH(s, e->map.lpost, n * 8); e->fetch_after.push_back([=] { memcpy(lpost, s, n * 8); }); }
  if (llike) { FETCH(s, e->map.ll, n * 8); e->fetch_after.push_back([=] { memcpy(llike, s, n * 8); }); }
  if (lprior) { FETCH(s, e->map.lp, n * 8); e->fetch_after.push_back([=] { memcpy(lprior, s, n * 8); }); }
  return fetch_done(e);
}

extern "C" int ptm_restore(ptm_engine* e, const double* X, const double* llike, const int32_t* ntries, const int32_t* naccept,
                           const int32_t* last_type, const int64_t* nhist, uint64_t step_count, const int64_t* swap_tries,
                           const int64_t* swap_accepts) {
  SETTLE(e);
  NO_BATCH(e, "ptm_restore");
  if (!e || !X || !llike || !ntries || !naccept || !last_type || !nhist) return fail(PTM_ERR_INVALID, "null argument");
  // the counters first, before anything is touched: inside the horizon (PTM_COUNT_MAX), and no more accepts than tries
  const size_t Nc = e->Nc;
  std::vector<unsigned int> nh(Nc);
  for (size_t c = 0; c < Nc; ++c) {
    const char* why = count_restore_error(ntries[c], naccept[c], nhist[c]);
    if (why) return fail(PTM_ERR_INVALID, "%s out of range (chain %zu: ntries %d, naccept %d, nhist %lld): every counter lies in [0, PTM_COUNT_MAX = %lld] and naccept <= ntries",
                         why, c, (int)ntries[c], (int)naccept[c], (long long)nhist[c], (long long)PTM_COUNT_MAX);
    nh[c] = (unsigned int)nhist[c];
  }
  // (a history ring / MAP restart from the restored state here; ptm_set_history / ptm_set_map put saved ones back)
  int rc = set_states(e, X, llike, false);   // the states as they were saved (no second enforce), their lpriors recomputed, the counters reset
  if (rc) return rc;
  if ((rc = upload(e->ntries, ntries, Nc, e->stream)) || (rc = upload(e->naccept, naccept, Nc, e->stream)) ||
      (rc = upload(e->last_type, last_type, Nc, e->stream)) || (rc = upload(e->nhist, nh.data(), Nc, e->stream)))
    return rc;
  const size_t np = (size_t)e->W * (e->Nt > 1 ? e->Nt - 1 : 1);
  {
    std::vector<long long> both(2 * np, 0);
    for (size_t i = 0; i < np; ++i) {
      if (swap_tries) both[2 * i] = swap_tries[i];
      if (swap_accepts) both[2 * i + 1] = swap_accepts[i];
    }
    e->log_pending = 0;   // (the counters are replaced: steps logged before belong to the run that is left)
    if ((rc = upload(e->swap_cnt, both.data(), 2 * np, e->stream))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));   // `both` leaves scope
  }
  e->step = step_count;
  e->horizon.rebase(count_true_max(ntries, nh.data(), Nc));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

extern "C" int ptm_set_map(ptm_engine* e, const double* X, const double* lpost, const double* llike, const double* lprior) {
  SETTLE(e);
  NO_BATCH(e, "ptm_set_map");
  if (!e || !X || !lpost || !llike || !lprior) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->map.rungs) return fail(PTM_ERR_INVALID, "MAP tracking is off (ptm_config.map_rungs)");
  const size_t n = (size_t)e->map.MC;
  const std::vector<double> rows = pad_rows(X, n, e->D, e->DP);
  int rc;
  if ((rc = upload(e->map.x, rows.data(), rows.size(), e->stream)) || (rc = upload(e->map.lpost, lpost, n, e->stream)) ||
      (rc = upload(e->map.ll, llike, n, e->stream)) || (rc = upload(e->map.lp, lprior, n, e->stream)))
    return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

extern "C" int ptm_set_history(ptm_engine* e, const double* X, const double* llike, const double* lprior, const int32_t* meta,
                               const double* invtemps) {
  SETTLE(e);
  NO_BATCH(e, "ptm_set_history");
  if (!e || !X || !llike || !lprior || !meta) return fail(PTM_ERR_INVALID, "null argument");
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "history is off (ptm_config.history_rungs)");
  if (e->hist.beta && !invtemps) return fail(PTM_ERR_INVALID, "an evolving run's history needs the rows' temperatures (ptm_get_history_invtemps)");
  const size_t n = (size_t)e->hist.cap * e->hist.HC;
  const std::vector<double> rows = pad_rows(X, n, e->D, e->DP);
  int rc;
  if ((rc = upload(e->hist.x, rows.data(), rows.size(), e->stream)) || (rc = upload(e->hist.ll, llike, n, e->stream)) ||
      (rc = upload(e->hist.lp, lprior, n, e->stream)) || (rc = upload((int*)e->hist.meta, (const int*)meta, 4 * n, e->stream)))
    return rc;
  if (e->hist.beta && (rc = upload(e->hist.beta, invtemps, n, e->stream))) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

extern "C" int ptm_max_swaps_per_step(ptm_engine* e) { return e ? e->ms : 0; }

extern "C" int ptm_get_history(ptm_engine* e, double* X, double* llike, double* lprior, int32_t* meta) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "history is off (ptm_config.history_rungs)");
  const size_t n = (size_t)e->hist.cap * e->hist.HC, D = e->D, DP = e->DP;
  const unsigned char* s;
  if (X) { FETCH(s, e->hist.x, n * DP * 8); e->fetch_after.push_back([=] { unpad_rows((const double*)s, n, D, DP, X); }); }
  if (llike) { FETCH(s, e->hist.ll, n * 8); e->fetch_after.push_back([=] { memcpy(llike, s, n * 8); }); }
  if (lprior) { FETCH(s, e->hist.lp, n * 8); e->fetch_after.push_back([=] { memcpy(lprior, s, n * 8); }); }
  if (meta) { FETCH(s, e->hist.meta, n * 16); e->fetch_after.push_back([=] { memcpy(meta, s, n * 16); }); }
  return fetch_done(e);
}
// The history ring of chains [chain_begin, chain_begin + chain_count) only, into host arrays of the FULL layout of ptm_get_history
// ([capacity][history chains][..]: the other chains' entries stay as they are): a chain-file writer reads the two or three rungs it
// dumps, not every rung's ring -- with differential evolution on the device the ring holds every rung for the whole run.
extern "C" int ptm_get_history_chains(ptm_engine* e, int chain_begin, int chain_count, double* X, double* llike, double* lprior, int32_t* meta, double* beta) {
  SETTLE(e);
  NO_BATCH(e, "ptm_get_history_chains");
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "history is off (ptm_config.history_rungs)");
  const size_t cap = (size_t)e->hist.cap, HC = (size_t)e->hist.HC, D = e->D, DP = e->DP;
  if (chain_begin < 0 || chain_count < 0 || (size_t)chain_begin + (size_t)chain_count > HC) return fail(PTM_ERR_INVALID, "chain range outside the history's chains");
  if (!chain_count) return PTM_OK;
  const size_t n = (size_t)chain_count, b0 = (size_t)chain_begin;
  HIPCHK(hipStreamSynchronize(e->stream));
  std::vector<double> tmp;
  if (X) {
    tmp.resize(cap * n * DP);
    HIPCHK(hipMemcpy2D(tmp.data(), n * DP * 8, e->hist.x + b0 * DP, HC * DP * 8, n * DP * 8, cap, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < cap; ++r) unpad_rows(tmp.data() + r * n * DP, n, D, DP, X + (r * HC + b0) * D);
  }
  auto scalars = [&](const double* dev, double* out) -> hipError_t { return hipMemcpy2D(out + b0, HC * 8, dev + b0, HC * 8, n * 8, cap, hipMemcpyDeviceToHost); };
  if (llike) HIPCHK(scalars(e->hist.ll, llike));
  if (lprior) HIPCHK(scalars(e->hist.lp, lprior));
  if (meta) HIPCHK(hipMemcpy2D(meta + 4 * b0, HC * 16, reinterpret_cast<const char*>(e->hist.meta) + b0 * 16, HC * 16, n * 16, cap, hipMemcpyDeviceToHost));
  if (beta) {
    if (e->hist.beta) HIPCHK(scalars(e->hist.beta, beta));
    else {
      if (!e->have_ladder) return fail(PTM_ERR_INVALID, "no ladder set");
      for (size_t r = 0; r < cap; ++r)
        for (size_t c = b0; c < b0 + n; ++c) beta[r * HC + c] = e->h_beta[e->r0 + (int)c / e->W];
    }
  }
  return PTM_OK;
}
extern "C" uint64_t ptm_step_count(ptm_engine* e) {
  if (e) (void)ladder_settle(e);
  return e ? e->step : 0;
}

// ---- measurement ------------------------------------------------------------------------------------------------------
extern "C" int ptm_timer_start(ptm_engine* e) {
  SETTLE(e);
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  HIPCHK(hipEventRecord(e->t0, e->stream));
  return PTM_OK;
}
extern "C" int ptm_timer_stop(ptm_engine* e, float* ms) {
  SETTLE(e);
  if (!e || !ms) return fail(PTM_ERR_INVALID, "null argument");
  HIPCHK(hipEventRecord(e->t1, e->stream));
  HIPCHK(hipEventSynchronize(e->t1));
  HIPCHK(hipEventElapsedTime(ms, e->t0, e->t1));
  return PTM_OK;
}
extern "C" int ptm_get_kernel_times(ptm_engine* e, float* ms, int capacity, int* count) {
  SETTLE(e);
  if (!e || !count) return fail(PTM_ERR_INVALID, "null argument");
  HIPCHK(hipStreamSynchronize(e->stream));
  int n = 0;
  for (size_t k = 0; k + 1 < e->kev_used + 1 && k + 1 < e->kev.size() + 1 && k < e->kev_used; k += 2) {
    float t = 0;
    if (ms && n < capacity) {   // (ms == NULL: the records are only dropped -- hundreds of event queries are a gap the device idles in)
      HIPCHK(hipEventElapsedTime(&t, e->kev[k], e->kev[k + 1]));
      ms[n] = t;
    }
    n++;
  }
  *count = n;
  e->kev_used = 0;
  return PTM_OK;
}

extern "C" int ptm_get_ladder_stats(ptm_engine* e, int64_t out[4]) {
  if (!e || !out) return fail(PTM_ERR_INVALID, "null argument");
  SETTLE(e);
  out[0] = e->ladder_launches; out[1] = e->ladder_fallbacks; out[2] = e->ladder_whole_steps; out[3] = e->lad_disabled ? 1 : 0;
  return PTM_OK;
}

extern "C" int ptm_get_counter_sums(ptm_engine* e, int64_t* ntries_sum, int64_t* naccept_sum) {
  if (!e) return fail(PTM_ERR_INVALID, "null engine");
  NO_BATCH(e, "ptm_get_counter_sums");
  int rc = ladder_settle(e);
  if (rc) return rc;
  if (!e->sums) {
    HIPCHK(hipMalloc((void**)&e->sums, 16));
    HIPCHK(hipHostMalloc((void**)&e->h_sums, 16, hipHostMallocDefault));
  }
  HIPCHK(hipMemsetAsync(e->sums, 0, 16, e->stream));
  hipLaunchKernelGGL(counter_sums_kernel, dim3(1024), dim3(256), 0, e->stream, e->ntries, e->naccept, (size_t)e->Nc, e->sums);
  HIPCHK(hipMemcpyAsync(e->h_sums, e->sums, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (ntries_sum) *ntries_sum = (int64_t)e->h_sums[0];
  if (naccept_sum) *naccept_sum = (int64_t)e->h_sums[1];
  return PTM_OK;
}

extern "C" int ptm_get_prefilter_counts(ptm_engine* e, int64_t out[4]) {
  if (!e || !out) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_get_prefilter_counts");
  int rc = ladder_settle(e);
  if (rc) return rc;
  out[0] = out[1] = out[2] = 0;
  out[3] = step_sweep_plan(e).prefilter ? 1 : 0;
  if (!e->pf_counts) return PTM_OK;
  unsigned long long h[2];
  HIPCHK(hipMemcpyAsync(h, e->pf_counts, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  out[0] = (int64_t)h[0]; out[1] = (int64_t)h[1]; out[2] = e->pf_flagged;
  return PTM_OK;
}

extern "C" int ptm_calibrate(ptm_engine* e, ptm_calibration* out) {
  SETTLE(e);
  if (!e || !out) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_calibrate");
  memset(out, 0, sizeof *out);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, e->device));
  const int cus = prop.multiProcessorCount;
  out->compute_units = cus;
  hipEvent_t a = nullptr, b = nullptr;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  // (1) the copy: 2.4 GB read + 2.4 GB written (the bench's state is 4.8 GB), far beyond the 256 MiB Infinity Cache
  const size_t half = (size_t)2400 << 20;
  void *src = nullptr, *dst = nullptr;
  HIPCHK(hipMalloc(&src, half));
  if (hipMalloc(&dst, half) != hipSuccess) { (void)hipFree(src); return fail(PTM_ERR_HIP, "ptm_calibrate: no room for its 4.8 GB of scratch"); }
  HIPCHK(hipMemsetAsync(src, 0x3c, half, e->stream));
  HIPCHK(hipMemsetAsync(dst, 0, half, e->stream));
  float best = 1e30f;
  for (int rep = 0; rep < 6; ++rep) {
    HIPCHK(hipEventRecord(a, e->stream));
    // (a block per 4 KB: tools/probes/copy_probe.hip -- 6.2 TB/s; a persistent grid-stride copy reaches 4.7-5.5, hipMemcpyAsync 4.7)
    hipLaunchKernelGGL(calib_copy_kernel, dim3((unsigned)(half / 16 / 256)), dim3(256), 0, e->stream, (const uint4*)src, (uint4*)dst, half / 16);
    HIPCHK(hipEventRecord(b, e->stream));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    if (rep > 0 && ms < best) best = ms;   // (the first pass warms the clocks and the page tables)
  }
  HIPCHK(hipFree(src));
  HIPCHK(hipFree(dst));
  out->copy_bytes = 2.0 * (double)half;
  out->copy_ms = best;
  out->copy_GBs = 2.0 * (double)half / (best * 1e-3) / 1e9;
  // (2) the f64 issue loop: 4 blocks of 256 threads per CU (four waves per SIMD), 8 chains x iters fma per lane
  const int blocks = cus * 4, iters = 1 << 15;
  double* sink = nullptr;
  long long* clk = nullptr;
  HIPCHK(hipMalloc((void**)&sink, 64));
  HIPCHK(hipMalloc((void**)&clk, (size_t)blocks * 16));
  best = 1e30f;
  std::vector<long long> hc((size_t)blocks * 2);
  for (int rep = 0; rep < 4; ++rep) {
    HIPCHK(hipEventRecord(a, e->stream));
    hipLaunchKernelGGL(calib_fma_kernel, dim3(blocks), dim3(256), 0, e->stream, sink, clk, iters);
    HIPCHK(hipEventRecord(b, e->stream));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    if (rep > 0 && ms < best) { best = ms; HIPCHK(hipMemcpy(hc.data(), clk, hc.size() * 8, hipMemcpyDeviceToHost)); }
  }
  HIPCHK(hipFree(sink));
  HIPCHK(hipFree(clk));
  HIPCHK(hipEventDestroy(a));
  HIPCHK(hipEventDestroy(b));
  std::vector<double> mhz;
  for (int i = 0; i < blocks; ++i)
    if (hc[2 * i + 1] > 0) mhz.push_back(100.0 * (double)hc[2 * i] / (double)hc[2 * i + 1]);
  std::sort(mhz.begin(), mhz.end());
  out->sclk_MHz = mhz.empty() ? 0.0 : mhz[mhz.size() / 2];
  out->fma_ms = best;
  out->f64_fma_TFs = 2.0 * 8.0 * (double)iters * 256.0 * (double)blocks / (best * 1e-3) / 1e12;
  return PTM_OK;
}

extern "C" const char* ptm_sweep_kernel_name(ptm_engine* e) {
  if (!e) return "";
  char b[96];
  if (de_mfma_sweep(e, e->Nc)) format_de_mfma_name(e->prop_kind == PTM_PROP_DENSE ? KIND_DENSE : KIND_LOWER, e->betaC != nullptr, b, sizeof b);
  else format_sweep_name(step_sweep_plan(e), b, sizeof b);   // (in PT steps; the plain sweeps of a big population visit every chain)
  e->kname = b;
  if (e->dfn && e->dprior) e->kname += " + device prior";   // (pack of the valid proposals, the user's work, prior gate)
  if (e->dfn) e->kname += " + device likelihood";   // (propose pass, pack, the user's work, scatter, accept pass)
  return e->kname.c_str();
}

extern "C" const char* ptm_step_kernel_name(ptm_engine* e) {
  if (!e) return "";
  static thread_local std::string name;
  char b[160];
  if (e->nloc != e->Nt) snprintf(b, sizeof b, "(sharded: ptm_exchange_* / ptm_shard_step) decide_kernel + %s", ptm_sweep_kernel_name(e));
  else if (ladder_applies(e)) snprintf(b, sizeof b, "ladder_persistent_kernel<%d, %d, %d>", e->DP, e->prop_kind == PTM_PROP_DIAG ? KIND_DIAG : KIND_DENSE, ladder_flavour(e));
  else if (fused_applies(e)) snprintf(b, sizeof b, "ladder_steps_kernel<%d, %d, %d>", e->DP, e->prop_kind == PTM_PROP_DIAG ? KIND_DIAG : KIND_DENSE, (long long)e->Nt * e->DP <= 64 ? 64 : 256);
  else snprintf(b, sizeof b, "decide_kernel + %s", ptm_sweep_kernel_name(e));
  name = b;
  return name.c_str();
}

// ---- effective sample size on the device (ptm_ess_kernels.hpp) ------------------------------------------------------------
// ess_estimator::windowed (ptmcmc_amd/host/ptmcmc_gpu.hh) for nseries series at once.  The table of nfeat x nwin x nlag cells per series
// lives in a workspace of at most PTM_ESS_WORKSPACE_MB (default 256) MiB: the series are done in chunks that fit it (one series at
// least).  *ws / *ws_bytes: the caller's workspace, grown on demand.
static size_t ess_budget() {
  const char* v = getenv("PTM_ESS_WORKSPACE_MB");
  const double mb = v && *v ? atof(v) : 256.0;
  return mb > 0 ? (size_t)(mb * 1048576.0) : (size_t)256 << 20;
}
static std::vector<int> ess_lags(int every, int burn, int per_window) {   // the facade's loop
  std::vector<int> lags(1, 0);
  double grow = 1;
  for (int k = 1; k < burn * per_window;) {
    lags.push_back(every * k);
    const int was = k;
    while (k == was) { grow *= 1.1; k = (int)grow; }
  }
  return lags;
}
static size_t ess_align(size_t b) { return (b + 255) & ~(size_t)255; }
// steps_of (host, [series of the source], or null: src.steps for all) / sel (host list of the nseries series taken, or null: all in
// order): the series of one pass may differ in length.  *launched: kernels ran (a pass too short for one window runs none).
static int ess_windowed_run(hipStream_t st, void** ws, size_t* ws_bytes, EssSrc src, int nsource, const int* steps_of, const int* sel, int nseries,
                            int nfeat, int width, int every, int burn, double* ess, int32_t* nwin_out, bool* launched) {
  for (int s = 0; s < nseries; ++s) { ess[s] = 0; nwin_out[s] = 0; }
  if (width < 2) width = 2;
  if (every < 1) every = 1;
  if (burn < 1) burn = 1;
  const int per_window = width / every, span = per_window * every;
  if (per_window < 1) return PTM_OK;
  int steps_max = src.steps;
  if (steps_of) {
    steps_max = 0;
    for (int k = 0; k < nseries; ++k) steps_max = std::max(steps_max, steps_of[sel ? sel[k] : k]);
  }
  const int nwin = steps_max / span - burn;   // of the longest series: the table's and the grid's
  if (nwin < 1) return PTM_OK;
  if (nwin > 65535) return fail(PTM_ERR_UNSUPPORTED, "ptm_ess: %d windows (at most 65535: widen them)", nwin);
  if ((double)burn * per_window > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_ess: burn windows x samples per window overflows");
  const std::vector<int> lags = ess_lags(every, burn, per_window);
  const int nlag = (int)lags.size();
  const size_t cells1 = (size_t)nfeat * nwin * nlag;                               // one series' table
  const size_t per_series = cells1 * 20 + (size_t)nfeat * nwin * 8;
  size_t chunk = ess_budget() / per_series;
  if (chunk < 1) chunk = 1;
  if (chunk > (size_t)nseries) chunk = (size_t)nseries;
  if ((double)chunk * nfeat > 2.0e9) chunk = (size_t)(2.0e9 / nfeat);
  const size_t lanes_max = chunk * nfeat;
  const size_t o_lags = 0, o_ess = o_lags + ess_align((size_t)nlag * 4), o_nwin = o_ess + ess_align((size_t)nseries * 8),
               o_sel = o_nwin + ess_align((size_t)nseries * 4), o_steps = o_sel + ess_align(sel ? (size_t)nseries * 4 : 0),
               o_mean = o_steps + ess_align(steps_of ? (size_t)nsource * 4 : 0), o_cov = o_mean + ess_align(lanes_max * nwin * nlag * 8),
               o_cnt = o_cov + ess_align(lanes_max * nwin * nlag * 8), o_e = o_cnt + ess_align(lanes_max * nwin * nlag * 4),
               total = o_e + ess_align(lanes_max * nwin * 8);
  if (*ws_bytes < total) {
    if (*ws) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(*ws)); *ws = nullptr; *ws_bytes = 0; }
    HIPCHK(hipMalloc(ws, total));
    *ws_bytes = total;
  }
  unsigned char* b = (unsigned char*)*ws;
  int* d_lags = (int*)(b + o_lags);
  double* d_ess = (double*)(b + o_ess);
  int* d_nwin = (int*)(b + o_nwin);
  double *d_mean = (double*)(b + o_mean), *d_cov = (double*)(b + o_cov), *d_e = (double*)(b + o_e);
  int* d_cnt = (int*)(b + o_cnt);
  EssWho who = {nullptr, nullptr, span, burn};
  HIPCHK(hipMemcpyAsync(d_lags, lags.data(), (size_t)nlag * 4, hipMemcpyHostToDevice, st));
  if (sel) { who.sel = (const int*)(b + o_sel); HIPCHK(hipMemcpyAsync(b + o_sel, sel, (size_t)nseries * 4, hipMemcpyHostToDevice, st)); }
  if (steps_of) { who.steps_of = (const int*)(b + o_steps); HIPCHK(hipMemcpyAsync(b + o_steps, steps_of, (size_t)nsource * 4, hipMemcpyHostToDevice, st)); }
  HIPCHK(hipStreamSynchronize(st));   // (the lag list is a local; the callers' lists may be too)
  // no division per sample where the saved row of a sample is linear in its number and the ring has not wrapped
  const bool linear = every % src.add_every == 0 && (long long)src.first_row + (steps_max - 1) / src.add_every < (long long)src.cap;
  for (size_t s0 = 0; s0 < (size_t)nseries; s0 += chunk) {
    const int ns = (int)std::min(chunk, (size_t)nseries - s0), lanes = ns * nfeat;
    const dim3 grid((unsigned)((lanes + ESS_THREADS - 1) / ESS_THREADS), (unsigned)nwin, (unsigned)((nlag + ESS_LAGS - 1) / ESS_LAGS));
    if (linear) hipLaunchKernelGGL(ess_accumulate_kernel<true>, grid, dim3(ESS_THREADS), 0, st, src, who, (int)s0, lanes, nfeat, per_window, every, nlag, d_lags, d_mean, d_cov, d_cnt);
    else hipLaunchKernelGGL(ess_accumulate_kernel<false>, grid, dim3(ESS_THREADS), 0, st, src, who, (int)s0, lanes, nfeat, per_window, every, nlag, d_lags, d_mean, d_cov, d_cnt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ess_combine_kernel, dim3(grid.x), dim3(ESS_THREADS), 0, st, src, who, (int)s0, lanes, nfeat, nwin, nlag, d_lags, width, every, d_mean, d_cov, d_cnt, d_e);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ess_reduce_kernel, dim3((unsigned)((ns + ESS_THREADS - 1) / ESS_THREADS)), dim3(ESS_THREADS), 0, st, src, who, (int)s0, ns, nfeat, nwin, d_e, d_ess + s0, d_nwin + s0);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(ess, d_ess, (size_t)nseries * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(nwin_out, d_nwin, (size_t)nseries * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (launched) *launched = true;
  return PTM_OK;
}
// ess_estimator::report: the passes (width, every, burn) it makes for a series of `steps` steps -- they depend on the length and the
// limit alone -- and whether the best of them is taken (the search of esslimit >= 0) or the one pass stands as it is
struct EssPass { int width, every, burn; bool operator<(const EssPass& o) const { return width != o.width ? width < o.width : (every != o.every ? every < o.every : burn < o.burn); } };
static std::vector<EssPass> ess_report_plan(int steps, int width, int every, double esslimit) {
  const int min_burn = 2, min_per_window = 1000, max_windows = 20;
  std::vector<EssPass> plan;
  while (width < steps * 0.05) width *= 2;
  if (esslimit < 0) {
    while (width * (max_windows + min_burn) < steps) width *= 2;
    plan.push_back(EssPass{width, every, min_burn});
    return plan;
  }
  const double length = steps, reach = esslimit * 3.0;
  for (bool last_round = false; !last_round; every *= 2) {
    int windows = (int)(length / (min_per_window * every));
    if (windows > max_windows) windows = max_windows;
    if (windows < 1) break;
    width = (int)(length / windows);
    if (width * (windows - 1) > reach * every) {
      windows = (int)(reach / min_per_window + 1);
      if (windows > max_windows) windows = max_windows;
      if (windows > 1) width = (int)((reach * every) / (windows - 1));
      else { windows = 1; width = min_per_window * every; }
    } else last_round = true;
    if ((length - length / (max_windows + min_burn)) * 0.5 < windows * width) plan.push_back(EssPass{width, every, (int)(length / width - windows)});
  }
  return plan;
}
// ... for every series at once.  Series whose lengths give the same passes (all of them, unless their add_state counts differ and
// with them a width) share each pass; windowed(pass, sel, n, e, nw) runs one for the n series listed in sel (null: all, in order).
#include <map>
template <class F>
static int ess_report_run(const int* steps_of, int steps_common, int nseries, int width, int every, double esslimit, F windowed, double* ess, int32_t* length_out) {
  std::map<std::vector<EssPass>, std::vector<int>> groups;
  {
    std::map<int, std::vector<EssPass>> plans;   // by length
    for (int s = 0; s < nseries; ++s) {
      const int st = steps_of ? steps_of[s] : steps_common;
      auto it = plans.find(st);
      if (it == plans.end()) it = plans.insert(std::make_pair(st, ess_report_plan(st, width, every, esslimit))).first;
      groups[it->second].push_back(s);
    }
  }
  for (int s = 0; s < nseries; ++s) { ess[s] = 0; length_out[s] = 0; }
  for (const auto& g : groups) {
    const std::vector<int>& who = g.second;
    const int n = (int)who.size();
    const int* sel = n == nseries ? nullptr : who.data();
    std::vector<double> e((size_t)n);
    std::vector<int32_t> nw((size_t)n);
    for (const EssPass& p : g.first) {
      const int rc = windowed(p, sel, n, e.data(), nw.data());
      if (rc) return rc;
      for (int k = 0; k < n; ++k) {
        const int s = who[(size_t)k];
        if (esslimit < 0 || e[(size_t)k] > ess[s]) { ess[s] = e[(size_t)k]; length_out[s] = p.width * nw[(size_t)k]; }
      }
    }
  }
  return PTM_OK;
}

// the saved history of local rung `rung` as the kernels' source; steps_of: every walker's own count of add_state calls
// nh: every chain's count of add_state calls, fetched by the caller (ess_ring_counts) -- once for a call that reads many rungs
static int ess_ring_counts(ptm_engine* e, std::vector<int64_t>* nh) {
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "this engine keeps no history (ptm_config.history_rungs)");
  nh->resize((size_t)e->Nc);
  return ptm_get_array(e, PTM_ARR_NHIST, nh->data());
}
static int ess_ring_source_of(ptm_engine* e, const std::vector<int64_t>& nh, int rung, int nfeat, EssSrc* src, std::vector<int>* steps_of) {
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "this engine keeps no history (ptm_config.history_rungs)");
  if (rung < 0 || rung >= e->hist.rungs) return fail(PTM_ERR_INVALID, "rung %d keeps no history (history_rungs = %d)", rung, e->hist.rungs);
  if (nfeat < 1 || nfeat > e->D) return fail(PTM_ERR_INVALID, "nfeat must be in 1..dim (%d)", e->D);
  steps_of->resize((size_t)e->W);
  bool same = true;
  for (int w = 0; w < e->W; ++w) {
    const int64_t st = nh[(size_t)rung * e->W + w];
    if (st > 2000000000) return fail(PTM_ERR_UNSUPPORTED, "ptm_ess: more than 2e9 steps");
    (*steps_of)[(size_t)w] = (int)st;
    same = same && st == nh[(size_t)rung * e->W];
  }
  src->steps = (*steps_of)[0];
  if (same) steps_of->clear();   // (one length for all: no per-series table)
  src->x = e->hist.x + (size_t)rung * e->W * e->DP;
  src->meta = e->hist.meta + (size_t)rung * e->W;
  src->slot_stride = (long long)e->hist.HC * e->DP;
  src->meta_stride = e->hist.HC;
  src->series_stride = e->DP;
  src->cap = e->hist.cap;
  src->add_every = e->cfg.add_every_n;
  src->first_row = 1;
  src->permuted = (e->DP == 32 || e->DP == 64 || e->DP == 128) ? 1 : 0;
  return PTM_OK;
}
static int ess_ring_source(ptm_engine* e, int rung, int nfeat, EssSrc* src, std::vector<int>* steps_of) {
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "this engine keeps no history (ptm_config.history_rungs)");
  if (rung < 0 || rung >= e->hist.rungs) return fail(PTM_ERR_INVALID, "rung %d keeps no history (history_rungs = %d)", rung, e->hist.rungs);
  if (nfeat < 1 || nfeat > e->D) return fail(PTM_ERR_INVALID, "nfeat must be in 1..dim (%d)", e->D);
  std::vector<int64_t> nh;
  int rc = ess_ring_counts(e, &nh);
  if (rc) return rc;
  return ess_ring_source_of(e, nh, rung, nfeat, src, steps_of);
}

extern "C" int ptm_ess_windowed(ptm_engine* e, int rung, int nfeat, int width, int every, int burn, double* ess, int32_t* nwin) {
  if (!e || !ess || !nwin) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_ess_windowed");
  e->ess_on_device = 0;
  EssSrc src;
  std::vector<int> steps_of;
  int rc = ess_ring_source(e, rung, nfeat, &src, &steps_of);
  if (rc) return rc;
  bool launched = false;
  if ((rc = ess_windowed_run(e->stream, &e->ess_ws, &e->ess_ws_bytes, src, e->W, steps_of.empty() ? nullptr : steps_of.data(), nullptr, e->W, nfeat, width, every, burn, ess, nwin, &launched))) return rc;
  e->ess_on_device = launched ? 1 : 0;
  return PTM_OK;
}
extern "C" int ptm_ess_report(ptm_engine* e, int rung, int nfeat, int width, int every, double esslimit, double* ess, int32_t* length) {
  if (!e || !ess || !length) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_ess_report");
  e->ess_on_device = 0;
  if (width < 1 || every < 1) return fail(PTM_ERR_INVALID, "ptm_ess_report: width and every must be >= 1");
  EssSrc src;
  std::vector<int> steps_of;
  int rc = ess_ring_source(e, rung, nfeat, &src, &steps_of);
  if (rc) return rc;
  const int* so = steps_of.empty() ? nullptr : steps_of.data();
  bool launched = false;
  auto pass = [&](const EssPass& p, const int* sel, int n, double* out_e, int32_t* out_n) {
    return ess_windowed_run(e->stream, &e->ess_ws, &e->ess_ws_bytes, src, e->W, so, sel, n, nfeat, p.width, p.every, p.burn, out_e, out_n, &launched);
  };
  if ((rc = ess_report_run(so, src.steps, e->W, width, every, esslimit, pass, ess, length))) return rc;
  e->ess_on_device = launched ? 1 : 0;
  return PTM_OK;
}
extern "C" int ptm_ess_last_on_device(ptm_engine* e) { return e ? e->ess_on_device : 0; }

// a caller's series on the device: series[(t * nseries + s) * nfeat + f]
struct EssSeries {
  double* x = nullptr;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int device_before = -1;   // the caller's current device, put back when the call ends
  EssSrc src;
  ~EssSeries() {
    if (x) (void)hipFree(x);
    if (ws) (void)hipFree(ws);
    if (device_before >= 0) (void)hipSetDevice(device_before);
  }
};
static int ess_series_source(EssSeries* S, int device, const double* series, int64_t n, int nseries, int nfeat) {
  int rc = need_device();
  if (rc) return rc;
  if (!series) return fail(PTM_ERR_INVALID, "null argument");
  if (n < 1 || n > 2000000000 || nseries < 1 || nfeat < 1 || (double)nseries * nfeat > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_ess_series: bad shape");
  if (device >= 0) {
    int cur = -1;
    HIPCHK(hipGetDevice(&cur));
    if (cur != device) { HIPCHK(hipSetDevice(device)); S->device_before = cur; }
  }
  const size_t count = (size_t)n * nseries * nfeat;
  HIPCHK(hipMalloc((void**)&S->x, count * 8));
  HIPCHK(hipMemcpy(S->x, series, count * 8, hipMemcpyHostToDevice));
  S->src.x = S->x; S->src.meta = nullptr;
  S->src.slot_stride = (long long)nseries * nfeat; S->src.meta_stride = 0; S->src.series_stride = nfeat;
  S->src.cap = (int)n; S->src.add_every = 1; S->src.first_row = 0; S->src.permuted = 0; S->src.steps = (int)n;
  return PTM_OK;
}
extern "C" int ptm_ess_series_windowed(int device, const double* series, int64_t n, int nseries, int nfeat, int width, int every, int burn, double* ess,
                                       int32_t* nwin) {
  if (!ess || !nwin) return fail(PTM_ERR_INVALID, "null argument");
  EssSeries S;
  int rc = ess_series_source(&S, device, series, n, nseries, nfeat);
  if (rc) return rc;
  return ess_windowed_run(nullptr, &S.ws, &S.ws_bytes, S.src, nseries, nullptr, nullptr, nseries, nfeat, width, every, burn, ess, nwin, nullptr);
}
extern "C" int ptm_ess_series_report(int device, const double* series, int64_t n, int nseries, int nfeat, int width, int every, double esslimit, double* ess,
                                     int32_t* length) {
  if (!ess || !length) return fail(PTM_ERR_INVALID, "null argument");
  if (width < 1 || every < 1) return fail(PTM_ERR_INVALID, "ptm_ess_series_report: width and every must be >= 1");
  EssSeries S;
  int rc = ess_series_source(&S, device, series, n, nseries, nfeat);
  if (rc) return rc;
  auto pass = [&](const EssPass& p, const int* sel, int k, double* out_e, int32_t* out_n) {
    return ess_windowed_run(nullptr, &S.ws, &S.ws_bytes, S.src, nseries, nullptr, sel, k, nfeat, p.width, p.every, p.burn, out_e, out_n, nullptr);
  };
  return ess_report_run(nullptr, (int)n, nseries, width, every, esslimit, pass, ess, length);
}

// ---- log-evidence by thermodynamic integration on the device (ptm_evidence_kernels.hpp) --------------------------------------
// evidence_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) on the ring where it lies, for every walker's ladder at once.  The kernels
// write into the workspace; the caller's arrays are filled only when no row of a window was missing.
extern "C" int ptm_log_evidence(ptm_engine* e, int ilen, double* log_evidence, double* up, double* down, int32_t* count) {
  if (!e || !log_evidence) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_log_evidence");
  if (ilen < 1) return fail(PTM_ERR_INVALID, "ptm_log_evidence: ilen must be >= 1");
  if (!e->hist.rungs) return fail(PTM_ERR_INVALID, "this engine keeps no history (ptm_config.history_rungs)");
  if (e->nloc != e->Nt) return fail(PTM_ERR_UNSUPPORTED, "ptm_log_evidence on a rung shard (the integral runs over the whole ladder; split populations by walkers)");
  if (e->hist.rungs < e->Nt) return fail(PTM_ERR_INVALID, "ptm_log_evidence reads every rung's saved llikes: history_rungs (%d) must be n_rungs (%d)", e->hist.rungs, e->Nt);
  if (e->Nt < 2) return fail(PTM_ERR_INVALID, "ptm_log_evidence needs a ladder of at least two rungs");
  if (!e->have_ladder) return fail(PTM_ERR_INVALID, "no ladder set");
  const size_t Nc = e->Nc, W = (size_t)e->W, np = (size_t)(e->Nt - 1) * W;
  std::vector<int64_t> nh(Nc);
  int rc = ptm_get_array(e, PTM_ARR_NHIST, nh.data());   // (settles a pending ladder launch and the uncounted adds first)
  if (rc) return rc;
  int64_t nh_max = 0;
  for (size_t c = 0; c < Nc; ++c) nh_max = std::max(nh_max, nh[c]);
  if (nh_max > 2000000000) return fail(PTM_ERR_UNSUPPORTED, "ptm_log_evidence: more than 2e9 steps");
  // the newest saved row of the longest chain: below the capacity, no slot was ever written twice
  const bool wrapped = 1 + (nh_max > 0 ? (nh_max - 1) / e->cfg.add_every_n : 0) >= (int64_t)e->hist.cap;
  const size_t o_up = 0, o_dn = o_up + ess_align(np * 8), o_ev = o_dn + ess_align(np * 8), o_cnt = o_ev + ess_align(W * 8), o_flag = o_cnt + ess_align(Nc * 4),
               total = o_flag + 256;
  if (e->ess_ws_bytes < total) {
    if (e->ess_ws) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->ess_ws)); e->ess_ws = nullptr; e->ess_ws_bytes = 0; }
    HIPCHK(hipMalloc(&e->ess_ws, total));
    e->ess_ws_bytes = total;
  }
  unsigned char* b = (unsigned char*)e->ess_ws;
  double *d_up = (double*)(b + o_up), *d_dn = (double*)(b + o_dn), *d_ev = (double*)(b + o_ev);
  int *d_cnt = (int*)(b + o_cnt), *d_flag = (int*)(b + o_flag);
  EvidSrc src;
  src.ll = e->hist.ll; src.meta = e->hist.meta; src.nhist = e->nhist; src.beta = e->beta; src.beta_w = e->beta_w;
  src.HC = e->hist.HC; src.cap = e->hist.cap; src.W = e->W; src.Nt = e->Nt; src.add_every = e->cfg.add_every_n; src.ilen = ilen;
  HIPCHK(hipMemsetAsync(d_flag, 0, 4, e->stream));
  const dim3 grid((unsigned)((Nc + EVID_THREADS - 1) / EVID_THREADS));
  if (wrapped) hipLaunchKernelGGL(evidence_ratio_kernel<true>, grid, dim3(EVID_THREADS), 0, e->stream, src, d_up, d_dn, d_cnt, d_flag);
  else hipLaunchKernelGGL(evidence_ratio_kernel<false>, grid, dim3(EVID_THREADS), 0, e->stream, src, d_up, d_dn, d_cnt, d_flag);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(evidence_total_kernel, dim3((unsigned)((W + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, e->stream, src, d_up, d_dn, d_ev);
  HIPCHK(hipGetLastError());
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (flag) return fail(PTM_ERR_INVALID, "ptm_log_evidence: history_capacity must hold the evidence window (%d rows hold less than the last %d steps of every chain)", e->hist.cap, ilen);
  HIPCHK(hipMemcpyAsync(log_evidence, d_ev, W * 8, hipMemcpyDeviceToHost, e->stream));
  if (up) HIPCHK(hipMemcpyAsync(up, d_up, np * 8, hipMemcpyDeviceToHost, e->stream));
  if (down) HIPCHK(hipMemcpyAsync(down, d_dn, np * 8, hipMemcpyDeviceToHost, e->stream));
  if (count) HIPCHK(hipMemcpyAsync(count, d_cnt, Nc * 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PTM_OK;
}

// ---- split R-hat across the walkers of a rung on the device (ptm_rhat_kernels.hpp) ------------------------------------------
// rhat_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) on the ring where it lies, or on a caller's series.  The kernels write into the
// workspace; the caller's arrays are filled only when no row of a window was missing.  d_nhist: the chains' own counts of add_state
// calls on the device (null: src.steps for all); wrapped: a slot may have been written twice.
static int rhat_run(hipStream_t st, void** ws, size_t* ws_bytes, EssSrc src, const unsigned int* d_nhist, bool wrapped, int W, int nfeat, int nrows,
                    double* rhat, double* mean, double* within, double* between, double* seq_mean, double* seq_var) {
  const size_t lanes = (size_t)2 * W * nfeat;
  const size_t o_mean = 0, o_var = o_mean + ess_align(lanes * 8), o_out = o_var + ess_align(lanes * 8), o_flag = o_out + ess_align((size_t)4 * nfeat * 8),
               total = o_flag + 256;
  if (*ws_bytes < total) {
    if (*ws) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(*ws)); *ws = nullptr; *ws_bytes = 0; }
    HIPCHK(hipMalloc(ws, total));
    *ws_bytes = total;
  }
  unsigned char* b = (unsigned char*)*ws;
  double *d_mean = (double*)(b + o_mean), *d_var = (double*)(b + o_var), *d_out = (double*)(b + o_out);
  int* d_flag = (int*)(b + o_flag);
  HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
  const dim3 grid((unsigned)((lanes + RHAT_THREADS - 1) / RHAT_THREADS));
  if (wrapped) hipLaunchKernelGGL(rhat_sequence_kernel<true>, grid, dim3(RHAT_THREADS), 0, st, src, d_nhist, W, nfeat, nrows, d_mean, d_var, d_flag);
  else hipLaunchKernelGGL(rhat_sequence_kernel<false>, grid, dim3(RHAT_THREADS), 0, st, src, d_nhist, W, nfeat, nrows, d_mean, d_var, d_flag);
  HIPCHK(hipGetLastError());
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag) return fail(PTM_ERR_INVALID, "ptm_rhat: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", src.cap, nrows);
  hipLaunchKernelGGL(rhat_reduce_kernel, dim3((unsigned)((nfeat + RHAT_THREADS - 1) / RHAT_THREADS)), dim3(RHAT_THREADS), 0, st, 2 * W, nfeat, nrows / 2, d_mean, d_var, d_out);
  HIPCHK(hipGetLastError());
  std::vector<double> out((size_t)4 * nfeat);
  HIPCHK(hipMemcpyAsync(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost, st));
  if (seq_mean) HIPCHK(hipMemcpyAsync(seq_mean, d_mean, lanes * 8, hipMemcpyDeviceToHost, st));
  if (seq_var) HIPCHK(hipMemcpyAsync(seq_var, d_var, lanes * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int f = 0; f < nfeat; ++f) {
    const size_t F = (size_t)f, N = (size_t)nfeat;
    if (mean) mean[f] = out[F];
    if (within) within[f] = out[N + F];
    if (between) between[f] = out[2 * N + F];
    rhat[f] = std::sqrt(out[3 * N + F] / out[N + F]);   // (the host's IEEE division and square root)
  }
  return PTM_OK;
}
static int rhat_shape(const char* who, int nfeat_max, int nfeat, int nrows) {
  if (nfeat < 1 || nfeat > nfeat_max) return fail(PTM_ERR_INVALID, "%s: nfeat must be in 1..%d", who, nfeat_max);
  if (nrows < 4 || (nrows & 1)) return fail(PTM_ERR_INVALID, "%s: nrows must be even and at least 4", who);
  return PTM_OK;
}
extern "C" int ptm_rhat(ptm_engine* e, int rung, int nfeat, int nrows, double* rhat, double* mean, double* within, double* between, double* seq_mean,
                        double* seq_var) {
  if (!e || !rhat) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_rhat");
  int rc = rhat_shape("ptm_rhat", e->D, nfeat, nrows);
  if (rc) return rc;
  EssSrc src;
  std::vector<int> steps_of;
  if ((rc = ess_ring_source(e, rung, nfeat, &src, &steps_of))) return rc;   // (settles a pending ladder launch and the uncounted adds first)
  if ((double)2 * e->W * nfeat > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_rhat: bad shape");
  long long newest_min = 0, newest_max = 0;
  for (int w = 0; w < e->W; ++w) {
    const long long st = steps_of.empty() ? src.steps : steps_of[(size_t)w];
    const long long newest = st > 0 ? 1 + (st - 1) / src.add_every : 0;   // (= the saved rows behind the start state)
    if (!w || newest < newest_min) newest_min = newest;
    if (!w || newest > newest_max) newest_max = newest;
  }
  if (newest_min < nrows) return fail(PTM_ERR_INVALID, "ptm_rhat: a chain of the rung has saved %lld rows behind its start state, fewer than nrows (%d)", newest_min, nrows);
  if (nrows > src.cap) return fail(PTM_ERR_INVALID, "ptm_rhat: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", src.cap, nrows);
  return rhat_run(e->stream, &e->ess_ws, &e->ess_ws_bytes, src, e->nhist + (size_t)rung * e->W, newest_max >= (long long)src.cap, e->W, nfeat, nrows, rhat, mean, within,
                  between, seq_mean, seq_var);
}
extern "C" int ptm_rhat_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, double* rhat, double* mean, double* within,
                               double* between, double* seq_mean, double* seq_var) {
  if (!rhat) return fail(PTM_ERR_INVALID, "null argument");
  int rc = rhat_shape("ptm_rhat_series", 2000000000, nfeat, nrows);
  if (rc) return rc;
  if ((int64_t)nrows > n) return fail(PTM_ERR_INVALID, "ptm_rhat_series: the series have %lld rows, fewer than nrows (%d)", (long long)n, nrows);
  if (nseries >= 1 && (double)2 * nseries * nfeat > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_rhat_series: bad shape");
  EssSeries S;
  if ((rc = ess_series_source(&S, device, series, n, nseries, nfeat))) return rc;
  return rhat_run(nullptr, &S.ws, &S.ws_bytes, S.src, nullptr, false, nseries, nfeat, nrows, rhat, mean, within, between, seq_mean, seq_var);
}

// ---- pooled posterior mean and covariance of a rung on the device (ptm_moments_kernels.hpp) ---------------------------------
// moments_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) on the ring where it lies, or on a caller's series.  The kernels write into the
// workspace; the caller's arrays are filled only when no row of a window was missing.  d_nhist, wrapped: as rhat_run's.
// The per-walker pair sums of the cross kernel are made and folded into their blocks' sums a group of walkers at a time (whole
// blocks, MOM_WS_BYTES of workspace at most; PTM_MOMENTS_GROUP=n walkers in the environment forces the size: tests).
static constexpr size_t MOM_WS_BYTES = (size_t)256 << 20;
// One call's plan: the walkers' sums, pair sums and blocks' sums (used by one rung after the other, in stream order) and every rung's
// own means, answers and flag, rung r at d_mean + r * F, d_out + r * out_stride, d_flag + r.
struct MomPlan {
  size_t F = 0, lanes = 0, P = 0, nblocks = 0, group = 0, out_stride = 0;
  double *d_sw = nullptr, *d_cw = nullptr, *d_blk = nullptr, *d_mean = nullptr, *d_out = nullptr;
  int* d_flag = nullptr;
};
static int moments_plan(hipStream_t st, void** ws, size_t* ws_bytes, int W, int nfeat, bool cov, bool var, int n_rungs, MomPlan* pl) {
  const size_t F = (size_t)nfeat, lanes = (size_t)W * F, P = cov ? F * (F + 1) / 2 : 0, nblocks = ((size_t)W + MOM_GROUP - 1) / MOM_GROUP, R = (size_t)n_rungs;
  size_t group = (size_t)W;   // walkers whose pair sums the workspace holds at a time
  if (cov) {
    const char* v = getenv("PTM_MOMENTS_GROUP");
    const long long forced = v && *v ? atoll(v) : 0;
    group = forced > 0 ? (size_t)forced : MOM_WS_BYTES / (P * 8);
    group = std::max((size_t)MOM_GROUP, group / MOM_GROUP * MOM_GROUP);
    group = std::min(group, nblocks * MOM_GROUP);
  }
  const size_t n_walker = cov ? group * P : (var ? lanes : 0), n_block = nblocks * std::max(F, P), out_stride = cov ? F * F : F;
  const size_t o_sw = 0, o_cw = o_sw + ess_align(lanes * 8), o_blk = o_cw + ess_align(n_walker * 8), o_mean = o_blk + ess_align(n_block * 8),
               o_out = o_mean + ess_align(R * F * 8), o_flag = o_out + ess_align(R * out_stride * 8), total = o_flag + std::max((size_t)256, ess_align(R * 4));
  if (*ws_bytes < total) {
    if (*ws) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(*ws)); *ws = nullptr; *ws_bytes = 0; }
    HIPCHK(hipMalloc(ws, total));
    *ws_bytes = total;
  }
  unsigned char* b = (unsigned char*)*ws;
  pl->F = F; pl->lanes = lanes; pl->P = P; pl->nblocks = nblocks; pl->group = group; pl->out_stride = out_stride;
  pl->d_sw = (double*)(b + o_sw); pl->d_cw = (double*)(b + o_cw); pl->d_blk = (double*)(b + o_blk); pl->d_mean = (double*)(b + o_mean); pl->d_out = (double*)(b + o_out);
  pl->d_flag = (int*)(b + o_flag);
  HIPCHK(hipMemsetAsync(pl->d_flag, 0, R * 4, st));
  return PTM_OK;
}
// the kernels of rung r of the plan, on the stream
static int moments_launch(hipStream_t st, const MomPlan& pl, int r, EssSrc src, const unsigned int* d_nhist, bool wrapped, int W, int nfeat, int nrows, bool cov,
                          bool var) {
  const int64_t N = (int64_t)W * nrows;
  const size_t F = pl.F, lanes = pl.lanes, P = pl.P, nblocks = pl.nblocks, group = pl.group;
  double *d_sw = pl.d_sw, *d_cw = pl.d_cw, *d_blk = pl.d_blk, *d_mean = pl.d_mean + (size_t)r * F, *d_out = pl.d_out + (size_t)r * pl.out_stride;
  int* d_flag = pl.d_flag + r;
  const dim3 T(MOM_THREADS);
  auto blocks_of = [](size_t n) { return dim3((unsigned)((n + MOM_THREADS - 1) / MOM_THREADS)); };
  // the means: s_w, S_b, S / N
  if (wrapped) hipLaunchKernelGGL(moments_sum_kernel<true>, blocks_of(lanes), T, 0, st, src, d_nhist, W, nfeat, nrows, (const double*)nullptr, d_sw, d_flag);
  else hipLaunchKernelGGL(moments_sum_kernel<false>, blocks_of(lanes), T, 0, st, src, d_nhist, W, nfeat, nrows, (const double*)nullptr, d_sw, d_flag);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(moments_block_kernel, blocks_of(nblocks * F), T, 0, st, W, nfeat, (const double*)d_sw, d_blk);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(moments_final_kernel, blocks_of(F), T, 0, st, (int)nblocks, nfeat, (const double*)d_blk, (double)N, 0, d_mean);
  HIPCHK(hipGetLastError());
  if (cov) {   // c_w, C_b, C / (N - 1): every pair
    // pairs a lane: as few as hold every pair in one chunk, MOM_PAIRS at most; then as many chunks as hold them all
    const int np = (int)std::min((size_t)MOM_PAIRS, (P + MOM_THREADS - 1) / MOM_THREADS);
    const unsigned chunks = (unsigned)((P + (size_t)MOM_THREADS * np - 1) / ((size_t)MOM_THREADS * np));
    void (*const cross[2][MOM_PAIRS])(EssSrc, const unsigned int*, int, int, int, int, const double*, double*, int*) = {
        {moments_cross_kernel<false, 1>, moments_cross_kernel<false, 2>, moments_cross_kernel<false, 3>, moments_cross_kernel<false, 4>},
        {moments_cross_kernel<true, 1>, moments_cross_kernel<true, 2>, moments_cross_kernel<true, 3>, moments_cross_kernel<true, 4>}};
    static_assert(MOM_PAIRS == 4, "one kernel per number of pairs a lane");
    for (size_t w0 = 0; w0 < (size_t)W; w0 += group) {
      const int nw = (int)std::min(group, (size_t)W - w0);
      const dim3 grid((unsigned)nw, chunks);
      hipLaunchKernelGGL(cross[wrapped ? 1 : 0][np - 1], grid, T, 0, st, src, d_nhist, (int)w0, nfeat, nrows, (int)P, (const double*)d_mean, d_cw, d_flag);
      HIPCHK(hipGetLastError());
      const size_t nb = ((size_t)nw + MOM_GROUP - 1) / MOM_GROUP;
      hipLaunchKernelGGL(moments_block_kernel, blocks_of(nb * P), T, 0, st, nw, (int)P, (const double*)d_cw, d_blk + (w0 / MOM_GROUP) * P);
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(moments_final_kernel, blocks_of(P), T, 0, st, (int)nblocks, (int)P, (const double*)d_blk, (double)(N - 1), nfeat, d_out);
    HIPCHK(hipGetLastError());
  } else if (var) {   // the diagonal pairs alone
    if (wrapped) hipLaunchKernelGGL(moments_sum_kernel<true>, blocks_of(lanes), T, 0, st, src, d_nhist, W, nfeat, nrows, (const double*)d_mean, d_cw, d_flag);
    else hipLaunchKernelGGL(moments_sum_kernel<false>, blocks_of(lanes), T, 0, st, src, d_nhist, W, nfeat, nrows, (const double*)d_mean, d_cw, d_flag);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(moments_block_kernel, blocks_of(nblocks * F), T, 0, st, W, nfeat, (const double*)d_cw, d_blk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(moments_final_kernel, blocks_of(F), T, 0, st, (int)nblocks, nfeat, (const double*)d_blk, (double)(N - 1), 0, d_out);
    HIPCHK(hipGetLastError());
  }
  return PTM_OK;
}
// the flags of the plan's n_rungs rungs: one wait; any raised: the window is not there
static int moments_flags(const char* who, hipStream_t st, const MomPlan& pl, int n_rungs, int cap, int nrows) {
  std::vector<int> flag((size_t)n_rungs, 0);
  HIPCHK(hipMemcpyAsync(flag.data(), pl.d_flag, (size_t)n_rungs * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int f : flag)
    if (f) return fail(PTM_ERR_INVALID, "%s: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", who, cap, nrows);
  return PTM_OK;
}
static int moments_run(const char* who, hipStream_t st, void** ws, size_t* ws_bytes, EssSrc src, const unsigned int* d_nhist, bool wrapped, int W, int nfeat,
                       int nrows, double* mean, double* cov, double* var, double* walker_sum, int64_t* count) {
  MomPlan pl;
  int rc;
  if ((rc = moments_plan(st, ws, ws_bytes, W, nfeat, cov != nullptr, var != nullptr, 1, &pl))) return rc;
  if ((rc = moments_launch(st, pl, 0, src, d_nhist, wrapped, W, nfeat, nrows, cov != nullptr, var != nullptr))) return rc;
  if ((rc = moments_flags(who, st, pl, 1, src.cap, nrows))) return rc;
  const size_t F = pl.F;
  HIPCHK(hipMemcpyAsync(mean, pl.d_mean, F * 8, hipMemcpyDeviceToHost, st));
  if (cov) HIPCHK(hipMemcpyAsync(cov, pl.d_out, F * F * 8, hipMemcpyDeviceToHost, st));
  else if (var) HIPCHK(hipMemcpyAsync(var, pl.d_out, F * 8, hipMemcpyDeviceToHost, st));
  if (walker_sum) HIPCHK(hipMemcpyAsync(walker_sum, pl.d_sw, pl.lanes * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (cov && var)
    for (size_t f = 0; f < F; ++f) var[f] = cov[f * F + f];   // (the diagonal pair's quotient: the same bits)
  if (count) *count = (int64_t)W * nrows;
  return PTM_OK;
}
static int moments_shape(const char* who, int nfeat_max, int nfeat, int nrows, const double* cov) {
  if (nfeat < 1 || nfeat > nfeat_max) return fail(PTM_ERR_INVALID, "%s: nfeat must be in 1..%d", who, nfeat_max);
  if (nrows < 1) return fail(PTM_ERR_INVALID, "%s: nrows must be at least 1", who);
  if (cov && nfeat > MOM_COV_NFEAT_MAX) return fail(PTM_ERR_UNSUPPORTED, "%s: the covariance is offered up to %d features (pass cov = NULL for the mean and the variances)", who, MOM_COV_NFEAT_MAX);
  return PTM_OK;
}
// the window of one rung against its chains' counts: what ptm_moments refuses; *wrapped: the ring no longer holds every row since the start
static int moments_window_check(const char* who, const ptm_engine* e, const EssSrc& src, const std::vector<int>& steps_of, int nrows, bool* wrapped) {
  if ((int64_t)e->W * nrows < 2) return fail(PTM_ERR_INVALID, "%s: at least two samples are needed (walkers x nrows = %lld)", who, (long long)e->W * nrows);
  long long newest_min = 0, newest_max = 0;
  for (int w = 0; w < e->W; ++w) {
    const long long st = steps_of.empty() ? src.steps : steps_of[(size_t)w];
    const long long newest = st > 0 ? 1 + (st - 1) / src.add_every : 0;   // (= the saved rows behind the start state)
    if (!w || newest < newest_min) newest_min = newest;
    if (!w || newest > newest_max) newest_max = newest;
  }
  if (newest_min < nrows) return fail(PTM_ERR_INVALID, "%s: a chain of the rung has saved %lld rows behind its start state, fewer than nrows (%d)", who, newest_min, nrows);
  if (nrows > src.cap) return fail(PTM_ERR_INVALID, "%s: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", who, src.cap, nrows);
  *wrapped = newest_max >= (long long)src.cap;
  return PTM_OK;
}
extern "C" int ptm_moments(ptm_engine* e, int rung, int nfeat, int nrows, double* mean, double* cov, double* var, double* walker_sum, int64_t* count) {
  if (!e || !mean) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_moments");
  int rc = moments_shape("ptm_moments", e->D, nfeat, nrows, cov);
  if (rc) return rc;
  EssSrc src;
  std::vector<int> steps_of;
  if ((rc = ess_ring_source(e, rung, nfeat, &src, &steps_of))) return rc;   // (settles a pending ladder launch and the uncounted adds first)
  if ((double)e->W * nfeat > 2.0e9 || (double)e->W * nrows > 4.0e18) return fail(PTM_ERR_INVALID, "ptm_moments: bad shape");
  bool wrapped = false;
  if ((rc = moments_window_check("ptm_moments", e, src, steps_of, nrows, &wrapped))) return rc;
  return moments_run("ptm_moments", e->stream, &e->ess_ws, &e->ess_ws_bytes, src, e->nhist + (size_t)rung * e->W, wrapped, e->W, nfeat, nrows,
                     mean, cov, var, walker_sum, count);
}
// ptm_moments for a range of rungs: the kernels of one rung after the other on the stream, every rung's answers kept in the workspace,
// nothing waited for.  *plan: where they lie (ptm_adapt_proposals reads them there) and the flags the caller has to look at (a
// raised one: a window's row was lost).  Checks every rung's window against the counts before anything is launched.
static int moments_rungs_device(const char* who, ptm_engine* e, int first_rung, int n_rungs, int nfeat, int nrows, bool cov, bool var, MomPlan* plan) {
  const double some = 0;
  int rc = moments_shape(who, e->D, nfeat, nrows, cov ? &some : nullptr);
  if (rc) return rc;
  std::vector<int64_t> nh;
  if ((rc = ess_ring_counts(e, &nh))) return rc;   // (settles a pending ladder launch and the uncounted adds first)
  if (n_rungs < 1 || first_rung < 0 || first_rung > e->hist.rungs - n_rungs)
    return fail(PTM_ERR_INVALID, "%s: rungs %d .. %d are not all recorded (history_rungs = %d)", who, first_rung, first_rung + n_rungs - 1, e->hist.rungs);
  if ((double)e->W * nfeat > 2.0e9 || (double)e->W * nrows > 4.0e18) return fail(PTM_ERR_INVALID, "%s: bad shape", who);
  std::vector<EssSrc> src((size_t)n_rungs);
  std::vector<char> wrapped((size_t)n_rungs, 0);
  std::vector<int> steps_of;
  for (int r = 0; r < n_rungs; ++r) {
    if ((rc = ess_ring_source_of(e, nh, first_rung + r, nfeat, &src[(size_t)r], &steps_of))) return rc;
    bool wr = false;
    if ((rc = moments_window_check(who, e, src[(size_t)r], steps_of, nrows, &wr))) return rc;
    wrapped[(size_t)r] = wr ? 1 : 0;
  }
  if ((rc = moments_plan(e->stream, &e->ess_ws, &e->ess_ws_bytes, e->W, nfeat, cov, var, n_rungs, plan))) return rc;
  for (int r = 0; r < n_rungs; ++r)
    if ((rc = moments_launch(e->stream, *plan, r, src[(size_t)r], e->nhist + (size_t)(first_rung + r) * e->W, wrapped[(size_t)r] != 0, e->W, nfeat, nrows, cov, var)))
      return rc;
  return PTM_OK;
}
extern "C" int ptm_moments_rungs(ptm_engine* e, int first_rung, int n_rungs, int nfeat, int nrows, double* mean, double* cov, double* var, int64_t* count) {
  if (!e || !mean) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_moments_rungs");
  MomPlan pl;
  int rc = moments_rungs_device("ptm_moments_rungs", e, first_rung, n_rungs, nfeat, nrows, cov != nullptr, var != nullptr, &pl);
  if (rc) return rc;
  const size_t F = pl.F, R = (size_t)n_rungs, n_out = cov || var ? R * pl.out_stride : 0;
  hipStream_t st = e->stream;
  std::vector<double> h_mean(R * F), h_out(n_out);   // (staged: the caller's arrays stay untouched when a flag is raised, and the call waits once)
  std::vector<int> flag(R, 0);
  HIPCHK(hipMemcpyAsync(h_mean.data(), pl.d_mean, R * F * 8, hipMemcpyDeviceToHost, st));
  if (n_out) HIPCHK(hipMemcpyAsync(h_out.data(), pl.d_out, n_out * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(flag.data(), pl.d_flag, R * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int f : flag)
    if (f) return fail(PTM_ERR_INVALID, "ptm_moments_rungs: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", e->hist.cap, nrows);
  memcpy(mean, h_mean.data(), R * F * 8);
  if (cov) memcpy(cov, h_out.data(), n_out * 8);
  else if (var) memcpy(var, h_out.data(), n_out * 8);
  if (cov && var)
    for (size_t r = 0; r < R; ++r)
      for (size_t f = 0; f < F; ++f) var[r * F + f] = cov[(r * F + f) * F + f];   // (the diagonal pair's quotient: the same bits)
  if (count) *count = (int64_t)e->W * nrows;
  return PTM_OK;
}
extern "C" int ptm_moments_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, double* mean, double* cov, double* var,
                                  double* walker_sum, int64_t* count) {
  if (!mean || !series) return fail(PTM_ERR_INVALID, "null argument");
  int rc = moments_shape("ptm_moments_series", 2000000000, nfeat, nrows, cov);
  if (rc) return rc;
  if ((int64_t)nrows > n) return fail(PTM_ERR_INVALID, "ptm_moments_series: the series have %lld rows, fewer than nrows (%d)", (long long)n, nrows);
  if (nseries >= 1 && (int64_t)nseries * nrows < 2) return fail(PTM_ERR_INVALID, "ptm_moments_series: at least two samples are needed (series x nrows = %lld)", (long long)nseries * nrows);
  EssSeries S;
  if ((rc = ess_series_source(&S, device, series, n, nseries, nfeat))) return rc;
  return moments_run("ptm_moments_series", nullptr, &S.ws, &S.ws_bytes, S.src, nullptr, false, nseries, nfeat, nrows, mean, cov, var, walker_sum, count);
}
extern "C" int ptm_moments_tile_rows(int nfeat) { return nfeat >= 1 && nfeat <= MOM_COV_NFEAT_MAX ? moments_tile_rows(nfeat) : 0; }

// ---- Gaussian proposal factors of a batch of covariances; every rung's proposal from its own samples (ptm_eigen_kernels.hpp) ----
// gaussian_prop::eigen_factor (ptmcmc_amd/host/ptmcmc_gpu.hh) for n_mat matrices at d_cov, one workgroup each.  d_qt: [n_mat][n*n],
// needed above EIG_Q_LDS_N_MAX dimensions.
static int eigen_launch(hipStream_t st, const double* d_cov, int n_mat, int n, double scale, double* d_qt, double* d_fac, double* d_lam, int32_t* d_sweeps) {
  const size_t lds = eigen_lds_bytes(n);
  void (*const kf)(const double*, int, double, double*, double*, double*, int32_t*) = eigen_q_in_lds(n) ? eigen_factor_kernel<true> : eigen_factor_kernel<false>;
  if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kf, dim3((unsigned)n_mat), dim3((unsigned)eigen_threads(n)), lds, st, d_cov, n, scale, d_qt, d_fac, d_lam, d_sweeps);
  HIPCHK(hipGetLastError());
  return PTM_OK;
}
extern "C" int ptm_eigen_factors(int device, const double* cov, int n_mat, int n, double* factors, double* lambda, int32_t* sweeps) {
  if (!cov || !factors) return fail(PTM_ERR_INVALID, "null argument");
  if (n < 1 || n > EIG_N_MAX) return fail(PTM_ERR_INVALID, "ptm_eigen_factors: n must be in 1..%d", EIG_N_MAX);
  if (n_mat < 1 || (double)n_mat * n * n > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_eigen_factors: bad shape");
  int rc = need_device();
  if (rc) return rc;
  struct Scope {
    void* ws = nullptr;
    int device_before = -1;
    ~Scope() {
      if (ws) (void)hipFree(ws);
      if (device_before >= 0) (void)hipSetDevice(device_before);
    }
  } S;
  if (device >= 0) {
    int cur = -1;
    HIPCHK(hipGetDevice(&cur));
    if (cur != device) { HIPCHK(hipSetDevice(device)); S.device_before = cur; }
  }
  const size_t M = (size_t)n_mat, nn = (size_t)n * n;
  const size_t o_cov = 0, o_fac = o_cov + ess_align(M * nn * 8), o_qt = o_fac + ess_align(M * nn * 8), o_lam = o_qt + (eigen_q_in_lds(n) ? 0 : ess_align(M * nn * 8)),
               o_sw = o_lam + ess_align(M * n * 8), total = o_sw + ess_align(M * 4);
  HIPCHK(hipMalloc(&S.ws, total));
  unsigned char* b = (unsigned char*)S.ws;
  double *d_cov = (double*)(b + o_cov), *d_fac = (double*)(b + o_fac), *d_qt = (double*)(b + o_qt), *d_lam = (double*)(b + o_lam);
  int32_t* d_sw = (int32_t*)(b + o_sw);
  HIPCHK(hipMemcpy(d_cov, cov, M * nn * 8, hipMemcpyHostToDevice));
  if ((rc = eigen_launch(nullptr, d_cov, n_mat, n, 1.0, d_qt, d_fac, d_lam, d_sw))) return rc;
  HIPCHK(hipMemcpy(factors, d_fac, M * nn * 8, hipMemcpyDeviceToHost));
  if (lambda) HIPCHK(hipMemcpy(lambda, d_lam, M * n * 8, hipMemcpyDeviceToHost));
  if (sweeps) HIPCHK(hipMemcpy(sweeps, d_sw, M * 4, hipMemcpyDeviceToHost));
  return PTM_OK;
}

// Every rung's Gaussian factor from that rung's own pooled moments: moments and eigen-decompositions stay on the device; the factors
// come back once for the packer that ptm_set_proposal_rung uses (install_rung_factor).
extern "C" int ptm_adapt_proposals(ptm_engine* e, int first_rung, int n_rungs, int nrows, double scale, int32_t* status, double* factors_out) {
  if (!e || !status) return fail(PTM_ERR_INVALID, "null argument");
  if (e->fetch_depth > 0) return fail(PTM_ERR_UNSUPPORTED, "ptm_adapt_proposals between ptm_batch_begin and ptm_batch_end (only reads go there)");
  if (!e->have_prop) return fail(PTM_ERR_INVALID, "set all proposals first (ptm_set_proposals)");
  if (user_prop(e)) return fail(PTM_ERR_INVALID, "ptm_adapt_proposals: user proposals (host-side or device) are set: the factors are not read");
  if (!(scale > 0) || !(scale < HUGE_VAL)) return fail(PTM_ERR_INVALID, "ptm_adapt_proposals: scale must be finite and above 0");
  if (e->prop_kind == KIND_LOWER) return fail(PTM_ERR_UNSUPPORTED, "ptm_adapt_proposals: no Cholesky form (PTM_PROP_LOWER) is built");
  const bool diag = e->prop_kind == KIND_DIAG;
  const int D = e->D;
  if (!diag && D > EIG_N_MAX) return fail(PTM_ERR_UNSUPPORTED, "ptm_adapt_proposals: dense factors are offered up to %d dimensions", EIG_N_MAX);
  MomPlan pl;
  int rc = moments_rungs_device("ptm_adapt_proposals", e, first_rung, n_rungs, D, nrows, !diag, diag, &pl);
  if (rc) return rc;
  const size_t R = (size_t)n_rungs, fsz = diag ? (size_t)D : (size_t)D * D;
  const bool qt = !diag && !eigen_q_in_lds(D);
  const size_t o_fac = 0, o_qt = o_fac + ess_align(R * fsz * 8), o_lam = o_qt + (qt ? ess_align(R * fsz * 8) : 0), o_st = o_lam + ess_align(R * D * 8),
               total = o_st + ess_align(R * 4);
  hipStream_t st = e->stream;
  if (e->eig_ws_bytes < total) {
    if (e->eig_ws) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(e->eig_ws)); e->eig_ws = nullptr; e->eig_ws_bytes = 0; }
    HIPCHK(hipMalloc(&e->eig_ws, total));
    e->eig_ws_bytes = total;
  }
  unsigned char* b = (unsigned char*)e->eig_ws;
  double *d_fac = (double*)(b + o_fac), *d_qt = (double*)(b + o_qt), *d_lam = (double*)(b + o_lam);
  int32_t* d_st = (int32_t*)(b + o_st);
  if (diag) {
    hipLaunchKernelGGL(diag_factor_kernel, dim3((unsigned)R), dim3(EIG_STATUS_THREADS), 0, st, (const double*)pl.d_out, D, scale, d_fac, d_st);
    HIPCHK(hipGetLastError());
  } else {
    if ((rc = eigen_launch(st, pl.d_out, n_rungs, D, scale, d_qt, d_fac, d_lam, nullptr))) return rc;
    hipLaunchKernelGGL(eigen_status_kernel, dim3((unsigned)R), dim3(EIG_STATUS_THREADS), 0, st, (const double*)pl.d_out, (const double*)d_lam, D, d_st);
    HIPCHK(hipGetLastError());
  }
  std::vector<double> fac(R * fsz);
  std::vector<int32_t> stat(R, 0);
  HIPCHK(hipMemcpyAsync(fac.data(), d_fac, R * fsz * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(stat.data(), d_st, R * 4, hipMemcpyDeviceToHost, st));
  if ((rc = moments_flags("ptm_adapt_proposals", st, pl, n_rungs, e->hist.cap, nrows))) return rc;   // (the wait; nothing has changed yet)
  std::vector<std::vector<double> > pending;   // the host images of the enqueued copies: one wait for all the rungs
  pending.reserve(2 * R);
  for (size_t r = 0; r < R; ++r)
    if (stat[r] == 0 && (rc = install_rung_factor(e, first_rung + (int)r, fac.data() + r * fsz, &pending))) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
  HIPCHK(hipStreamSynchronize(st));
  memcpy(status, stat.data(), R * 4);
  if (factors_out) memcpy(factors_out, fac.data(), R * fsz * 8);
  return PTM_OK;
}

// ---- exact posterior quantiles of a rung on the device (ptm_quantiles_kernels.hpp) -------------------------------------------
// quantile_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) on the ring where it lies, or on a caller's series: radix selection of the
// order statistics, the interpolation formed here from them.  d_nhist, wrapped: as rhat_run's.  The caller's arrays are filled
// only when no row of a window was missing.
// Choices, every one forceable from the environment (tests, the probe); the bits do not depend on them:
//   PTM_QUANTILES_PATH=ring|packed   ring (the default): every pass walks the ring.  packed: after a pass the keys that are still
//       candidates are copied into the workspace as soon as they fit, and the passes after that read the copy.  Measured
//       (profiles/quantiles_device.json), the copy costs more than the walks it saves -- its kernel draws every position from one
//       counter per feature, and those returning atomics serialise -- so nothing packs unless it is asked to.
//   PTM_QUANTILES_PACK_BYTES=n       the room of the copy (QNT_PACK_BYTES at most).  Candidates that do not fit -- ties can keep
//       every key a candidate -- stay where they are: the passes go on walking the ring.
//   PTM_QUANTILES_TILE=n             features of a tile of the LDS histogram (QNT_STATE_MAX / slots at most).
// Features pass through the workspace a group at a time: QNT_HIST_BYTES of global histograms at most.
static constexpr size_t QNT_PACK_BYTES = (size_t)256 << 20;
static constexpr size_t QNT_HIST_BYTES = (size_t)32 << 20;
static int g_qnt_ring_passes = 0, g_qnt_packed_passes = 0;
static int quantiles_run(const char* who, hipStream_t st, void** ws, size_t* ws_bytes, EssSrc src, const unsigned int* d_nhist, bool wrapped, int W, int nfeat,
                         int nrows, int nq, const double* probs, double* q, double* x_lo, double* x_hi, int64_t* count) {
  const int64_t N = (int64_t)W * nrows;
  // the ranks asked for, and the distinct ones among them in ascending order: the slots
  std::vector<long long> lo_of((size_t)nq), hi_of((size_t)nq), ranks;
  std::vector<double> g_of((size_t)nq);
  for (int k = 0; k < nq; ++k) {
    const double h = (double)(N - 1) * probs[k], fl = std::floor(h);
    lo_of[(size_t)k] = (long long)fl;
    hi_of[(size_t)k] = std::min(lo_of[(size_t)k] + 1, (long long)N - 1);
    g_of[(size_t)k] = h - fl;
    ranks.push_back(lo_of[(size_t)k]);
    ranks.push_back(hi_of[(size_t)k]);
  }
  std::sort(ranks.begin(), ranks.end());
  ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
  const int ns = (int)ranks.size();
  auto slot_of = [&](long long r) { return (size_t)(std::lower_bound(ranks.begin(), ranks.end(), r) - ranks.begin()); };
  auto env_ll = [](const char* name) { const char* v = getenv(name); return v && *v ? atoll(v) : 0ll; };
  const char* path = getenv("PTM_QUANTILES_PATH");
  const bool forced = path && *path, pack = forced && !strcmp(path, "packed");
  if (forced && !pack && strcmp(path, "ring")) return fail(PTM_ERR_INVALID, "%s: PTM_QUANTILES_PATH must be ring or packed", who);
  const int ft_max = QNT_STATE_MAX / ns;
  const long long tile_forced = env_ll("PTM_QUANTILES_TILE");
  const int ft = (int)std::max(1ll, std::min((long long)std::min(ft_max, nfeat), tile_forced > 0 ? tile_forced : (long long)ft_max));
  const size_t per_feature = (size_t)ns * QNT_BINS, fg = std::min((size_t)nfeat, std::max((size_t)1, QNT_HIST_BYTES / (per_feature * 8)));
  const long long bytes_forced = env_ll("PTM_QUANTILES_PACK_BYTES");
  const size_t pack_bytes = pack ? (bytes_forced > 0 ? std::min((size_t)bytes_forced, QNT_PACK_BYTES) : QNT_PACK_BYTES) : 0;
  const long long room = std::min((long long)(pack_bytes / (8 * fg)), (long long)N);   // positions of the copy
  const size_t o_ranks = 0, o_ao = o_ranks + ess_align((size_t)QNT_SLOTS_MAX * 8), o_hb = o_ao + ess_align(2 * fg * 8), o_prefix = o_hb + ess_align(fg * 4),
               o_rank = o_prefix + ess_align(fg * ns * 8), o_leader = o_rank + ess_align(fg * ns * 8), o_cand = o_leader + ess_align(fg * ns * 4),
               o_fill = o_cand + ess_align(fg * 8), o_hist = o_fill + ess_align(fg * 8), o_flag = o_hist + ess_align(fg * per_feature * 8), o_packed = o_flag + 256,
               total = o_packed + ess_align((size_t)std::max(room, 0ll) * fg * 8);
  if (*ws_bytes < total) {
    if (*ws) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(*ws)); *ws = nullptr; *ws_bytes = 0; }
    HIPCHK(hipMalloc(ws, total));
    *ws_bytes = total;
  }
  // (every call: the attribute belongs to the current device, and a series call may name another one)
  HIPCHK(hipFuncSetAttribute((const void*)quantiles_count_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, QNT_LDS_BYTES));
  HIPCHK(hipFuncSetAttribute((const void*)quantiles_count_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, QNT_LDS_BYTES));
  unsigned char* b = (unsigned char*)*ws;
  int* d_flag = (int*)(b + o_flag);
  qnt_u64* d_fill = (qnt_u64*)(b + o_fill);
  qnt_u64* d_packed = (qnt_u64*)(b + o_packed);
  HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
  HIPCHK(hipMemcpyAsync(b + o_ranks, ranks.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st));
  std::vector<qnt_u64> keys((size_t)nfeat * ns);
  std::vector<int> hb;
  std::vector<long long> cand;
  const dim3 T(QNT_THREADS);
  // the grid of a walk: lanes (walkers x features of a tile), chunks of rows (about 2048 workgroups in all), tiles
  auto grid_of = [&](QntWalk* k) {
    const unsigned tiles = (unsigned)((k->nf + k->ft - 1) / k->ft);
    const unsigned bx = (unsigned)(((size_t)k->W * std::min(k->ft, k->nf) + QNT_THREADS - 1) / QNT_THREADS);
    long long chunks = std::max(1ll, std::min({(long long)k->nrows, 65535ll, 2048ll / ((long long)bx * tiles)}));
    k->rows_per_chunk = (int)((k->nrows + chunks - 1) / chunks);
    chunks = (k->nrows + (long long)k->rows_per_chunk - 1) / k->rows_per_chunk;
    return dim3(bx, (unsigned)chunks, tiles);
  };
  int ring_passes = 0, packed_passes = 0;
  for (size_t f0 = 0; f0 < (size_t)nfeat; f0 += fg) {
    const int nf = (int)std::min(fg, (size_t)nfeat - f0);
    QntState s;
    s.ranks = (const long long*)(b + o_ranks); s.and_or = (qnt_u64*)(b + o_ao); s.hb = (int*)(b + o_hb); s.prefix = (qnt_u64*)(b + o_prefix);
    s.rank = (long long*)(b + o_rank); s.leader = (int*)(b + o_leader); s.hist = (qnt_u64*)(b + o_hist); s.cand = (long long*)(b + o_cand);
    s.nf = nf; s.ns = ns;
    HIPCHK(hipMemsetAsync(s.and_or, 0xFF, (size_t)nf * 8, st));
    HIPCHK(hipMemsetAsync(s.and_or + nf, 0, (size_t)nf * 8, st));
    HIPCHK(hipMemsetAsync(s.hist, 0, (size_t)nf * per_feature * 8, st));
    QntWalk ring;
    ring.src = src; ring.nhist = d_nhist; ring.valid = nullptr; ring.room = 0; ring.W = W; ring.f0 = (int)f0; ring.nf = nf; ring.ft = ft; ring.nrows = nrows;
    const dim3 ring_grid = grid_of(&ring);
    if (wrapped) hipLaunchKernelGGL(quantiles_bits_kernel<true>, ring_grid, T, 0, st, ring, s.and_or, d_flag);
    else hipLaunchKernelGGL(quantiles_bits_kernel<false>, ring_grid, T, 0, st, ring, s.and_or, d_flag);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(quantiles_update_kernel, dim3((unsigned)nf), dim3(QNT_SLOTS_MAX), 0, st, s, -1, d_flag);
    HIPCHK(hipGetLastError());
    int flag = 0;
    hb.resize((size_t)nf);
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hb.data(), s.hb, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (flag) return fail(PTM_ERR_INVALID, "%s: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", who, src.cap, nrows);
    int npass = 0;
    for (int f = 0; f < nf; ++f)
      if (hb[(size_t)f] >= 0) npass = std::max(npass, hb[(size_t)f] / QNT_BITS + 1);
    QntWalk cur = ring;
    dim3 cur_grid = ring_grid;
    bool packed = false;
    for (int p = 0; p < npass; ++p) {
      const size_t lds = (size_t)std::min(cur.ft, nf) * per_feature * 4;
      if (wrapped && !packed) hipLaunchKernelGGL(quantiles_count_kernel<true>, cur_grid, T, lds, st, cur, s, p, d_flag);
      else hipLaunchKernelGGL(quantiles_count_kernel<false>, cur_grid, T, lds, st, cur, s, p, d_flag);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(quantiles_update_kernel, dim3((unsigned)nf), dim3(QNT_SLOTS_MAX), 0, st, s, p, d_flag);
      HIPCHK(hipGetLastError());
      ++(packed ? packed_passes : ring_passes);
      if (packed || room < 1 || p + 1 >= npass) continue;
      // do the candidates fit the copy?
      cand.resize((size_t)nf);
      HIPCHK(hipMemcpyAsync(cand.data(), s.cand, (size_t)nf * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const long long cmax = *std::max_element(cand.begin(), cand.end());
      if (cmax < 1 || cmax > room) continue;
      HIPCHK(hipMemsetAsync(d_fill, 0, (size_t)nf * 8, st));
      if (wrapped) hipLaunchKernelGGL(quantiles_pack_kernel<true>, ring_grid, T, 0, st, ring, s, p + 1, d_fill, room, d_packed, d_flag);
      else hipLaunchKernelGGL(quantiles_pack_kernel<false>, ring_grid, T, 0, st, ring, s, p + 1, d_fill, room, d_packed, d_flag);
      HIPCHK(hipGetLastError());
      const long long rows = (cmax + QNT_PACK_WALKERS - 1) / QNT_PACK_WALKERS;
      cur.src.x = (const double*)d_packed; cur.src.meta = nullptr;
      cur.src.slot_stride = (long long)QNT_PACK_WALKERS * nf; cur.src.meta_stride = 0; cur.src.series_stride = nf;
      cur.src.cap = (int)rows; cur.src.add_every = 1; cur.src.first_row = 0; cur.src.permuted = 0; cur.src.steps = (int)rows;
      cur.nhist = nullptr; cur.valid = (const long long*)d_fill; cur.room = room; cur.W = QNT_PACK_WALKERS; cur.f0 = 0; cur.nrows = (int)rows;
      cur_grid = grid_of(&cur);
      packed = true;
    }
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(keys.data() + f0 * ns, s.prefix, (size_t)nf * ns * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (flag == 1) return fail(PTM_ERR_INVALID, "%s: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", who, src.cap, nrows);
    if (flag) return fail(PTM_ERR_HIP, "%s: the selection lost a rank (an error of the kernels)", who);
  }
  g_qnt_ring_passes = ring_passes; g_qnt_packed_passes = packed_passes;
  auto value_of = [&](int f, size_t slot) {
    const qnt_u64 u = quantiles_unkey(keys[(size_t)f * ns + slot]);
    double v;
    memcpy(&v, &u, 8);
    return v;
  };
  for (int k = 0; k < nq; ++k) {
    const size_t sl = slot_of(lo_of[(size_t)k]), sh = slot_of(hi_of[(size_t)k]);
    const double g = g_of[(size_t)k];
    for (int f = 0; f < nfeat; ++f) {
      const double a = value_of(f, sl), c = value_of(f, sh);
      volatile double step = g * (c - a);   // (the product rounded before the sum, whatever the compiler's contraction rule)
      q[(size_t)k * nfeat + f] = g == 0 ? a : a + step;
      if (x_lo) x_lo[(size_t)k * nfeat + f] = a;
      if (x_hi) x_hi[(size_t)k * nfeat + f] = c;
    }
  }
  if (count) *count = N;
  return PTM_OK;
}
static int quantiles_shape(const char* who, int nfeat_max, int nfeat, int nrows, int nq, const double* probs) {
  if (nfeat < 1 || nfeat > nfeat_max) return fail(PTM_ERR_INVALID, "%s: nfeat must be in 1..%d", who, nfeat_max);
  if (nrows < 1) return fail(PTM_ERR_INVALID, "%s: nrows must be at least 1", who);
  if (nq < 1 || nq > QNT_SLOTS_MAX / 2) return fail(PTM_ERR_INVALID, "%s: nq must be in 1..%d", who, QNT_SLOTS_MAX / 2);
  for (int k = 0; k < nq; ++k)
    if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return fail(PTM_ERR_INVALID, "%s: probability %d is outside [0, 1]", who, k);
  return PTM_OK;
}
extern "C" int ptm_quantiles(ptm_engine* e, int rung, int nfeat, int nrows, int nq, const double* probs, double* q, double* x_lo, double* x_hi, int64_t* count) {
  if (!e || !probs || !q) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_quantiles");
  int rc = quantiles_shape("ptm_quantiles", e->D, nfeat, nrows, nq, probs);
  if (rc) return rc;
  EssSrc src;
  std::vector<int> steps_of;
  if ((rc = ess_ring_source(e, rung, nfeat, &src, &steps_of))) return rc;   // (settles a pending ladder launch and the uncounted adds first)
  if ((double)e->W * nfeat > 2.0e9 || (double)e->W * nrows > 9.0e15) return fail(PTM_ERR_INVALID, "ptm_quantiles: bad shape");
  long long newest_min = 0, newest_max = 0;
  for (int w = 0; w < e->W; ++w) {
    const long long st = steps_of.empty() ? src.steps : steps_of[(size_t)w];
    const long long newest = st > 0 ? 1 + (st - 1) / src.add_every : 0;   // (= the saved rows behind the start state)
    if (!w || newest < newest_min) newest_min = newest;
    if (!w || newest > newest_max) newest_max = newest;
  }
  if (newest_min < nrows) return fail(PTM_ERR_INVALID, "ptm_quantiles: a chain of the rung has saved %lld rows behind its start state, fewer than nrows (%d)", newest_min, nrows);
  if (nrows > src.cap) return fail(PTM_ERR_INVALID, "ptm_quantiles: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", src.cap, nrows);
  return quantiles_run("ptm_quantiles", e->stream, &e->ess_ws, &e->ess_ws_bytes, src, e->nhist + (size_t)rung * e->W, newest_max >= (long long)src.cap, e->W, nfeat, nrows,
                       nq, probs, q, x_lo, x_hi, count);
}
extern "C" int ptm_quantiles_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, int nq, const double* probs, double* q,
                                    double* x_lo, double* x_hi, int64_t* count) {
  if (!probs || !q || !series) return fail(PTM_ERR_INVALID, "null argument");
  int rc = quantiles_shape("ptm_quantiles_series", 2000000000, nfeat, nrows, nq, probs);
  if (rc) return rc;
  if ((int64_t)nrows > n) return fail(PTM_ERR_INVALID, "ptm_quantiles_series: the series have %lld rows, fewer than nrows (%d)", (long long)n, nrows);
  if (n > 2000000000 || nseries < 1 || (double)nseries * nfeat > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_quantiles_series: bad shape");
  for (size_t i = 0, end = (size_t)n * nseries * nfeat; i < end; ++i)   // (before anything is queued; infinities are values like any other)
    if (series[i] != series[i]) return fail(PTM_ERR_INVALID, "ptm_quantiles_series: the series hold a NaN (row %lld)", (long long)(i / ((size_t)nseries * nfeat)));
  EssSeries S;
  if ((rc = ess_series_source(&S, device, series, n, nseries, nfeat))) return rc;
  return quantiles_run("ptm_quantiles_series", nullptr, &S.ws, &S.ws_bytes, S.src, nullptr, false, nseries, nfeat, nrows, nq, probs, q, x_lo, x_hi, count);
}
extern "C" int ptm_quantiles_last_path(int* ring_passes, int* packed_passes) {
  if (ring_passes) *ring_passes = g_qnt_ring_passes;
  if (packed_passes) *packed_passes = g_qnt_packed_passes;
  return g_qnt_packed_passes > 0 ? 1 : 0;
}

// ---- corner-plot histograms of a rung on the device (ptm_histograms_kernels.hpp) ---------------------------------------------
// histogram_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) on the ring where it lies, or on a caller's series.  d_nhist, wrapped: as
// rhat_run's.  The caller's arrays are filled only when no row of a window was missing.
// Forceable from the environment (tests, the probe); the counts do not depend on them:
//   PTM_HIST_TILE=n          pairs of a tile of the 2-D kernel's LDS tables (what HIST_TABLE_BYTES hold at most)
//   PTM_HIST_MAP=pairs|rows  how the 2-D kernel deals its adds to the lanes (pairs: the default)
static int g_hist_tile = 0, g_hist_tiles = 0, g_hist_map = 0;
// the ranges as the kernels read them, [HIST_PAR * f]: lo, hi, step, nbins / (hi - lo); refuses what the definition refuses
static int histograms_shape(const char* who, int nfeat_max, int nfeat, int nrows, int nbins, const double* lo, const double* hi, bool pairs, std::vector<double>* par) {
  if (nfeat < 1 || nfeat > nfeat_max) return fail(PTM_ERR_INVALID, "%s: nfeat must be in 1..%d", who, nfeat_max);
  if (nrows < 1) return fail(PTM_ERR_INVALID, "%s: nrows must be at least 1", who);
  if (nbins < 1 || nbins > HIST_BINS_MAX) return fail(PTM_ERR_INVALID, "%s: nbins must be in 1..%d", who, HIST_BINS_MAX);
  par->resize((size_t)HIST_PAR * nfeat);
  for (int f = 0; f < nfeat; ++f) {
    const double a = lo[f], b = hi[f];
    if (!(std::isfinite(a) && std::isfinite(b) && a < b)) return fail(PTM_ERR_INVALID, "%s: the range of feature %d is not finite with lo < hi", who, f);
    const double width = b - a, step = width / (double)nbins;
    bool ok = std::isfinite(step);
    for (int k = 0; ok && k < nbins; ++k) {
      const double e0 = histograms_edge(a, b, step, nbins, k), e1 = histograms_edge(a, b, step, nbins, k + 1);
      ok = std::isfinite(e0) && e0 < e1;
    }
    if (!ok) return fail(PTM_ERR_INVALID, "%s: the range cannot hold nbins bins (feature %d: the %d edges from %.17g to %.17g are not finite and strictly increasing)", who, f, nbins + 1, a, b);
    double* pf = par->data() + (size_t)HIST_PAR * f;
    pf[0] = a; pf[1] = b; pf[2] = step; pf[3] = (double)nbins / width;
  }
  if (pairs && nfeat > 1 && (double)nfeat * (nfeat - 1) / 2.0 * nbins * nbins > (double)HIST_CELLS_MAX)
    return fail(PTM_ERR_UNSUPPORTED, "%s: %d features and %d bins need more than 2^25 pair counters", who, nfeat, nbins);
  return PTM_OK;
}
static int histograms_run(const char* who, hipStream_t st, void** ws, size_t* ws_bytes, EssSrc src, const unsigned int* d_nhist, bool wrapped, int W, int nfeat,
                          int nrows, int nbins, const std::vector<double>& par, int64_t* h1, int64_t* h2, int64_t* below, int64_t* above, int64_t* count) {
  const int64_t N = (int64_t)W * nrows;
  const bool pairs = h2 && nfeat > 1;
  const long long npairs = (long long)nfeat * (nfeat - 1) / 2, nb2 = (long long)nbins * nbins;
  const size_t cells1 = (size_t)nfeat * (nbins + 2), cells2 = pairs ? (size_t)(npairs * nb2) : 0;
  auto env_ll = [](const char* name) { const char* v = getenv(name); return v && *v ? atoll(v) : 0ll; };
  const char* map_env = getenv("PTM_HIST_MAP");
  const bool map_forced = map_env && *map_env, map_rows = map_forced && !strcmp(map_env, "rows");
  if (map_forced && !map_rows && strcmp(map_env, "pairs")) return fail(PTM_ERR_INVALID, "%s: PTM_HIST_MAP must be pairs or rows", who);
  const size_t o_par = 0, o_flag = o_par + ess_align(par.size() * 8), o_h1 = o_flag + 256, o_h2 = o_h1 + ess_align(cells1 * 8), total = o_h2 + ess_align(cells2 * 8);
  if (*ws_bytes < total) {
    if (*ws) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(*ws)); *ws = nullptr; *ws_bytes = 0; }
    HIPCHK(hipMalloc(ws, total));
    *ws_bytes = total;
  }
  unsigned char* b = (unsigned char*)*ws;
  const double* d_par = (const double*)(b + o_par);
  int* d_flag = (int*)(b + o_flag);
  qnt_u64 *d_h1 = (qnt_u64*)(b + o_h1), *d_h2 = (qnt_u64*)(b + o_h2);
  HIPCHK(hipMemcpyAsync(b + o_par, par.data(), par.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_flag, 0, total - o_flag, st));   // the flag and every counter
  // the 1-D kernel: quantiles_run's grid -- lanes (walkers x features of a tile), chunks of rows, tiles
  {
    QntWalk q;
    q.src = src; q.nhist = d_nhist; q.valid = nullptr; q.room = 0; q.W = W; q.f0 = 0; q.nf = nfeat; q.ft = std::min(nfeat, HIST_FEATS); q.nrows = nrows;
    const unsigned tiles = (unsigned)((nfeat + q.ft - 1) / q.ft);
    const unsigned bx = (unsigned)(((size_t)W * q.ft + QNT_THREADS - 1) / QNT_THREADS);
    long long chunks = std::max(1ll, std::min({(long long)nrows, 65535ll, std::max(2ll * HIST_BLOCKS / ((long long)bx * tiles), ((long long)nrows * QNT_THREADS >> 31) + 1)}));
    q.rows_per_chunk = (int)((nrows + chunks - 1) / chunks);
    chunks = (nrows + (long long)q.rows_per_chunk - 1) / q.rows_per_chunk;
    const dim3 grid(bx, (unsigned)chunks, tiles);
    const size_t lds = (size_t)q.ft * (nbins + 2) * 4;
    if (wrapped) hipLaunchKernelGGL(histograms_1d_kernel<true>, grid, dim3(QNT_THREADS), lds, st, q, d_par, nbins, d_h1, d_flag);
    else hipLaunchKernelGGL(histograms_1d_kernel<false>, grid, dim3(QNT_THREADS), lds, st, q, d_par, nbins, d_h1, d_flag);
    HIPCHK(hipGetLastError());
  }
  int tile = 0, tiles = 0;
  if (pairs) {
    // tiles of pairs (grid.z), blocks of walkers (grid.x), chunks of rows (grid.y): HIST_BLOCKS workgroups, about, and fewer than
    // 2^31 samples a workgroup
    tile = HistLds::tile_pairs(nbins, npairs, env_ll("PTM_HIST_TILE"));
    if ((npairs + tile - 1) / tile > 65535) tile = (int)((npairs + 65534) / 65535);
    tiles = (int)((npairs + tile - 1) / tile);
    HistWalk q;
    q.src = src; q.nhist = d_nhist; q.W = W; q.nfeat = nfeat; q.nbins = nbins; q.nrows = nrows; q.tp = tile; q.map = map_rows ? HIST_MAP_ROWS : HIST_MAP_PAIRS; q.npairs = npairs;
    const long long bx = ((long long)W + HIST_WALKERS - 1) / HIST_WALKERS;
    long long chunks = std::max({1ll, (long long)HIST_BLOCKS / (bx * tiles), ((long long)nrows * HIST_WALKERS >> 30) + 1});
    chunks = std::min({chunks, (long long)nrows, 65535ll});
    q.rows_per_chunk = (int)((nrows + chunks - 1) / chunks);
    chunks = (nrows + (long long)q.rows_per_chunk - 1) / q.rows_per_chunk;
    const dim3 grid((unsigned)bx, (unsigned)chunks, (unsigned)tiles);
    const size_t lds = HistLds(nullptr, nfeat, nbins, tile).bytes;
    // (every call: the attribute belongs to the current device, and a series call may name another one)
    HIPCHK(hipFuncSetAttribute((const void*)histograms_2d_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HistLds(nullptr, 2, 1, HIST_PAIRS_MAX).bytes));
    HIPCHK(hipFuncSetAttribute((const void*)histograms_2d_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HistLds(nullptr, 2, 1, HIST_PAIRS_MAX).bytes));
    if (wrapped) hipLaunchKernelGGL(histograms_2d_kernel<true>, grid, dim3(HIST_THREADS), lds, st, q, d_par, d_h2, d_flag);
    else hipLaunchKernelGGL(histograms_2d_kernel<false>, grid, dim3(HIST_THREADS), lds, st, q, d_par, d_h2, d_flag);
    HIPCHK(hipGetLastError());
  }
  int flag = 0;
  std::vector<qnt_u64> c1(cells1);
  HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(c1.data(), d_h1, cells1 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag) return fail(PTM_ERR_INVALID, "%s: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", who, src.cap, nrows);
  if (pairs) {
    HIPCHK(hipMemcpyAsync(h2, d_h2, cells2 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int f = 0; f < nfeat; ++f) {
    const qnt_u64* c = c1.data() + (size_t)f * (nbins + 2);
    for (int k = 0; k < nbins; ++k) h1[(size_t)f * nbins + k] = (int64_t)c[k];
    if (below) below[f] = (int64_t)c[nbins];
    if (above) above[f] = (int64_t)c[nbins + 1];
  }
  if (count) *count = N;
  g_hist_tile = tile; g_hist_tiles = tiles; g_hist_map = map_rows ? 1 : 0;
  return PTM_OK;
}
extern "C" int ptm_histograms(ptm_engine* e, int rung, int nfeat, int nrows, int nbins, const double* lo, const double* hi, int64_t* h1, int64_t* h2, int64_t* below,
                              int64_t* above, int64_t* count) {
  if (!e || !lo || !hi || !h1) return fail(PTM_ERR_INVALID, "null argument");
  NO_BATCH(e, "ptm_histograms");
  std::vector<double> par;
  int rc = histograms_shape("ptm_histograms", e->D, nfeat, nrows, nbins, lo, hi, h2 != nullptr, &par);
  if (rc) return rc;
  EssSrc src;
  std::vector<int> steps_of;
  if ((rc = ess_ring_source(e, rung, nfeat, &src, &steps_of))) return rc;   // (settles a pending ladder launch and the uncounted adds first)
  if ((double)e->W * nfeat > 2.0e9 || (double)e->W * nrows > 9.0e15) return fail(PTM_ERR_INVALID, "ptm_histograms: bad shape");
  long long newest_min = 0, newest_max = 0;
  for (int w = 0; w < e->W; ++w) {
    const long long st = steps_of.empty() ? src.steps : steps_of[(size_t)w];
    const long long newest = st > 0 ? 1 + (st - 1) / src.add_every : 0;   // (= the saved rows behind the start state)
    if (!w || newest < newest_min) newest_min = newest;
    if (!w || newest > newest_max) newest_max = newest;
  }
  if (newest_min < nrows) return fail(PTM_ERR_INVALID, "ptm_histograms: a chain of the rung has saved %lld rows behind its start state, fewer than nrows (%d)", newest_min, nrows);
  if (nrows > src.cap) return fail(PTM_ERR_INVALID, "ptm_histograms: history_capacity must hold the window (%d rows no longer hold the newest %d saved rows of every chain)", src.cap, nrows);
  return histograms_run("ptm_histograms", e->stream, &e->ess_ws, &e->ess_ws_bytes, src, e->nhist + (size_t)rung * e->W, newest_max >= (long long)src.cap, e->W, nfeat, nrows,
                        nbins, par, h1, h2, below, above, count);
}
extern "C" int ptm_histograms_series(int device, const double* series, int64_t n, int nseries, int nfeat, int nrows, int nbins, const double* lo, const double* hi,
                                     int64_t* h1, int64_t* h2, int64_t* below, int64_t* above, int64_t* count) {
  if (!lo || !hi || !h1 || !series) return fail(PTM_ERR_INVALID, "null argument");
  std::vector<double> par;
  int rc = histograms_shape("ptm_histograms_series", 2000000000, nfeat, nrows, nbins, lo, hi, h2 != nullptr, &par);
  if (rc) return rc;
  if ((int64_t)nrows > n) return fail(PTM_ERR_INVALID, "ptm_histograms_series: the series have %lld rows, fewer than nrows (%d)", (long long)n, nrows);
  if (n > 2000000000 || nseries < 1 || (double)nseries * nfeat > 2.0e9) return fail(PTM_ERR_INVALID, "ptm_histograms_series: bad shape");
  for (size_t i = 0, end = (size_t)n * nseries * nfeat; i < end; ++i)   // (before anything is queued; infinities are values like any other)
    if (series[i] != series[i]) return fail(PTM_ERR_INVALID, "ptm_histograms_series: the series hold a NaN (row %lld)", (long long)(i / ((size_t)nseries * nfeat)));
  EssSeries S;
  if ((rc = ess_series_source(&S, device, series, n, nseries, nfeat))) return rc;
  return histograms_run("ptm_histograms_series", nullptr, &S.ws, &S.ws_bytes, S.src, nullptr, false, nseries, nfeat, nrows, nbins, par, h1, h2, below, above, count);
}
extern "C" int ptm_histograms_last_launch(int* tile_pairs, int* tiles, int* map) {
  if (tile_pairs) *tile_pairs = g_hist_tile;
  if (tiles) *tiles = g_hist_tiles;
  if (map) *map = g_hist_map;
  return g_hist_tiles;
}

// ---- exact nearest-neighbour squared distances for the k-NN KL estimator (ptm_kl_kernels.hpp) --------------------------------
// kl_estimator::one_nnd2 / all_nnd2 (ptmcmc_amd/host/ptmcmc_gpu.hh) on a caller's two sample sets.
// The number of splits of the searched set: four waves for every SIMD of the chip (a wave is KL_THREADS queries), as long as a split
// keeps four tiles.  PTM_KL_SPLITS=n forces it (tests).
static int kl_splits(long long nP, long long nQ, int cus) {
  const char* v = getenv("PTM_KL_SPLITS");
  long long s = v && *v ? atoll(v) : 0;
  if (s < 1) {
    const long long waves = (nP + KL_THREADS - 1) / KL_THREADS, want = 16ll * cus, most = (nQ + 4 * KL_TILE - 1) / (4 * KL_TILE);
    s = std::min((want + waves - 1) / waves, most);
  }
  return (int)std::max(1ll, std::min(s, 1024ll));
}
// The workspace and the stream of ptm_nn_dist2, kept from call to call (a stream costs milliseconds to make, a search of ten thousand
// points less than one): one allocation, grown when a call needs more and given back after a call that needed more than KL_KEEP_BYTES;
// a stream of its own, so that nothing waits on, or is waited on by, an engine of the same process.  One call at a time.
static const size_t KL_KEEP_BYTES = (size_t)256 << 20;
struct KlWorkspace {
  std::mutex lock;
  void* all = nullptr;
  size_t bytes = 0;
  hipStream_t st = nullptr;
  int device = -1;
  int release() {
    if (st) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipStreamDestroy(st)); st = nullptr; }
    if (all) { HIPCHK(hipFree(all)); all = nullptr; bytes = 0; }
    device = -1;
    return PTM_OK;
  }
  int reserve(int dev, size_t need) {
    int rc;
    if (device != dev && (rc = release())) return rc;
    if (!st) { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); device = dev; }
    if (bytes < need) {
      if (all) { HIPCHK(hipFree(all)); all = nullptr; bytes = 0; }
      HIPCHK(hipMalloc(&all, need));
      bytes = need;
    }
    return PTM_OK;
  }
};
static KlWorkspace g_kl;
struct KlDeviceGuard {
  int device_before = -1;   // the caller's current device, put back when the call ends
  ~KlDeviceGuard() {
    if (device_before >= 0) (void)hipSetDevice(device_before);
  }
};
template <int DP>
static void kl_launch(hipStream_t st, bool wrap, dim3 grid, const double* pt, long long nP_pad, int nP, const double* qr, int nQ, int per_split, int same_set, double* part) {
  if (wrap) hipLaunchKernelGGL((kl_nn_kernel<DP, true>), grid, dim3(KL_THREADS), 0, st, pt, nP_pad, nP, qr, nQ, per_split, same_set, part);
  else hipLaunchKernelGGL((kl_nn_kernel<DP, false>), grid, dim3(KL_THREADS), 0, st, pt, nP_pad, nP, qr, nQ, per_split, same_set, part);
}
extern "C" int ptm_nn_dist2(int device, const double* P, int64_t nP, const double* Q, int64_t nQ, int dim, const int32_t* wrapped, const double* xmin,
                            const double* xmax, int same_set, double* nnd2) {
  if (!P || !Q || !nnd2) return fail(PTM_ERR_INVALID, "null argument");
  if (dim < 1) return fail(PTM_ERR_INVALID, "ptm_nn_dist2: dim must be >= 1");
  if (nP < 1 || nQ < 1 || nP > 2000000000 || nQ > 2000000000) return fail(PTM_ERR_INVALID, "ptm_nn_dist2: nP and nQ must be in 1..2e9");
  if (same_set && (nQ != nP || nP < 2)) return fail(PTM_ERR_INVALID, "ptm_nn_dist2: same_set needs nQ == nP >= 2");
  if (dim > KL_MAX_DIM) return fail(PTM_ERR_UNSUPPORTED, "ptm_nn_dist2: dim > %d (the host estimator serves there)", KL_MAX_DIM);
  bool wrap = false;
  for (int d = 0; wrapped && d < dim; ++d)
    if (wrapped[d]) {
      if (!xmin || !xmax) return fail(PTM_ERR_INVALID, "null argument");
      if (!(xmax[d] > xmin[d]) || !std::isfinite(xmin[d]) || !std::isfinite(xmax[d])) return fail(PTM_ERR_INVALID, "ptm_nn_dist2: wrapped dimension %d needs finite xmin < xmax", d);
      wrap = true;
    }
  for (int64_t k = 0; k < nP * dim; ++k)
    if (!std::isfinite(P[k])) return fail(PTM_ERR_INVALID, "ptm_nn_dist2: P has a non-finite coordinate (point %lld)", (long long)(k / dim));
  if (!same_set || Q != P)
    for (int64_t k = 0; k < nQ * dim; ++k)
      if (!std::isfinite(Q[k])) return fail(PTM_ERR_INVALID, "ptm_nn_dist2: Q has a non-finite coordinate (point %lld)", (long long)(k / dim));
  int rc = need_device();
  if (rc) return rc;
  KlDeviceGuard B;
  std::lock_guard<std::mutex> one_call(g_kl.lock);
  if (device >= 0) {
    int cur = -1;
    HIPCHK(hipGetDevice(&cur));
    if (cur != device) { HIPCHK(hipSetDevice(device)); B.device_before = cur; }
  }
  int dev = 0, cus = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  int DP = 4;
  while (DP < dim) DP *= 2;
  const int row = kl_row(DP, wrap);
  const long long nP_pad = (nP + KL_THREADS - 1) / KL_THREADS * KL_THREADS, nQ_pad = (nQ + KL_TILE - 1) / KL_TILE * KL_TILE;
  const int splits = kl_splits(nP, nQ, cus);
  const long long per = (nQ + splits - 1) / splits;
  const int per_split = (int)std::min<long long>((per + KL_TILE - 1) / KL_TILE * KL_TILE, nQ_pad);
  // the workspace: both sets as the search wants them, both as they came, the partial minima and the answer, the bounds
  const size_t pt_bytes = ess_align((size_t)row * nP_pad * 8), qr_bytes = ess_align((size_t)nQ_pad * row * 8), rawp_bytes = ess_align((size_t)nP * dim * 8),
               rawq_bytes = ess_align((size_t)nQ * dim * 8), part_bytes = ess_align((size_t)(splits + 1) * nP * 8), bounds_bytes = ess_align((size_t)dim * 20);
  const size_t total = pt_bytes + qr_bytes + rawp_bytes + rawq_bytes + part_bytes + bounds_bytes;
  if ((rc = g_kl.reserve(dev, total))) return rc;
  const hipStream_t st = g_kl.st;
  unsigned char* base = (unsigned char*)g_kl.all;
  double *d_pt = (double*)base, *d_qr = (double*)(base + pt_bytes), *d_rawp = (double*)(base + pt_bytes + qr_bytes),
         *d_rawq = (double*)(base + pt_bytes + qr_bytes + rawp_bytes), *part = (double*)(base + pt_bytes + qr_bytes + rawp_bytes + rawq_bytes),
         *d_min = (double*)(base + pt_bytes + qr_bytes + rawp_bytes + rawq_bytes + part_bytes), *d_max = d_min + dim, *d_out = part + (size_t)splits * nP;
  int* d_wrapped = (int*)(d_max + dim);
  if (wrap) {
    HIPCHK(hipMemcpyAsync(d_min, xmin, (size_t)dim * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_max, xmax, (size_t)dim * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_wrapped, wrapped, (size_t)dim * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemsetAsync(d_pt, 0, pt_bytes + qr_bytes, st));   // (the columns and rows behind the last point are read, never used)
  HIPCHK(hipMemcpyAsync(d_rawp, P, (size_t)nP * dim * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_rawq, Q, (size_t)nQ * dim * 8, hipMemcpyHostToDevice, st));
  auto blocks = [](long long lanes) { return dim3((unsigned)((lanes + 255) / 256)); };
  hipLaunchKernelGGL(kl_prepare_kernel, blocks(nP * DP), dim3(256), 0, st, (const double*)d_rawp, (long long)nP, dim, DP, d_wrapped, d_min, d_max, d_pt, 1ll, nP_pad,
                     (long long)DP * nP_pad, wrap ? 1 : 0);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(kl_prepare_kernel, blocks(nQ * DP), dim3(256), 0, st, (const double*)d_rawq, (long long)nQ, dim, DP, d_wrapped, d_min, d_max, d_qr, (long long)row,
                     1ll, (long long)DP, wrap ? 1 : 0);
  HIPCHK(hipGetLastError());
  const dim3 grid((unsigned)(nP_pad / KL_THREADS), (unsigned)splits);
  const double *pt = d_pt, *qr = d_qr;
#define KL_CASE(N) case N: kl_launch<N>(st, wrap, grid, pt, nP_pad, (int)nP, qr, (int)nQ, per_split, same_set ? 1 : 0, part); break;
  switch (DP) {
    KL_CASE(4) KL_CASE(8) KL_CASE(16) KL_CASE(32) KL_CASE(64) KL_CASE(128)
    default: return fail(PTM_ERR_UNSUPPORTED, "ptm_nn_dist2: no kernel for %d padded dimensions", DP);
  }
#undef KL_CASE
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(kl_min_kernel, blocks(nP), dim3(256), 0, st, (const double*)part, splits, (int)nP, d_out);
  HIPCHK(hipGetLastError());
  std::vector<double> out((size_t)nP);
  HIPCHK(hipMemcpyAsync(out.data(), d_out, (size_t)nP * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (total > KL_KEEP_BYTES) { HIPCHK(hipFree(g_kl.all)); g_kl.all = nullptr; g_kl.bytes = 0; }
  std::copy(out.begin(), out.end(), nnd2);   // (the caller's array is written last, when nothing can fail any more)
  return PTM_OK;
}
extern "C" int ptm_nn_dist2_tile(void) { return KL_TILE; }

// ---- verification hooks ------------------------------------------------------------------------------------------------
extern "C" int ptm_debug_eval(int device, int fn, const double* a, const double* b, double* out, int n) {
  int rc = need_device();
  if (rc) return rc;
  if (device >= 0) HIPCHK(hipSetDevice(device));
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  HIPCHK(hipMalloc((void**)&da, (size_t)n * 8));
  HIPCHK(hipMalloc((void**)&db, (size_t)n * 8));
  HIPCHK(hipMalloc((void**)&dout, (size_t)n * 8));
  HIPCHK(hipMemcpy(da, a, (size_t)n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db, b ? b : a, (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(debug_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, fn, da, db, dout, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost));
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
  return PTM_OK;
}

extern "C" int ptm_debug_philox(int device, uint64_t seed, int tag, uint32_t stream, uint64_t step, uint32_t block, uint32_t out[4]) {
  int rc = need_device();
  if (rc) return rc;
  if (device >= 0) HIPCHK(hipSetDevice(device));
  uint32_t* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, 16));
  hipLaunchKernelGGL(debug_philox_kernel, dim3(1), dim3(1), 0, 0, seed, tag, stream, step, block, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d, 16, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return PTM_OK;
}

extern "C" int ptm_debug_boxmuller(int device, const uint32_t* k1, const uint32_t* k2, double* z0, double* z1, int n) {
  int rc = need_device();
  if (rc) return rc;
  if (device >= 0) HIPCHK(hipSetDevice(device));
  uint32_t *d1 = nullptr, *d2 = nullptr;
  double *o0 = nullptr, *o1 = nullptr;
  HIPCHK(hipMalloc((void**)&d1, (size_t)n * 4));
  HIPCHK(hipMalloc((void**)&d2, (size_t)n * 4));
  HIPCHK(hipMalloc((void**)&o0, (size_t)n * 8));
  HIPCHK(hipMalloc((void**)&o1, (size_t)n * 8));
  HIPCHK(hipMemcpy(d1, k1, (size_t)n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d2, k2, (size_t)n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(debug_boxmuller_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d1, d2, o0, o1, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(z0, o0, (size_t)n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(z1, o1, (size_t)n * 8, hipMemcpyDeviceToHost));
  (void)hipFree(d1); (void)hipFree(d2); (void)hipFree(o0); (void)hipFree(o1);
  return PTM_OK;
}

extern "C" int ptm_debug_sqrt_scan(int device, uint64_t* mismatches) {
  int rc = need_device();
  if (rc) return rc;
  if (!mismatches) return fail(PTM_ERR_INVALID, "null argument");
  if (device >= 0) HIPCHK(hipSetDevice(device));
  unsigned long long* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, 16));
  HIPCHK(hipMemset(d, 0, 16));
  hipLaunchKernelGGL(debug_sqrt_scan_kernel, dim3(256 * 16), dim3(256), 0, 0, d);
  HIPCHK(hipGetLastError());
  unsigned long long v[2] = {0, 0};
  HIPCHK(hipMemcpy(v, d, 16, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  *mismatches = v[0] + v[1];   // arguments where bm_sqrt is not the correctly rounded root + arguments outside its domain
  return PTM_OK;
}

extern "C" int ptm_debug_boxmuller_f32_scan(int device, double out[8]) {
  int rc = need_device();
  if (rc) return rc;
  if (!out) return fail(PTM_ERR_INVALID, "null argument");
  if (device >= 0) HIPCHK(hipSetDevice(device));
  unsigned long long* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, 48));
  HIPCHK(hipMemset(d, 0, 48));
  hipLaunchKernelGGL(debug_boxmuller_f32_scan_kernel, dim3(256 * 16), dim3(256), 0, 0, 0, d);
  hipLaunchKernelGGL(debug_boxmuller_f32_scan_kernel, dim3(256 * 16), dim3(256), 0, 0, 1, d + 3);
  HIPCHK(hipGetLastError());
  unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpy(v, d, 48, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  double w[6];
  memcpy(w, v, sizeof w);   // (the maxima are bit patterns of doubles)
  out[0] = w[0]; out[1] = w[1]; out[2] = (double)v[2];   // radius: max |r_f32 - r|, max r_f32, NaNs
  out[3] = w[3]; out[4] = (double)v[5];                  // sine and cosine: max difference, NaNs
  out[5] = PTM_BP_DZ; out[6] = PTM_BP_F32_SLACK; out[7] = 0.0;
  return PTM_OK;
}

extern "C" int ptm_debug_evaluate(ptm_engine* e, const double* X, int n, int32_t* valid, double* Xe, double* lprior, double* llike) {
  if (!e || !X || n < 1) return fail(PTM_ERR_INVALID, "bad argument");
  const size_t D = e->D, DP = e->DP;
  std::vector<double> rows = pad_rows(X, (size_t)n, D, DP);
  double *dx = nullptr, *dlp = nullptr, *dll = nullptr;
  int* dv = nullptr;
  HIPCHK(hipMalloc((void**)&dx, (size_t)n * DP * 8));
  HIPCHK(hipMalloc((void**)&dlp, (size_t)n * 8));
  HIPCHK(hipMalloc((void**)&dll, (size_t)n * 8));
  HIPCHK(hipMalloc((void**)&dv, (size_t)n * 4));
  HIPCHK(hipMemcpy(dx, rows.data(), (size_t)n * DP * 8, hipMemcpyHostToDevice));
  int rc = run_eval(e, n, dx, dv, dlp, dll, (e->have_target && !user_like(e)) ? 1 : 0);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(rows.data(), dx, (size_t)n * DP * 8, hipMemcpyDeviceToHost));
  if (Xe) unpad_rows(rows, (size_t)n, D, DP, Xe);
  if (valid) HIPCHK(hipMemcpy(valid, dv, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (lprior) HIPCHK(hipMemcpy(lprior, dlp, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (lprior && e->dprior) {   // the device prior's log-priors of the enforced states that are valid
    std::vector<double> xe((size_t)n * D);
    std::vector<int32_t> hv((size_t)n);
    unpad_rows(rows, (size_t)n, D, DP, xe.data());
    HIPCHK(hipMemcpy(hv.data(), dv, (size_t)n * 4, hipMemcpyDeviceToHost));
    if ((rc = devprior_debug(e, xe.data(), n, hv.data(), lprior))) return rc;
  }
  if (llike && e->have_target && !user_like(e)) HIPCHK(hipMemcpy(llike, dll, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (llike && e->dfn) {   // the device likelihood's llikes of the enforced states
    std::vector<double> xe((size_t)n * D);
    unpad_rows(rows, (size_t)n, D, DP, xe.data());
    if ((rc = devlike_debug(e, xe.data(), n, llike))) return rc;
  }
  (void)hipFree(dx); (void)hipFree(dlp); (void)hipFree(dll); (void)hipFree(dv);
  return PTM_OK;
}
